// TEST INFRASTRUCTURE: one kernel and one launcher for tests/test_emu_lds_optin.py to check the emulation's own enforcement of
// the dynamic-LDS opt-in (include/hip/hip_runtime.h) with no product kernel involved.
#include "common.hpp"

static_assert(dinv::kDefaultLdsBytes <= emu::kDefaultDynLds, "the launchers opt in no later than the emulation (and the runtime) requires");

namespace {
__global__ void lds_probe_kernel(int* out, int last) {
    DINV_DYN_LDS(int, lds);
    if (threadIdx.x == 0) {
        lds[last] = 7;
        *out = lds[last];
    }
}
}  // namespace

// one launch with `bytes` of dynamic LDS; opt_in = 0 is a launch path that forgot dinv::raise_lds_cap
extern "C" int dinv_emu_lds_probe(int* out, size_t bytes, int opt_in) {
    if (opt_in)
        if (int e = dinv::raise_lds_cap<lds_probe_kernel>(dinv::kMaxLdsBytes)) return e;
    hipLaunchKernelGGL(lds_probe_kernel, dim3(1), dim3(64), bytes, nullptr, out, (int)(bytes / 4) - 1);
    DINV_CHECK_LAUNCH();
    return 0;
}
