// TEST INFRASTRUCTURE: the launch log of the emulation.  hipLaunchKernelGGL (include/hip/hip_runtime.h) records the spelling of
// every kernel expression it launches, in order, so that a test can assert which kernel a call of the C ABI reached.
#include <string>
#include <vector>

namespace {
std::vector<std::string> g_launches;
}

extern "C" void dinv_emu_log_launch(const char* kernel) { g_launches.emplace_back(kernel); }
extern "C" void dinv_emu_launch_log_reset() { g_launches.clear(); }
extern "C" int dinv_emu_launch_log_count() { return (int)g_launches.size(); }
extern "C" const char* dinv_emu_launch_log_name(int i) {
    return i >= 0 && i < (int)g_launches.size() ? g_launches[i].c_str() : nullptr;
}
