// Common host/device helpers for libdeepinv_amd (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/deepinv_amd.h"

// blur.hip's 80 KB of static LDS, the packed-fp32 inline assembly and the MFMA forms used here exist on gfx950 only
#if defined(__HIP_DEVICE_COMPILE__) && !defined(DINV_EMU) && !defined(__gfx950__)
#error "libdeepinv_amd device code is written for gfx950 only: build with --offload-arch=gfx950"
#endif

// dynamic LDS of a kernel as a typed pointer (the host emulation used by the CPU tests supplies its own definition)
#ifndef DINV_DYN_LDS
#define DINV_DYN_LDS(T, name)                                                   \
    extern __shared__ __attribute__((aligned(16))) unsigned char name##_raw[];  \
    T* name = reinterpret_cast<T*>(name##_raw)
#endif

namespace dinv {

// ---------------------------------------------------------------- error handling
inline char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

#define DINV_CHECK_HIP(expr)                                                              \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return ::dinv::fail(100 + (int)_e, "%s failed: %s (%s:%d)", #expr,            \
                                hipGetErrorString(_e), __FILE__, __LINE__);               \
    } while (0)

#define DINV_CHECK_LAUNCH()                                                               \
    do {                                                                                  \
        hipError_t _e = hipGetLastError();                                                \
        if (_e != hipSuccess)                                                             \
            return ::dinv::fail(100 + (int)_e, "kernel launch failed: %s (%s:%d)",        \
                                hipGetErrorString(_e), __FILE__, __LINE__);               \
    } while (0)

#define DINV_REQUIRE(cond, ...)                                                           \
    do {                                                                                  \
        if (!(cond)) return ::dinv::fail(2, __VA_ARGS__);                                 \
    } while (0)

constexpr int kErrArg = 2;

// ---------------------------------------------------------------- the host side of the DINV_CDENSE_* epilogues
// (dinv_cdense_apply, dinv_cstructured_apply, dinv_ptycho_apply; `op` prefixes the message)
inline bool needs_aux(int epilogue) { return epilogue == DINV_CDENSE_WEIGHT || epilogue == DINV_CDENSE_AMPLITUDE; }

inline int check_epilogue(const char* op, int epilogue) {
    DINV_REQUIRE(epilogue >= DINV_CDENSE_NONE && epilogue <= DINV_CDENSE_AMPLITUDE, "%s: unknown epilogue %d", op, epilogue);
    return 0;
}

// the epilogues that read `aux` need it, and not as the output; `what` says which real array it is
inline int check_aux(const char* op, int epilogue, const void* aux, const void* out, const char* what) {
    DINV_REQUIRE(!needs_aux(epilogue) || (aux && aux != out), "%s: epilogue %d needs a real array %s that is not the output", op,
                 epilogue, what);
    return 0;
}

// ---------------------------------------------------------------- small device math
__host__ __device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__host__ __device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__host__ __device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
// a * conj(b)
__host__ __device__ __forceinline__ float2 cmulc(float2 a, float2 b) {
    return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__host__ __device__ __forceinline__ float2 cscale(float2 a, float s) { return make_float2(a.x * s, a.y * s); }

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------- launch-side resources
constexpr size_t kMaxLdsBytes = 160 * 1024;        // LDS of one compute unit: the most a workgroup can be given
constexpr size_t kDefaultLdsBytes = 48 * 1024;     // a launch that asks for more dynamic LDS than this needs its kernel's cap raised

inline int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return dev;
}

// Allow `Kernel` up to `cap` bytes of dynamic LDS: one runtime call per (kernel, device), later calls only read a mask.  `cap` is
// the most that instantiation ever asks for (a compile-time size, or kMaxLdsBytes) and not the size of one launch: the cap is a
// permission and costs no occupancy, the launch's own bytes do.  The mask is a static of this template, which is keyed on the
// kernel's address and not on its type, so instantiations that share a signature (fft_rows_kernel<Io, true / false>) each have one.
template <auto Kernel>
inline int raise_lds_cap(size_t cap) {
    static std::atomic<uint64_t> raised{0};
    const uint64_t bit = 1ull << (current_device() & 63);
    if (raised.load(std::memory_order_relaxed) & bit) return 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap);
    if (e != hipSuccess) return fail(100 + (int)e, "hipFuncSetAttribute(lds=%zu): %s", cap, hipGetErrorString(e));
    raised.fetch_or(bit, std::memory_order_relaxed);
    return 0;
}

// compute units of the current device (256 on MI355X), cached per device
inline int compute_units() {
    static std::atomic<int> cache[64];
    const int dev = current_device();
    int v = cache[dev & 63].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 256;
        cache[dev & 63].store(v, std::memory_order_relaxed);
    }
    return v;
}

}  // namespace dinv
