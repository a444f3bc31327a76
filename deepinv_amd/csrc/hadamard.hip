// Fast Walsh-Hadamard transform on hand-written kernels (gfx950) and the fused operators of SinglePixelCamera.
//
// Replaces the ATen launches behind
//   hadamard_1d / hadamard_2d                deepinv/physics/singlepixel.py:9-43 (log2(n) rounds of torch.cat over strided slices
//                                            and two transposes: 2 log2(H W) passes through HBM per 2-D transform)
//   SinglePixelCamera (fast=True)            deepinv/physics/singlepixel.py:408-439 V / V_adjoint with DecomposablePhysics'
//                                            A / A_adjoint / A_adjoint_A / A_A_adjoint / prox_l2 / A_dagger
//                                            (deepinv/physics/forward.py:1080-1117, 1212-1252)
//
// The transform is in natural (Sylvester) order, where H_H (x) H_W = H_{HW}: the 2-D transform of an [H, W] plane IS the 1-D
// transform of its n = H W contiguous floats, a butterfly on every bit of the flat index.  No transpose is needed, and since the
// butterflies of different bits commute, any subset of bits can be done wherever the data happens to be.
//
// One kernel, hadamard_tile_kernel, in two address maps:
//   chunk   a workgroup owns Nt contiguous floats (one plane of up to 2^14 floats, or a group of smaller planes) in LDS and
//           runs the butterflies of the index bits below log2(chunk).  Planes of up to 2^14 floats (128 x 128) are RESIDENT: one
//           launch, one read and one write of the plane.
//   strip   for larger planes, a workgroup owns R = n / 2^14 rows of the plane seen as [R, 2^14] over a strip of 2^14 / R
//           columns (>= 1 KB contiguous per row) and runs the butterflies of the high bits.
// A TWO-PASS transform is chunk then strip; an operator with two transforms is chunk, strip (high bits of the first transform,
// the symbol, high bits of the second transform from the same LDS tile), chunk.  Every pass reads its whole tile before it
// writes it, so the passes after the first run in place on `out` and no workspace is needed.
//
// In LDS the butterflies run in rounds of up to four bits: a thread reads the 16 values that differ in those bits, combines
// them in registers and writes them back, one barrier per round (four rounds for a resident 128 x 128 plane).  Logical index i
// lives at i + 4 (i >> 6): the pad keeps 16-byte alignment and spreads the strided reads of the low-bit rounds over the banks.
// Plain adds and subtracts in a fixed order: no atomics, bit-reproducible.
#include "common.hpp"

#include <cmath>

using namespace dinv;

namespace {

constexpr int kMaxThreads = 512;
constexpr int kTileLog2 = 14;                     // floats of LDS per workgroup (64 KB + pad); two workgroups per CU

__host__ __device__ __forceinline__ int phys(int i) { return i + ((i >> 6) << 2); }
inline size_t lds_bytes(int nt) { return (size_t)phys(nt) * sizeof(float) + 16; }

// symbol modes (DINV_HAD_SYM / DINV_HAD_PRE of the header)
enum : int { kSymNone = 0, kSymMask = 1, kSymMask2 = 2, kSymProx = 3, kSymProxAdjY = 4, kSymDagger = 5 };

struct Pass {
    int64_t total;        // floats of the whole tensor
    int64_t n;            // floats per plane
    int64_t mask_period;  // floats of the mask (mask_planes * n)
    int nt;               // floats per tile
    int lo, hi;           // the butterflies of tile-index bits [lo, hi) run here
    int strip;            // 0 chunk, 1 strip
    int wd_log2;          // strip: log2 of the strip width;  row stride is 1 << kTileLog2-or-override (row_log2)
    int row_log2;
    int strips_log2;      // strip: log2 of strips per plane
    int pre, sym, second; // symbol before the butterflies, after them, and whether they run again after the symbol
    int sym_at_store;     // the symbol is applied at the store (one transform) rather than in LDS (two)
    float a;              // multiplies the transform's value inside the symbol
    float ginv;           // 1 / gamma of the prox symbols
    float oscale;         // multiplies what is stored
};

__device__ __forceinline__ float dagger_inv(float m) { return m > 1e-5f ? 1.0f / m : 0.0f; }

__device__ __forceinline__ float apply_sym(int mode, float v, float a, float ginv, const float* __restrict__ mask,
                                           const float* __restrict__ y, int64_t g, int64_t mi) {
    v *= a;
    switch (mode) {
        case kSymMask: return mask[mi] * v;
        case kSymMask2: { const float m = mask[mi]; return (m * m) * v; }
        case kSymProx: { const float m = mask[mi]; return ((y ? m * y[g] : 0.0f) + v * ginv) / (m * m + ginv); }
        case kSymProxAdjY: { const float m = mask[mi]; return m * v / (m * m + ginv); }
        case kSymDagger: return v * dagger_inv(mask[mi]);
        default: return v;
    }
}

// global float offset of tile-local index i (a multiple of 4; the 4 floats are contiguous in both maps)
__device__ __forceinline__ int64_t global_of(const Pass& p, int64_t tile, int i) {
    if (!p.strip) return tile * p.nt + i;
    const int64_t plane = tile >> p.strips_log2;
    const int64_t strip = tile & (((int64_t)1 << p.strips_log2) - 1);
    const int r = i >> p.wd_log2, c = i & ((1 << p.wd_log2) - 1);
    return plane * p.n + ((int64_t)r << p.row_log2) + (strip << p.wd_log2) + c;
}

template <int R>
__device__ __forceinline__ void fwht_round(float* __restrict__ t, int nt, int b) {
    constexpr int M = 1 << R;
    for (int j = threadIdx.x; j < (nt >> R); j += blockDim.x) {
        const int base = ((j >> b) << (b + R)) | (j & ((1 << b) - 1));
        float v[M];
#pragma unroll
        for (int k = 0; k < M; ++k) v[k] = t[phys(base + (k << b))];
#pragma unroll
        for (int s = 1; s < M; s <<= 1) {
#pragma unroll
            for (int k = 0; k < M; ++k) {
                if (!(k & s)) {
                    const float u = v[k], w = v[k | s];
                    v[k] = u + w;
                    v[k | s] = u - w;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < M; ++k) t[phys(base + (k << b))] = v[k];
    }
    __syncthreads();
}

// the butterflies of bits [lo, hi) of the tile index, four bits a round (5 remaining bits go 3 + 2)
__device__ __forceinline__ void fwht_bits(float* __restrict__ t, int nt, int lo, int hi) {
    int b = lo;
    while (b < hi) {
        const int rem = hi - b;
        const int r = rem > 4 ? (rem == 5 ? 3 : 4) : rem;
        if (r == 4) fwht_round<4>(t, nt, b);
        else if (r == 3) fwht_round<3>(t, nt, b);
        else if (r == 2) fwht_round<2>(t, nt, b);
        else fwht_round<1>(t, nt, b);
        b += r;
    }
}

__global__ __launch_bounds__(kMaxThreads) void hadamard_tile_kernel(Pass p, const float* x, const float* __restrict__ y,
                                                                   const float* __restrict__ mask, float* out) {
    // x and out may be the same buffer (the in-place passes): the whole tile is in LDS before anything is stored
    DINV_DYN_LDS(float, t);
    const int64_t tile = blockIdx.x;
    // load, 16 bytes a lane; floats past the end of the tensor (a partial last group of planes) read as zero
    for (int i = 4 * threadIdx.x; i < p.nt; i += 4 * blockDim.x) {
        const int64_t g = global_of(p, tile, i);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (g + 3 < p.total) {
            const float4 q = *reinterpret_cast<const float4*>(x + g);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (int k = 0; k < 4; ++k)
                if (g + k < p.total) v[k] = x[g + k];
        }
        if (p.pre != kSymNone) {
            const int64_t mi = g % p.mask_period;
            for (int k = 0; k < 4; ++k)
                if (g + k < p.total) v[k] = p.pre == kSymMask ? mask[mi + k] * v[k] : v[k] * dagger_inv(mask[mi + k]);
        }
        *reinterpret_cast<float4*>(t + phys(i)) = make_float4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
    fwht_bits(t, p.nt, p.lo, p.hi);
    if (p.second) {
        for (int i = 4 * threadIdx.x; i < p.nt; i += 4 * blockDim.x) {
            const int64_t g = global_of(p, tile, i);
            float* q = t + phys(i);
            const int64_t mi = g % p.mask_period;
            for (int k = 0; k < 4; ++k)
                if (g + k < p.total) q[k] = apply_sym(p.sym, q[k], p.a, p.ginv, mask, y, g + k, mi + k);
        }
        __syncthreads();
        fwht_bits(t, p.nt, p.lo, p.hi);
    }
    for (int i = 4 * threadIdx.x; i < p.nt; i += 4 * blockDim.x) {
        const int64_t g = global_of(p, tile, i);
        if (g >= p.total) continue;
        const float4 q = *reinterpret_cast<const float4*>(t + phys(i));
        float v[4] = {q.x, q.y, q.z, q.w};
        if (p.sym_at_store) {
            const int64_t mi = p.sym != kSymNone ? g % p.mask_period : 0;
            for (int k = 0; k < 4; ++k)
                if (g + k < p.total) v[k] = apply_sym(p.sym, v[k], p.a, p.ginv, mask, y, g + k, mi + k);
        }
        for (int k = 0; k < 4; ++k) v[k] *= p.oscale;
        if (g + 3 < p.total) {
            *reinterpret_cast<float4*>(out + g) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int k = 0; k < 4; ++k)
                if (g + k < p.total) out[g + k] = v[k];
        }
    }
}

int ilog2(int64_t v) {
    int l = 0;
    while (((int64_t)1 << l) < v) ++l;
    return l;
}
bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

int launch(const Pass& p, int64_t tiles, const float* x, const float* y, const float* mask, float* out, hipStream_t s) {
    DINV_REQUIRE(tiles > 0 && tiles < ((int64_t)1 << 31), "hadamard: too many tiles");
    const size_t lds = lds_bytes(p.nt);
    if (lds > kDefaultLdsBytes)      // the cap: the largest tile
        if (int e = raise_lds_cap<hadamard_tile_kernel>(lds_bytes(1 << kTileLog2))) return e;
    int threads = p.nt / 16;
    threads = threads < 64 ? 64 : (threads > kMaxThreads ? kMaxThreads : threads);
    hipLaunchKernelGGL(hadamard_tile_kernel, dim3((unsigned)tiles), dim3(threads), lds, s, p, x, y, mask, out);
    DINV_CHECK_LAUNCH();
    return 0;
}

// 1 / sqrt(2^l), correctly rounded (exact for even l)
float ortho_scale(int l) { return std::ldexp(l & 1 ? 0.70710678118654752440f : 1.0f, -(l >> 1)); }

// The whole operator: `planes` planes of n = 2^l floats with the butterflies of the index bits below tbits (l for the 2-D
// transform, log2 W for the last axis only).  c = log2 of the largest resident chunk.
int run(const float* x, const float* y, const float* mask, float* out, int64_t planes, int l, int tbits, int64_t mask_planes,
        int pre, int sym, int second, int ntrans, float a, float ginv, float oscale, int c, hipStream_t s) {
    Pass p{};
    const int64_t n = (int64_t)1 << l;
    p.total = planes * n;
    p.n = n;
    p.mask_period = (mask_planes > 0 ? mask_planes : 1) * n;
    p.ginv = ginv;
    if (ntrans == 0) tbits = 0;
    if (tbits <= c) {
        // resident: groups of whole planes (4096 floats a workgroup while that leaves a workgroup for every compute unit)
        int g = l < 12 ? 12 - l : 0;
        const int cus = compute_units();
        while (g > 0 && ceil_div(planes, (int64_t)1 << g) < cus) --g;
        if (l + g < 2) g = 2 - l;
        const int cl = l < c ? l : c;     // a plane wider than the chunk (last-axis transform of a large plane) is cut into chunks
        p.nt = 1 << (cl + g);
        p.lo = 0; p.hi = tbits;
        p.pre = pre; p.sym = sym; p.second = second; p.sym_at_store = !second;
        p.a = a; p.oscale = oscale;
        return launch(p, ceil_div(p.total, p.nt), x, y, mask, out, s);
    }
    // two-pass: chunks of 2^c floats (low bits), then strips over the R = 2^(l - c) rows (high bits)
    const int rl = l - c;
    DINV_REQUIRE(rl <= kTileLog2 - 2, "hadamard: plane too large for the two-pass form");
    Pass lo_pass = p;
    lo_pass.nt = 1 << c; lo_pass.lo = 0; lo_pass.hi = c; lo_pass.sym_at_store = 1; lo_pass.a = 1.f; lo_pass.oscale = 1.f;
    Pass hi_pass = p;
    hi_pass.strip = 1;
    hi_pass.row_log2 = c;
    hi_pass.wd_log2 = (kTileLog2 - rl) < c ? (kTileLog2 - rl) : c;
    hi_pass.strips_log2 = c - hi_pass.wd_log2;
    hi_pass.nt = 1 << (hi_pass.wd_log2 + rl);
    hi_pass.lo = hi_pass.wd_log2; hi_pass.hi = hi_pass.wd_log2 + rl;
    const int64_t chunks = p.total >> c, strips = planes << hi_pass.strips_log2;
    // first pass: pre-symbol and the low bits
    lo_pass.pre = pre;
    if (int rc = launch(lo_pass, chunks, x, nullptr, mask, out, s)) return rc;
    // second pass, in place: the high bits and the symbol (and, for two transforms, the high bits again)
    hi_pass.sym = sym; hi_pass.second = second; hi_pass.sym_at_store = !second; hi_pass.a = a; hi_pass.oscale = second ? 1.f : oscale;
    if (int rc = launch(hi_pass, strips, out, y, mask, out, s)) return rc;
    if (second) {
        lo_pass.pre = kSymNone; lo_pass.oscale = oscale;
        if (int rc = launch(lo_pass, chunks, out, nullptr, mask, out, s)) return rc;
    }
    return 0;
}

int check_shape(int64_t P, int32_t H, int32_t W) {
    DINV_REQUIRE(P > 0, "hadamard: bad plane count");
    DINV_REQUIRE(pow2(H) && pow2(W), "hadamard: H and W must be powers of two (got %d x %d)", H, W);
    DINV_REQUIRE(H <= DINV_HADAMARD_MAX_SIDE && W <= DINV_HADAMARD_MAX_SIDE, "hadamard: side above %d (got %d x %d)",
                 DINV_HADAMARD_MAX_SIDE, H, W);
    DINV_REQUIRE(P * (int64_t)H * W < ((int64_t)1 << 40), "hadamard: tensor too large");
    return 0;
}

int chunk_log2(int32_t flags) {
    const int c = (flags >> 16) & 31;
    return c == 0 ? kTileLog2 : c;
}

}  // namespace

extern "C" size_t dinv_hadamard_workspace_bytes(int64_t P, int32_t H, int32_t W) {
    (void)P; (void)H; (void)W;
    return 0;   // the passes after the first run in place on `out`
}

extern "C" int dinv_hadamard(const float* x, float* out, int64_t P, int32_t H, int32_t W, int32_t flags, float scale, void* ws,
                             size_t ws_bytes, dinv_stream_t stream) {
    (void)ws; (void)ws_bytes;
    if (int rc = check_shape(P, H, W)) return rc;
    DINV_REQUIRE(x && out && aligned16(x) && aligned16(out), "hadamard: operands must be non-null and 16-byte aligned");
    const int c = chunk_log2(flags);
    DINV_REQUIRE(c >= 2 && c <= kTileLog2, "hadamard: resident chunk override must be 2..%d", kTileLog2);
    const int lw = ilog2(W), l = ilog2((int64_t)H * W);
    const bool last = flags & DINV_HAD_LAST_AXIS;
    const int tb = last ? lw : l;
    const float sc = scale * ((flags & DINV_HAD_NO_NORMALIZE) ? 1.0f : ortho_scale(tb));
    // the last-axis transform of rows is the transform of planes of W floats
    if (last) return run(x, nullptr, nullptr, out, P * H, lw, lw, 0, kSymNone, kSymNone, 0, 1, sc, 0.f, 1.f, c, (hipStream_t)stream);
    return run(x, nullptr, nullptr, out, P, l, l, 0, kSymNone, kSymNone, 0, 1, sc, 0.f, 1.f, c, (hipStream_t)stream);
}

extern "C" int dinv_hadamard_apply(const float* x, const float* y, const float* mask, float* out, int64_t P, int32_t H, int32_t W,
                                   int64_t mask_planes, int32_t flags, float add, float scale, void* ws, size_t ws_bytes,
                                   dinv_stream_t stream) {
    (void)ws; (void)ws_bytes;
    if (int rc = check_shape(P, H, W)) return rc;
    const int pre = flags & 3, sym = (flags >> 4) & 7;
    const bool second = flags & DINV_HAD_SECOND, none = flags & DINV_HAD_NO_TRANSFORM;
    DINV_REQUIRE((int64_t)H * W >= 4, "hadamard: the fused operators need planes of at least 4 pixels");
    DINV_REQUIRE(pre <= 2 && sym <= kSymDagger, "hadamard: unknown symbol mode in flags 0x%x", flags);
    DINV_REQUIRE(!(second && none) && !(second && pre), "hadamard: contradictory flags 0x%x", flags);
    DINV_REQUIRE(x && out && aligned16(x) && aligned16(out), "hadamard: operands must be non-null and 16-byte aligned");
    DINV_REQUIRE(mask && mask_planes > 0 && P % mask_planes == 0,
                 "hadamard: the mask must hold a number of planes that divides P (got %lld for P = %lld)", (long long)mask_planes,
                 (long long)P);
    DINV_REQUIRE(!y || ((const float*)out != y && sym == kSymProx), "hadamard: y is the prox symbol's second input and must not alias out");
    const int c = chunk_log2(flags);
    DINV_REQUIRE(c >= 2 && c <= kTileLog2, "hadamard: resident chunk override must be 2..%d", kTileLog2);
    const int l = ilog2((int64_t)H * W);
    const float s1 = none ? 1.0f : ortho_scale(l);
    // one transform: value = scale * SYM(s1 * raw); two: SYM(s1 * raw) between them, scale * s1 on the way out
    return run(x, y, mask, out, P, l, l, mask_planes, pre == 1 ? kSymMask : (pre == 2 ? kSymDagger : kSymNone), sym, second,
               none ? 0 : 1, s1, add, second ? scale * s1 : scale, c, (hipStream_t)stream);
}
