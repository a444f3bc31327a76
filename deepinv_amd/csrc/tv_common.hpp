// Helpers shared by the total-variation kernels (tv.hip) and the total-generalized-variation kernels (tgv.hip): the image
// geometry, pixel coordinates, the axis table and the wave reductions.
#pragma once
#include "common.hpp"

#include <algorithm>

// (in the anonymous namespace, as they were in tv.hip: the TV kernels keep their symbol names)
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;   // 256 CUs x 8 resident workgroups of 256 lanes

struct Geo {
    int D, H, W;
    int64_t plane;   // D * H * W
    int planes_per_sample;   // channels: lam[] is indexed by plane / channels
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// coordinates of pixel p (W fastest): c[0] = d, c[1] = h, c[2] = w
// (32-bit arithmetic: the entry points require n * nd < 2^31)
__device__ __forceinline__ void coords(const Geo& g, int64_t p, int& pl, int& d, int& h, int& w) {
    const uint32_t pp = (uint32_t)p;
    const uint32_t q = pp / (uint32_t)g.W;
    w = (int)(pp - q * (uint32_t)g.W);
    const uint32_t r = q / (uint32_t)g.H;
    h = (int)(q - r * (uint32_t)g.H);
    pl = (int)(r / (uint32_t)g.D);
    d = (int)(r - (uint32_t)pl * (uint32_t)g.D);
}

// axis k of an nd-dimensional field: (extent, coordinate, pixel stride).  nd = 2: k = 0 -> h, 1 -> w; nd = 3: d, h, w
template <int ND>
__device__ __forceinline__ void axis(const Geo& g, int k, int d, int h, int w, int& n, int& c, int64_t& s) {
    const int a = k + (3 - ND);
    if (a == 0) { n = g.D; c = d; s = (int64_t)g.H * g.W; }
    else if (a == 1) { n = g.H; c = h; s = g.W; }
    else { n = g.W; c = w; s = 1; }
}

inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>(std::max<int64_t>(dinv::ceil_div(n, kThreads), 1), kMaxBlocks); }

}  // namespace
