// What csrc/radon.hip and csrc/radon_tiled.hip share: the sample coordinates and the disc mask (device), the body of the sinogram pack kernels,
// and the host side every entry point opens with (descriptor -> geometry, images per group, the order of the argument checks).
//
// EVERY forward and adjoint kernel of both files takes its coordinates from the functions below and from nowhere else: an adjoint
// is the exact transpose of its forward only because both round every sample position alike, and a second copy of any of these
// functions is a second chance to round differently.
#pragma once
#include "common.hpp"

#include <algorithm>
#include <type_traits>

#pragma clang fp contract(off)  // forward and adjoint must round the sample coordinates identically

namespace dinv {

// the disc mask of radon.py:270-283, xa^2 + ya^2 <= 1, with both squares rounded before the sum as the reference's tensor
// expression rounds them: the squares are made opaque so that the compiler cannot contract the sum into a fused multiply-add,
// which moves points that lie on the circle outside it (row 56, column 7 of a 71 x 71 disc: 0.6^2 + 0.8^2 rounds to 1 in fp32,
// fma(0.6, 0.6, 0.8^2) to 1 + 2^-23)
__device__ __forceinline__ bool in_unit_disc(float xa, float ya) {
    float x2 = xa * xa, y2 = ya * ya;
#ifndef DINV_EMU
    asm volatile("" : "+v"(x2), "+v"(y2));
#endif
    return x2 + y2 <= 1.0f;
}

// pixel (row, col) of the W x W image against that mask: axes = 2 k / (W - 1) - 1 (symmetric in row and col)
__device__ __forceinline__ bool pixel_in_disc(int row, int col, int W) {
    const float ya = 2.0f * (float)col / (float)(W - 1) - 1.0f;
    const float xa = 2.0f * (float)row / (float)(W - 1) - 1.0f;
    return in_unit_disc(xa, ya);
}

// sample position (ix -> column, iy -> row) for grid = [gx, gy] R^T (radon.py:334-341), unnormalised as ATen's grid_sampler
// (align_corners=True): the fan-beam kernels, whose lattice is not uniform
__device__ __forceinline__ void sample_pos(float c, float s, float xj, float xi, float gm1, float& ix, float& iy) {
    const float gx = fmaf(c, xj, s * xi);
    const float gy = fmaf(-s, xj, c * xi);
    ix = ((gx + 1.0f) * 0.5f) * gm1;
    iy = ((gy + 1.0f) * 0.5f) * gm1;
}

// Parallel beam: the lattice is the rotation of the UNIFORM base grid xn = linspace(-1, 1, G) of affine_grid (radon.py:252-342), so
// in pixel units the sample of ray j at step i is   (ix, iy) = ctr + R (j - ctr, i - ctr),   ctr = (G - 1) / 2:
//   ix = fma(s, i - ctr, fma(c, j - ctr, ctr)),   iy = fma(c, i - ctr, fma(-s, j - ctr, ctr))
// - one fused multiply-add per coordinate and step from a per-ray base (j - ctr and i - ctr are exact), two roundings of at most
// half an ulp of G each (6e-5 pixel at G = 729), against nine operations per step for the chain above, whose own roundings are of
// the same size.  The adjoint's tap weights are the forward's.  (The base grid is the reference's linspace by construction; the
// `xn` arguments of the entry points keep their place in the ABI, the parallel-beam kernels do not read them.)
__device__ __forceinline__ void ray_base(float c, float s, float dj, float ctr, float& bx, float& by) {
    bx = fmaf(c, dj, ctr);
    by = fmaf(-s, dj, ctr);
}
__device__ __forceinline__ void lattice_pos(float c, float s, float bx, float by, float di, float& ix, float& iy) {
    ix = fmaf(s, di, bx);
    iy = fmaf(c, di, by);
}

// bilinear weight of integer pixel p for a sample at position t along one axis.  With f = floor(t): p == f gives
// 1 - (t - f) and p == f + 1 gives t - f, both EXACTLY what grid_sample's weights are (t - p is exact by Sterbenz,
// and 1 - (1 - frac) is exact because frac is a multiple of ulp(t) >= 2^-23); any other p clamps to 0.
__device__ __forceinline__ float weight_of(float t, float p) {
    const float w = 1.0f - fabsf(t - p);
    return w > 0.f ? w : 0.f;
}

// acc[k] += the bilinear sample of image k at fractions (tx, ty): p is the upper-left tap of NB packed images (batch innermost),
// GP the pitch of the packed image in pixels
template <int NB>
__device__ __forceinline__ void add_taps(float (&acc)[NB], const float* p, int GP, float tx, float ty) {
    const float w00 = (1.0f - tx) * (1.0f - ty), w01 = tx * (1.0f - ty);
    const float w10 = (1.0f - tx) * ty, w11 = tx * ty;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        acc[k] = fmaf(w00, p[k], acc[k]);
        acc[k] = fmaf(w01, p[NB + k], acc[k]);
        acc[k] = fmaf(w10, p[(int64_t)GP * NB + k], acc[k]);
        acc[k] = fmaf(w11, p[(int64_t)GP * NB + NB + k], acc[k]);
    }
}

// (The scaled store that ends the gather kernels is written out in each of them: as a helper it changed their generated code.)

// The sinogram pack, sino [n_img, N, A] -> sp [groups][A][jpad + N + jpad][NB], zeros in the padding and in the images past n_img:
// the whole body (grid-stride) of the pack kernels radon_pack_sino (radon.hip: jpad = 0) and radon_pack_sino2 (radon_tiled.hip:
// jpad = JPAD), which keep their names - the launch lists the tests and the profiles record name them
template <int NB>
__device__ __forceinline__ void pack_sino(int n_img, int groups, int A, int N, int jpad, const float* __restrict__ sino,
                                          float* __restrict__ sp) {
    const int NJ = N + 2 * jpad;
    const int64_t total = (int64_t)groups * A * NJ;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int grp = (int)(idx / ((int64_t)A * NJ));
        const int rem = (int)(idx - (int64_t)grp * A * NJ);
        const int a = rem / NJ, j = rem - a * NJ - jpad;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int n = grp * NB + k;
            sp[idx * NB + k] = (n < n_img && j >= 0 && j < N) ? sino[((int64_t)n * N + j) * A + a] : 0.f;
        }
    }
}

// ---- host side
// blocks of 256 threads for a grid-stride pack kernel over n elements
inline dim3 pack_blocks(int64_t n) { return dim3((unsigned)std::min<int64_t>(ceil_div(n, 256), 65535)); }

// descriptor -> the fields every kernel geometry (RadonGeom, TiledGeom) has; *NB = images per group (batch innermost in the packs)
template <class Geom>
int desc_to_geom(const dinv_radon_desc* d, Geom* g, int32_t* NB) {
    DINV_REQUIRE(d != nullptr, "null descriptor");
    DINV_REQUIRE(d->n_img >= 0 && d->width >= 2 && d->grid >= d->width && d->n_angles >= 1, "bad radon geometry");
    DINV_REQUIRE(d->pad_before >= 0 && d->pad_before + d->width <= d->grid, "bad padding");
    g->n_img = d->n_img; g->W = d->width; g->G = d->grid; g->pad = d->pad_before; g->A = d->n_angles;
    g->circle = d->circle; g->scale = d->scale;
    *NB = d->n_img >= 8 ? 8 : d->n_img >= 4 ? 4 : d->n_img >= 2 ? 2 : 1;
    g->groups = d->n_img == 0 ? 0 : (d->n_img + *NB - 1) / *NB;
    return 0;
}

// body(std::integral_constant<int, NB>) for NB = 8, 4, 2 or 1; returns what body returns (an error code, 0 = fine)
template <class F>
int dispatch_nb(int nb, F&& body) {
    switch (nb) {
        case 8: return body(std::integral_constant<int, 8>{});
        case 4: return body(std::integral_constant<int, 4>{});
        case 2: return body(std::integral_constant<int, 2>{});
        default: return body(std::integral_constant<int, 1>{});
    }
}

// What every entry point that packs and launches opens and ends with.  `geom_rc` is the result of its descriptor -> geometry step
// (which filled g), `pointers` whether all of its pointers are non-null, `ws_need` its *_workspace_bytes.  An empty batch returns
// before any other argument is looked at.  launch(stream, (cos, sin) table, workspace) holds the entry's own limits and launches.
template <class Geom, class F>
int radon_call(int geom_rc, const Geom& g, bool pointers, size_t ws_bytes, size_t ws_need, const float* cs, void* ws,
               dinv_stream_t stream, F&& launch) {
    if (geom_rc) return geom_rc;
    if (g.n_img == 0) return 0;
    DINV_REQUIRE(pointers, "null pointer");
    DINV_REQUIRE(ws_bytes >= ws_need, "workspace too small");
    if (int e = launch(reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float2*>(cs), reinterpret_cast<float*>(ws)))
        return e;
    DINV_CHECK_LAUNCH();
    return 0;
}

}  // namespace dinv
