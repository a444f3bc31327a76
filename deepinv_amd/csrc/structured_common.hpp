// What dst.hip (StructuredRandom on paired real rows) and cstructured.hip (the structured operator of phase retrieval on whole
// complex planes, and ptychography) share: the layer schedule, the two-float scale of an orthonormal transform and the pad / trim
// validation.  The kernels' loops are their own.
#pragma once
#include "fft_core.hpp"

#include <cmath>

namespace dinv {

// diagonal applied before / after transform t of T = layers + half (-1: none).  A: [F] then (D_i, F) for i = 0 .. L - 1;
// A_adjoint: (F^-1, conj D_{L-1-i}) for i = 0 .. L - 1, then [F^-1]
struct LayerSchedule {
    int layers, half, adjoint;
    __device__ __forceinline__ int diag_before(int t) const { return adjoint ? -1 : (t >= half ? t - half : -1); }
    __device__ __forceinline__ int diag_after(int t) const { return adjoint ? (t < layers ? layers - 1 - t : -1) : -1; }
};

// The scale 1 / sqrt(n) of an orthonormal transform as an unevaluated sum of two floats: the rounding of the constant would be a
// bias common to every output, which an iteration over the operator accumulates coherently
struct TwoFloat {
    float hi, lo;
};
inline TwoFloat make_two_float(double v) {
    TwoFloat t;
    t.hi = (float)v;
    t.lo = (float)(v - (double)t.hi);
    return t;
}
__device__ __forceinline__ float scaled(float z, TwoFloat s) { return fmaf(z, s.hi, z * s.lo); }
__device__ __forceinline__ float2 scaled(float2 z, TwoFloat s) { return make_float2(scaled(z.x, s), scaled(z.y, s)); }

// the geometry of a centred pad or trim: the working size is the larger side, and the offsets keep the small side inside it
inline int check_pad_trim(const char* op, int H_in, int W_in, int H_out, int W_out, int H_work, int W_work, int top, int left) {
    DINV_REQUIRE(H_in >= 1 && W_in >= 1 && H_out >= 1 && W_out >= 1, "%s: empty side", op);
    DINV_REQUIRE(H_work == (H_in > H_out ? H_in : H_out) && W_work == (W_in > W_out ? W_in : W_out),
                 "%s: the working size must be the larger of the two sides (got %d x %d for %d x %d -> %d x %d)", op, H_work, W_work,
                 H_in, W_in, H_out, W_out);
    const int h_small = H_in < H_out ? H_in : H_out, w_small = W_in < W_out ? W_in : W_out;
    DINV_REQUIRE(top >= 0 && left >= 0 && top + h_small <= H_work && left + w_small <= W_work,
                 "%s: offsets (%d, %d) put the small side outside the working one", op, top, left);
    return 0;
}

}  // namespace dinv
