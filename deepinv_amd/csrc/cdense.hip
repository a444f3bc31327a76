// out[I, R] = in[I, K] op(M) in complex64 on the fp32 matrix cores (gfx950), with a pointwise epilogue: the products of phase
// retrieval with a dense matrix, y = |Bx|^2.
//
// Replaces the ATen launches behind
//   RandomPhaseRetrieval.A / B / B_adjoint / B_dagger / A_vjp   deepinv/physics/phase_retrieval.py:42-99 over
//                          compressed_sensing.py:126-166 (a complex einsum, then abs, square, or a multiply, one pass each)
//   AmplitudeLoss.grad     deepinv/optim/distance.py:353-369 between B and B_adjoint (add, div, sqrt, rsub, mul: five passes)
//   spectral_methods       deepinv/optim/phase_retrieval.py:174-177 (B, a multiply, B_adjoint per power iteration)
//
// Every operand is complex64 as interleaved fp32 pairs.  op(M)(r, k) is selected by two flags:
//   transposed = 0   M is [R, K], row stride ldm (in complex elements):  M[r, k]
//   transposed = 1   M is [K, R], row stride ldm:                         M[k, r]     (B_adjoint reads _A itself: _A.conj().T)
//   conj = 1         the conjugate of either
// The design is that of dense.hip, and the tile constants, the K-slice and workspace rules, the checks, the grid and the dispatch are
// the same code (dense_core.hpp); the host check of the epilogue is that of common.hpp, shared with cstructured.hip.  One wave owns 32 output columns r, one slice of K and up to 32 NI input rows; lane l supplies
// row (l & 31) and the 8 consecutive k's of half (l >> 5) of a block of 16 (64 contiguous bytes of a row of M per lane, or for
// transposed = 1 eight loads that each cover 256 contiguous bytes per half wave).  A complex multiply-accumulate is four
// v_mfma_f32_32x32x2_f32: re += xr mr, re += (-xi) mi, im += xr mi, im += xi mr; conjugation is the sign of mi, applied once where M
// is loaded.  Edges (I, K, R of any size) are zero-filled in registers; M is never copied.  K is split over gridDim.y slices, every
// slice writes its partial tile to the workspace [S, I, R] and cdense_reduce_kernel adds the slices in index order: no atomics,
// bit-reproducible.  The epilogue is applied where the finished sum is at hand: in the store of the single-slice path, in the
// reduce kernel otherwise.
#include "dense_core.hpp"

using namespace dinv;

namespace {

constexpr int kBlockK = 16;     // complex k's per step: 8 per half wave
constexpr int kHalfK = 8;
constexpr DenseScalar kComplex{"cdense", (int)sizeof(float2), kBlockK, true};

struct CDenseArgs {
    const float2* in;
    const float2* M;
    float2* dst;         // the workspace [S, I, R], or null when the single slice stores the result itself
    float* out;          // complex [I, R] as pairs, or real [I, R] for DINV_CDENSE_ABS2
    const float* aux;    // w or y, real [I, R]
    int64_t I, K, R, ldm;
    int64_t kchunk;      // k's per slice, a multiple of kBlockK
    int transposed, conj;
    int vec_in, vec_m;   // 16-byte loads along k are aligned
    int epilogue;
    float eps;
};

// the finished sum z of output element e = i * R + r goes to `out` through the epilogue.  z arrives in double, the exact sum of the
// fp32 partial sums, and the epilogue is evaluated in double and rounded once: |z|^2 and the amplitude factor carry the error of the
// matrix-core accumulation alone, not a rounding of z, of its squares and of the division and the root on top
__device__ __forceinline__ void store_epilogue(float* __restrict__ out, const float* __restrict__ aux, int epilogue, float eps, int64_t e,
                                               double zr, double zi) {
    if (epilogue == DINV_CDENSE_ABS2) {
        out[e] = (float)(zr * zr + zi * zi);
        return;
    }
    double f = 1.0;
    if (epilogue == DINV_CDENSE_WEIGHT) f = (double)aux[e];
    if (epilogue == DINV_CDENSE_AMPLITUDE) f = 1.0 - sqrt((double)aux[e] / ((zr * zr + zi * zi) + (double)eps));
    reinterpret_cast<float2*>(out)[e] = make_float2((float)(zr * f), (float)(zi * f));
}

// 8 consecutive complex values of a row as separate real and imaginary parts, zero past `avail`
__device__ __forceinline__ void load_row8(const float2* __restrict__ p, int64_t avail, bool vec, float (&re)[kHalfK], float (&im)[kHalfK]) {
    if (vec && avail >= kHalfK) {
#pragma unroll
        for (int q = 0; q < kHalfK / 2; ++q) {
            const float4 f = reinterpret_cast<const float4*>(p)[q];
            re[2 * q] = f.x; im[2 * q] = f.y; re[2 * q + 1] = f.z; im[2 * q + 1] = f.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < kHalfK; ++q) {
            const float2 f = q < avail ? p[q] : make_float2(0.f, 0.f);
            re[q] = f.x; im[q] = f.y;
        }
    }
}

template <int NI>
__global__ __launch_bounds__(64) void cdense_partial_kernel(CDenseArgs a) {
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    const int64_t r = (int64_t)blockIdx.x * kTile + j;
    const int64_t s = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.z * kTile * NI;
    const int64_t kbeg = s * a.kchunk;
    const int64_t kend = kbeg + a.kchunk < a.K ? kbeg + a.kchunk : a.K;
    // NA independent accumulator pairs per tile of input rows, fed in turn and added at the end, as in dense.hip
    constexpr int NA = kMaxNI / NI;
    f32x16 are[NI][NA], aim[NI][NA];
#pragma unroll
    for (int t = 0; t < NI; ++t)
#pragma unroll
        for (int u = 0; u < NA; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) are[t][u][e] = aim[t][u][e] = 0.f;
    for (int64_t k0 = kbeg; k0 < kend; k0 += kBlockK) {
        const int64_t k = k0 + kHalfK * h;
        const int64_t avail = kend - k;      // may be <= 0 for the upper half of the last block
        float mr[kHalfK], mi[kHalfK];
        if (r >= a.R || avail <= 0) {
#pragma unroll
            for (int q = 0; q < kHalfK; ++q) mr[q] = mi[q] = 0.f;
        } else if (!a.transposed) {
            load_row8(a.M + r * a.ldm + k, avail, a.vec_m != 0, mr, mi);
        } else {
#pragma unroll
            for (int q = 0; q < kHalfK; ++q) {
                const float2 f = q < avail ? a.M[(k + q) * a.ldm + r] : make_float2(0.f, 0.f);
                mr[q] = f.x; mi[q] = f.y;
            }
        }
        if (a.conj) {
#pragma unroll
            for (int q = 0; q < kHalfK; ++q) mi[q] = -mi[q];
        }
#pragma unroll
        for (int t = 0; t < NI; ++t) {
            const int64_t i = i0 + t * kTile + j;
            float xr[kHalfK], xi[kHalfK];
            if (i >= a.I || avail <= 0) {
#pragma unroll
                for (int q = 0; q < kHalfK; ++q) xr[q] = xi[q] = 0.f;
            } else {
                load_row8(a.in + i * a.K + k, avail, a.vec_in != 0, xr, xi);
            }
#pragma unroll
            for (int q = 0; q < kHalfK; ++q) {
                f32x16& re = are[t][q % NA];
                f32x16& im = aim[t][q % NA];
                re = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[q], mr[q], re, 0, 0, 0);
                im = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[q], mi[q], im, 0, 0, 0);
                re = __builtin_amdgcn_mfma_f32_32x32x2f32(-xi[q], mi[q], re, 0, 0, 0);
                im = __builtin_amdgcn_mfma_f32_32x32x2f32(xi[q], mr[q], im, 0, 0, 0);
            }
        }
    }
    // D element e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5) (an input row), column l & 31 (a row of op(M))
    if (r < a.R) {
#pragma unroll
        for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int64_t i = i0 + t * kTile + (e & 3) + 8 * (e >> 2) + 4 * h;
                // a slice of several: the fp32 partial sum goes to the workspace; the only slice: the accumulators meet in double
                if (a.dst) {
                    float vr = are[t][0][e], vi = aim[t][0][e];
                    if constexpr (NA == 4) {
                        vr = (vr + are[t][1][e]) + (are[t][2][e] + are[t][3][e]);
                        vi = (vi + aim[t][1][e]) + (aim[t][2][e] + aim[t][3][e]);
                    }
                    if constexpr (NA == 2) {
                        vr = vr + are[t][1][e];
                        vi = vi + aim[t][1][e];
                    }
                    if (i < a.I) a.dst[(s * a.I + i) * a.R + r] = make_float2(vr, vi);
                    continue;
                }
                double vr = are[t][0][e], vi = aim[t][0][e];
#pragma unroll
                for (int u = 1; u < NA; ++u) {
                    vr += (double)are[t][u][e];
                    vi += (double)aim[t][u][e];
                }
                if (i >= a.I) continue;
                store_epilogue(a.out, a.aux, a.epilogue, a.eps, i * a.R + r, vr, vi);
            }
    }
}

__global__ __launch_bounds__(256) void cdense_reduce_kernel(const float2* __restrict__ ws, float* __restrict__ out,
                                                            const float* __restrict__ aux, int64_t total, int S, int epilogue, float eps) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        double vr = 0.0, vi = 0.0;
        for (int s = 0; s < S; ++s) {
            const float2 p = ws[(int64_t)s * total + e];
            vr += (double)p.x;
            vi += (double)p.y;
        }
        store_epilogue(out, aux, epilogue, eps, e, vr, vi);
    }
}

}  // namespace

extern "C" size_t dinv_cdense_workspace_bytes(int64_t I, int64_t K, int64_t R) { return dense_workspace_bytes(kComplex, I, K, R); }

extern "C" int dinv_cdense_apply(const float* in, const float* M, float* out, const float* aux, int64_t I, int64_t K, int64_t R,
                                 int64_t ldm, int32_t transposed, int32_t conj, int32_t epilogue, float eps, void* workspace,
                                 size_t workspace_bytes, dinv_stream_t stream) {
    if (int e = check_epilogue("cdense", epilogue)) return e;
    DensePlan p;
    if (int e = dense_plan(kComplex, in, M, out, I, K, R, ldm, transposed, workspace, workspace_bytes, &p)) return e;
    if (p.empty) return 0;
    if (int e = check_aux("cdense", epilogue, aux, out, "of the output's shape")) return e;
    hipStream_t st = (hipStream_t)stream;
    CDenseArgs a{};
    a.in = (const float2*)in; a.M = (const float2*)M;
    a.dst = p.S > 1 ? (float2*)workspace : nullptr;
    a.out = out; a.aux = needs_aux(epilogue) ? aux : nullptr;
    a.I = I; a.K = K; a.R = R; a.ldm = ldm; a.kchunk = p.kchunk;
    a.transposed = transposed ? 1 : 0;
    a.conj = conj ? 1 : 0;
    a.vec_in = p.vec_in; a.vec_m = p.vec_m;
    a.epilogue = epilogue; a.eps = eps;
    DINV_DENSE_LAUNCH_PARTIAL(cdense_partial_kernel, p, st, a);
    if (p.S > 1) {
        hipLaunchKernelGGL(cdense_reduce_kernel, p.reduce_grid, dim3(256), 0, st, (const float2*)workspace, out, a.aux, p.total, (int)p.S,
                           (int)epilogue, eps);
        DINV_CHECK_LAUNCH();
    }
    return 0;
}
