// out[I, R] = in[I, K] M^T on the fp32 matrix cores (gfx950): the three operators of CompressedSensing.
//
// Replaces the ATen launches behind
//   CompressedSensing.A / A_adjoint / A_dagger     deepinv/physics/compressed_sensing.py:126-166 (torch.einsum("in, mn->im"))
//
// The regime is few rows (I = the batch, 1 to a few tens) against a matrix of hundreds to thousands of rows and columns: the call
// is bound by streaming M from HBM once, so the layout follows M.
//   transposed = 0   out[i, r] = sum_k in[i, k] M[r, k]     M is [R, K], row stride ldm
//   transposed = 1   out[i, r] = sum_k in[i, k] M[k, r]     M is [K, R], row stride ldm  (A_adjoint reads _A itself)
//
// dense_partial_kernel: one wave owns 32 output columns r, one slice of K and up to 32 NI input rows, and accumulates
// v_mfma_f32_32x32x2_f32 with the input rows on the A side and the rows of M on the B side.  Lane l supplies row (l & 31) and the
// 16 consecutive k's of half (l >> 5) of a block of 32: for transposed = 0 that is 64 contiguous bytes of a row of M per lane
// (four 16-byte loads where the row is aligned), for transposed = 1 sixteen loads that each cover 128 contiguous bytes per half
// wave.  Which k a lane supplies to which MFMA is free as long as both operands agree, so no value is shuffled.  Edges (I, K, R of
// any size) are zero-filled in registers; M is never copied.
// K is split over gridDim.y slices so that more than R / 32 waves stream M; every slice writes its partial tile to the workspace
// [S, I, R] and dense_reduce_kernel adds the slices in index order: no atomics, bit-reproducible.  One slice writes `out` itself.
// The tile constants, the K-slice and workspace rules, the checks, the grid and the dispatch are those of dense_core.hpp, shared
// with cdense.hip; this file holds the fp32 kernels and what they are given.
// The Gaussian-mixture patch prior (dinv_gmm_*: scores, classification and the EPLL step) uses the same fp32 product scheme with
// its own epilogues: its kernels and planning are patch_gmm.hpp, its entry points are at the end of this file.  The sums of its EM
// step (dinv_gmm_posterior, dinv_gmm_moments) follow them: gmm_moments.hpp.
#include "dense_core.hpp"
#include "patch_gmm.hpp"
#include "gmm_moments.hpp"

using namespace dinv;

namespace {

constexpr int kBlockK = 32;     // k's per step: 16 per half wave
constexpr DenseScalar kReal{"dense", (int)sizeof(float), kBlockK, false};

struct DenseArgs {
    const float* in;
    const float* M;
    float* dst;          // out, or the workspace [S, I, R]
    int64_t I, K, R, ldm;
    int64_t kchunk;      // k's per slice, a multiple of kBlockK
    int transposed;
    int vec_in, vec_m;   // 16-byte loads along k are aligned
};

// 16 consecutive floats of a row, zero past `avail`
__device__ __forceinline__ void load_row16(const float* __restrict__ p, int64_t avail, bool vec, float (&v)[16]) {
    if (vec && avail >= 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 f = reinterpret_cast<const float4*>(p)[q];
            v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = q < avail ? p[q] : 0.f;
    }
}

template <int NI>
__global__ __launch_bounds__(64) void dense_partial_kernel(DenseArgs a) {
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    const int64_t r = (int64_t)blockIdx.x * kTile + j;
    const int64_t s = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.z * kTile * NI;
    const int64_t kbeg = s * a.kchunk;
    const int64_t kend = kbeg + a.kchunk < a.K ? kbeg + a.kchunk : a.K;
    // NA independent accumulators per tile of input rows, fed in turn and added at the end: back-to-back MFMAs never wait on
    // each other's result, and the chain of roundings of one sum is NA times shorter
    constexpr int NA = kMaxNI / NI;
    f32x16 acc[NI][NA];
#pragma unroll
    for (int t = 0; t < NI; ++t)
#pragma unroll
        for (int u = 0; u < NA; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][u][e] = 0.f;
    for (int64_t k0 = kbeg; k0 < kend; k0 += kBlockK) {
        const int64_t k = k0 + 16 * h;
        const int64_t avail = kend - k;      // may be <= 0 for the upper half of the last block
        float mv[16];
        if (r >= a.R || avail <= 0) {
#pragma unroll
            for (int q = 0; q < 16; ++q) mv[q] = 0.f;
        } else if (!a.transposed) {
            load_row16(a.M + r * a.ldm + k, avail, a.vec_m != 0, mv);
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) mv[q] = q < avail ? a.M[(k + q) * a.ldm + r] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < NI; ++t) {
            const int64_t i = i0 + t * kTile + j;
            float xv[16];
            if (i >= a.I || avail <= 0) {
#pragma unroll
                for (int q = 0; q < 16; ++q) xv[q] = 0.f;
            } else {
                load_row16(a.in + i * a.K + k, avail, a.vec_in != 0, xv);
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[t][q % NA] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[q], mv[q], acc[t][q % NA], 0, 0, 0);
        }
    }
    // D element e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5) (an input row), column l & 31 (a row of M)
    if (r < a.R) {
        float* dst = a.dst + s * a.I * a.R;
#pragma unroll
        for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int64_t i = i0 + t * kTile + (e & 3) + 8 * (e >> 2) + 4 * h;
                float v = acc[t][0][e];
                if constexpr (NA == 4) v = (v + acc[t][1][e]) + (acc[t][2][e] + acc[t][3][e]);
                if constexpr (NA == 2) v = v + acc[t][1][e];
                if (i < a.I) dst[i * a.R + r] = v;
            }
    }
}

__global__ __launch_bounds__(256) void dense_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, int64_t total, int S) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        float v = ws[e];
        for (int s = 1; s < S; ++s) v += ws[(int64_t)s * total + e];
        out[e] = v;
    }
}

}  // namespace

extern "C" size_t dinv_dense_workspace_bytes(int64_t I, int64_t K, int64_t R) { return dense_workspace_bytes(kReal, I, K, R); }

extern "C" int dinv_dense_apply(const float* in, const float* M, float* out, int64_t I, int64_t K, int64_t R, int64_t ldm,
                                int32_t transposed, void* workspace, size_t workspace_bytes, dinv_stream_t stream) {
    DensePlan p;
    if (int e = dense_plan(kReal, in, M, out, I, K, R, ldm, transposed, workspace, workspace_bytes, &p)) return e;
    if (p.empty) return 0;
    hipStream_t st = (hipStream_t)stream;
    DenseArgs a{};
    a.in = in; a.M = M;
    a.dst = p.S > 1 ? (float*)workspace : out;
    a.I = I; a.K = K; a.R = R; a.ldm = ldm; a.kchunk = p.kchunk;
    a.transposed = transposed ? 1 : 0;
    a.vec_in = p.vec_in; a.vec_m = p.vec_m;
    DINV_DENSE_LAUNCH_PARTIAL(dense_partial_kernel, p, st, a);
    if (p.S > 1) {
        hipLaunchKernelGGL(dense_reduce_kernel, p.reduce_grid, dim3(256), 0, st, (const float*)workspace, out, p.total, (int)p.S);
        DINV_CHECK_LAUNCH();
    }
    return 0;
}

// ---------------------------------------------------------------- Gaussian-mixture patch prior (patch_gmm.hpp)
extern "C" int dinv_gmm_scores(const float* src, int32_t image, int64_t N, int32_t C, int32_t H, int32_t W, int32_t p, const float* Wt,
                               const float* m, const float* lam, const float* logw, int32_t K, int32_t d, const float* r,
                               int32_t epilogue, void* out, dinv_stream_t stream) {
    const GmmModel g{Wt, m, lam, logw, K, d};
    GmmPlan pl;
    if (int e = gmm_check_epilogue("gmm_scores", epilogue)) return e;
    if (int e = image ? gmm_plan_image("gmm_scores", g, N, C, H, W, p, &pl) : gmm_plan_rows("gmm_scores", g, N, &pl)) return e;
    if (pl.empty) return 0;
    DINV_REQUIRE(src && out, "gmm_scores: src and out must be non-null");
    DINV_REQUIRE((const void*)src != out, "gmm_scores: out must not alias src");
    DINV_REQUIRE(epilogue != DINV_GMM_SCORES || pl.N * K < ((int64_t)1 << 40), "gmm_scores: a score matrix of %lld x %d is too large",
                 (long long)pl.N, K);
    hipStream_t st = (hipStream_t)stream;
    GmmScoreArgs a{};
    a.g = g; a.src = src; a.r = r; a.out = out; a.N = pl.N;
    a.C = C; a.H = H; a.W = W; a.p = image ? p : 1; a.PH = pl.PH; a.PW = pl.PW;
    a.epilogue = epilogue;
    if (image) DINV_GMM_LAUNCH_SCORE(true, pl, st, a);
    else DINV_GMM_LAUNCH_SCORE(false, pl, st, a);
    return 0;
}

extern "C" size_t dinv_gmm_epll_workspace_bytes(int64_t B, int32_t C, int32_t H, int32_t W, int32_t p) {
    return gmm_epll_workspace_bytes(B, C, H, W, p);
}

extern "C" int dinv_gmm_epll_step(const float* x, int64_t B, int32_t C, int32_t H, int32_t W, int32_t p, const float* Wt, const float* m,
                                  const float* lam, const float* logw, int32_t K, int32_t d, const float* r, const float* a,
                                  const float* cb, const float* bias, float* out, void* workspace, size_t workspace_bytes,
                                  dinv_stream_t stream) {
    const GmmModel g{Wt, m, lam, logw, K, d};
    GmmPlan pl;
    if (int e = gmm_plan_image("gmm_epll_step", g, B, C, H, W, p, &pl)) return e;
    if (pl.empty) return 0;
    DINV_REQUIRE(x && out && r && a, "gmm_epll_step: x, out, r and a must be non-null");
    const size_t need = gmm_epll_workspace_bytes(B, C, H, W, p);
    DINV_REQUIRE(workspace && workspace_bytes >= need, "gmm_epll_step: the workspace holds %zu bytes, %zu are needed "
                 "(dinv_gmm_epll_workspace_bytes)", workspace_bytes, need);
    DINV_REQUIRE(aligned16(workspace), "gmm_epll_step: the workspace must be 16-byte aligned");
    DINV_REQUIRE(2 * (size_t)d * sizeof(float) <= kDefaultLdsBytes, "gmm_epll_step: d = %d is too large for the estimate kernel", d);
    hipStream_t st = (hipStream_t)stream;
    float* z = (float*)workspace;
    int32_t* kstar = (int32_t*)(z + pl.N * d);
    GmmScoreArgs s{};
    s.g = g; s.src = x; s.r = r; s.out = kstar; s.N = pl.N;
    s.C = C; s.H = H; s.W = W; s.p = p; s.PH = pl.PH; s.PW = pl.PW;
    s.epilogue = DINV_GMM_ARGMAX;
    DINV_GMM_LAUNCH_SCORE(true, pl, st, s);
    GmmEstimateArgs e{};
    e.g = g; e.x = x; e.r = r; e.kstar = kstar; e.z = z; e.N = pl.N;
    e.C = C; e.H = H; e.W = W; e.p = p; e.PH = pl.PH; e.PW = pl.PW;
    hipLaunchKernelGGL(gmm_estimate_kernel, dim3((unsigned)ceil_div(pl.N, kGmmEstPatches)), dim3(64), 2 * (size_t)d * sizeof(float), st, e);
    DINV_CHECK_LAUNCH();
    GmmAggregateArgs ag{};
    ag.z = z; ag.a = a; ag.cb = cb; ag.bias = bias; ag.out = out; ag.total = B * C * H * W;
    ag.d = d; ag.C = C; ag.H = H; ag.W = W; ag.p = p; ag.PH = pl.PH; ag.PW = pl.PW;
    const int64_t blocks = ceil_div(ag.total, 256);
    hipLaunchKernelGGL(gmm_aggregate_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, st, ag);
    DINV_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------- EM for the Gaussian mixture (patch_gmm.hpp, gmm_moments.hpp)
extern "C" int dinv_gmm_posterior(const float* x, int64_t N, const float* Wt, const float* m, const float* lam, const float* logw,
                                  int32_t K, int32_t d, float* beta, float* nll, dinv_stream_t stream) {
    const GmmModel g{Wt, m, lam, logw, K, d};
    GmmPlan pl;
    if (int e = gmm_plan_rows("gmm_posterior", g, N, &pl)) return e;
    if (pl.empty) return 0;
    DINV_REQUIRE(logw, "gmm_posterior: the log weights must be non-null: a responsibility carries its component's weight");
    DINV_REQUIRE(x && beta && nll, "gmm_posterior: x, beta and nll must be non-null");
    DINV_REQUIRE(x != beta && x != nll && beta != nll, "gmm_posterior: beta and nll must not alias x or each other");
    DINV_REQUIRE(pl.N * K < ((int64_t)1 << 40), "gmm_posterior: a responsibility matrix of %lld x %d is too large", (long long)pl.N, K);
    hipStream_t st = (hipStream_t)stream;
    GmmScoreArgs a{};
    a.g = g; a.src = x; a.r = nullptr; a.out = beta; a.nll = nll; a.N = pl.N;
    a.p = 1;
    a.epilogue = kGmmPosterior;
    DINV_GMM_LAUNCH_SCORE(false, pl, st, a);
    return 0;
}

extern "C" size_t dinv_gmm_moments_workspace_bytes(int64_t N, int32_t K, int32_t d, int32_t chunk_rows) {
    return gmm_moments_workspace_bytes(N, K, d, chunk_rows);
}

extern "C" int dinv_gmm_moments(const float* x, const float* beta, const float* c, const float* nll, int64_t N, int32_t K, int32_t d,
                                int32_t chunk_rows, double* S0, double* S1, double* S2, double* obj, void* workspace,
                                size_t workspace_bytes, dinv_stream_t stream) {
    GmmMomentsPlan pl;
    if (int e = gmm_moments_plan("gmm_moments", N, K, d, chunk_rows, &pl)) return e;
    if (pl.empty) return 0;
    DINV_REQUIRE(x && beta && c, "gmm_moments: x, beta and c must be non-null");
    DINV_REQUIRE(S0 && S1 && S2, "gmm_moments: the accumulators S0, S1 and S2 must be non-null");
    DINV_REQUIRE(!nll || obj, "gmm_moments: nll is given, so the accumulator obj must be non-null");
    DINV_REQUIRE(workspace && workspace_bytes >= pl.ws_bytes, "gmm_moments: the workspace holds %zu bytes, %zu are needed "
                 "(dinv_gmm_moments_workspace_bytes)", workspace_bytes, pl.ws_bytes);
    DINV_REQUIRE(aligned16(workspace), "gmm_moments: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    GmmMomentsArgs a{};
    a.x = x; a.beta = beta; a.c = c; a.ws = (float*)workspace;
    a.N = N; a.chunk_rows = pl.chunk_rows; a.chunks = pl.chunks;
    a.K = K; a.d = d; a.T = pl.T; a.nblk = pl.nblk;
    const dim3 grid((unsigned)pl.items, (unsigned)pl.chunks, (unsigned)K);
    DINV_GMM_LAUNCH_MOMENTS(pl, grid, st, a);
    GmmReduceArgs r{};
    r.ws = a.ws; r.nll = nll; r.S0 = S0; r.S1 = S1; r.S2 = S2; r.obj = obj;
    r.N = N; r.chunks = pl.chunks; r.total = (int64_t)K * pl.nblk * 1024;
    r.K = K; r.d = d; r.T = pl.T; r.nblk = pl.nblk;
    hipLaunchKernelGGL(gmm_moments_reduce_kernel, dim3((unsigned)(r.total / 256 + 1)), dim3(256), 0, st, r);
    DINV_CHECK_LAUNCH();
    return 0;
}
