// The M-step sums of expectation-maximisation for a Gaussian mixture on the fp32 matrix cores (gfx950): the kernels and the host
// planning behind dinv_gmm_moments of dense.hip.  With dinv_gmm_posterior (gmm_score_kernel, epilogue POSTERIOR of patch_gmm.hpp)
// a batch of an EM step is THREE launches: posterior, moments, reduce.
//
// Replaces the ATen launches behind
//   GaussianMixtureModel._EM_step                                           deepinv/optim/utils.py:373-412
// which materialise beta_times_x [K, N, d], a K-fold tiled copy of x and the centred [K, N, d] tensor of the E-step per batch.
//
// For rows x [N, d], responsibilities beta [N, K] and centres c [K, d] let y_n = [x_n - c_k, 1] (d + 1 entries).  Then
//   G_k = sum_n beta_nk y_n y_n^T = [[S2_k, S1_k], [S1_k^T, S0_k]]
// holds all three sums of a component, and G_k = Y^T diag(beta_k) Y is one product with the contraction over n.  Centring keeps
// the entries of S2 at the scale of the covariance itself (raw second moments of patches in [0, 1] are about 0.25 and would lose
// eigenvalues of 1e-5 in C / w - mu mu^T); em_finalise of hip/gmm.py recovers the raw moments in fp64.
//
// gmm_moments_kernel<NJ>: one wave per (component k, chunk of rows, tile row bi and up to NJ tile columns bj >= bi of the upper
// triangle of G_k in tiles of 32 x 32).  v_mfma_f32_32x32x2_f32 contracts two rows per instruction: lane l = 32 h + j supplies
// A[i = j][n = h] = beta_nk y_n[32 bi + j] and B[n = h][j] = y_n[32 bj + j] of row n = 2 s + h of a tile of 32 rows, read where x
// lies (128 contiguous bytes per half wave); the 32 beta of a row tile are fetched once (lane j fetches row j) and handed out by
// __shfl.  Reads are clamped to the last row and the last column and masked to zero in registers, so the loop has no branches.
// The A value is shared by the NJ accumulators.  NJ = 1 for T = 1 tile per side (d <= 31), 2 for T = 2 (d <= 63), 4 above: a tile
// row of more than NJ blocks is split over waves (d = 192: T = 7, rows of 7 .. 1 blocks in 2, 2, 2, 1, 1, 1, 1 waves).  A wave
// accumulates its chunk in the MFMA accumulators and writes every block [32, 32] to the workspace [K, chunks, blocks, 32, 32].
// gmm_moments_reduce_kernel: one thread per entry (i <= j <= d) of G_k adds the chunks in ascending order in fp64 and adds the sum to
// the running fp64 accumulators S2 (both (i, j) and (j, i): S2 is exactly symmetric), S1 (j = d) and S0 (i = j = d); the last
// workgroup adds nll [N] in fp64 in a fixed order (thread t takes rows t mod 256, then a tree over LDS) to obj.  Every output
// has one writer: no atomics, two runs give the same bits.
//
// Chunks: chunk_rows is forced (a positive multiple of 32) or a function of (N, K, d) only: the rows are split so that
// K x (waves per chunk) x chunks reaches kGmmMomTargetWaves, with chunks of at least min(N, 128) rows, rounded up to 32.
// Executed over useful matrix-core work: (32 T)^2 over (d + 1)(d + 2) / 2 entries would be 2 with no symmetry; the upper triangle of
// blocks executes 1024 T (T + 1) / 2 products per row pair for (d + 1)(d + 2) / 2 useful ones: 4.37 at d = 36 (T = 2), 2.86 at 64,
// 1.71 at 108, 1.53 at 192; the last row tile of a chunk is padded to 32 rows.
//
// Limits (DINV_REQUIRE): 1 <= K <= 65535; 1 <= d <= 1023; N < 2^31; chunk_rows a non-negative multiple of 32; at most 65535 chunks;
// non-null operands and accumulators; the workspace of dinv_gmm_moments_workspace_bytes, 16-byte aligned.  N = 0 launches nothing.
#pragma once
#include "patch_gmm.hpp"

namespace dinv {

constexpr int kGmmMomRows = 32;              // rows per tile: the unit of chunk_rows
constexpr int kGmmMomTargetWaves = 4096;     // 16 per compute unit of an MI355X
constexpr int kGmmMomMinChunk = 128;         // the shortest automatic chunk: a chunk costs 4 KB of workspace traffic per block
constexpr int kGmmMomMaxD = 1023;

struct GmmMomentsArgs {
    const float* x;        // [N, d]
    const float* beta;     // [N, K]
    const float* c;        // [K, d]
    float* ws;             // [K, chunks, nblk, 32, 32]
    int64_t N, chunk_rows, chunks;
    int K, d, T, nblk;
};

// the index of block (bi, bj >= bi) in the upper triangle of T x T blocks, row by row
__host__ __device__ inline int gmm_mom_block(int T, int bi, int bj) { return bi * T - bi * (bi - 1) / 2 + (bj - bi); }

template <int NJ>
__global__ __launch_bounds__(64) void gmm_moments_kernel(GmmMomentsArgs a) {
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    const int k = (int)blockIdx.z, d = a.d, T = a.T;
    const int64_t ch = blockIdx.y;
    // the tile row and the first tile column of this wave: tile row bi is split into ceil((T - bi) / NJ) waves
    int bi = 0, it = (int)blockIdx.x;
    for (;; ++bi) {
        const int g = (T - bi + NJ - 1) / NJ;
        if (it < g) break;
        it -= g;
    }
    const int bj0 = bi + it * NJ;
    const int nj = T - bj0 < NJ ? T - bj0 : NJ;

    const float* ck = a.c + (int64_t)k * d;
    const int ci = 32 * bi + j, cic = ci < d ? ci : d - 1;
    const float cA = ck[cic];
    int cj[NJ], cjc[NJ];
    float cB[NJ];
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
        cj[q] = 32 * (bj0 + q) + j;
        cjc[q] = cj[q] < d ? cj[q] : d - 1;
        cB[q] = ck[cjc[q]];
    }
    f32x16 acc[NJ];
#pragma unroll
    for (int q = 0; q < NJ; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;

    const int64_t r0 = ch * a.chunk_rows;
    const int64_t r1 = r0 + a.chunk_rows < a.N ? r0 + a.chunk_rows : a.N;
    for (int64_t t0 = r0; t0 < r1; t0 += kGmmMomRows) {
        const int64_t rb = t0 + j < r1 ? t0 + j : r1 - 1;
        const float bw = t0 + j < r1 ? a.beta[rb * a.K + k] : 0.f;
#pragma unroll
        for (int s = 0; s < kGmmMomRows / 2; ++s) {
            const int64_t n = t0 + 2 * s + h;
            const bool in = n < r1;
            const float* xr = a.x + (in ? n : r1 - 1) * d;
            const float bv = __shfl(bw, 2 * s + h);
            const float xa = xr[cic];
            const float ya = !in ? 0.f : (ci < d ? xa - cA : (ci == d ? 1.f : 0.f));
            const float av = bv * ya;
#pragma unroll
            for (int q = 0; q < NJ; ++q)
                if (q < nj) {
                    const float xb = xr[cjc[q]];
                    const float yb = !in ? 0.f : (cj[q] < d ? xb - cB[q] : (cj[q] == d ? 1.f : 0.f));
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, yb, acc[q], 0, 0, 0);
                }
        }
    }
#pragma unroll
    for (int q = 0; q < NJ; ++q)
        if (q < nj) {
            float* dst = a.ws + ((((int64_t)k * a.chunks + ch) * a.nblk) + gmm_mom_block(T, bi, bj0 + q)) * 1024;
#pragma unroll
            for (int e = 0; e < 16; ++e) dst[((e & 3) + 8 * (e >> 2) + 4 * h) * 32 + j] = acc[q][e];
        }
}

struct GmmReduceArgs {
    const float* ws;
    const float* nll;      // [N] or null
    double* S0;            // [K]
    double* S1;            // [K, d]
    double* S2;            // [K, d, d]
    double* obj;           // [1]
    int64_t N, chunks, total;
    int K, d, T, nblk;
};

__global__ __launch_bounds__(256) void gmm_moments_reduce_kernel(GmmReduceArgs a) {
    const int tid = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {          // the objective
        __shared__ double part[256];
        if (!a.nll) return;
        double s = 0.0;
        for (int64_t n = tid; n < a.N; n += 256) s += (double)a.nll[n];
        part[tid] = s;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) part[tid] += part[tid + w];
            __syncthreads();
        }
        if (tid == 0) a.obj[0] += part[0];
        return;
    }
    const int64_t idx = (int64_t)blockIdx.x * 256 + tid;
    if (idx >= a.total) return;
    const int col = (int)(idx & 31), row = (int)((idx >> 5) & 31), blk = (int)((idx >> 10) % a.nblk), k = (int)((idx >> 10) / a.nblk);
    int bi = 0, rem = blk;
    while (rem >= a.T - bi) { rem -= a.T - bi; ++bi; }
    const int d = a.d, gi = 32 * bi + row, gj = 32 * (bi + rem) + col;
    if (gi > gj || gj > d) return;
    const float* src = a.ws + (((int64_t)k * a.chunks) * a.nblk + blk) * 1024 + row * 32 + col;
    double s = 0.0;
    for (int64_t ch = 0; ch < a.chunks; ++ch) s += (double)src[ch * a.nblk * 1024];
    if (gj < d) {
        a.S2[((int64_t)k * d + gi) * d + gj] += s;
        if (gi != gj) a.S2[((int64_t)k * d + gj) * d + gi] += s;
    } else if (gi < d) {
        a.S1[(int64_t)k * d + gi] += s;
    } else {
        a.S0[k] += s;
    }
}

// ---------------------------------------------------------------- host planning
struct GmmMomentsPlan {
    bool empty;
    int T, nblk, nj, items;        // tiles per side, blocks of the upper triangle, accumulators per wave, waves per (k, chunk)
    int64_t chunk_rows, chunks;
    size_t ws_bytes;
};

inline bool gmm_moments_shape_ok(int64_t N, int K, int d, int chunk_rows) {
    return K >= 1 && K < 65536 && d >= 1 && d <= kGmmMomMaxD && N >= 0 && N < ((int64_t)1 << 31) && chunk_rows >= 0 &&
           chunk_rows % kGmmMomRows == 0;
}

// the split of an accepted, non-empty shape: a function of (N, K, d, chunk_rows) only
inline void gmm_moments_split(int64_t N, int K, int d, int chunk_rows, GmmMomentsPlan* p) {
    p->T = (d + 1 + 31) / 32;
    p->nblk = p->T * (p->T + 1) / 2;
    p->nj = p->T == 1 ? 1 : (p->T == 2 ? 2 : 4);
    p->items = 0;
    for (int bi = 0; bi < p->T; ++bi) p->items += (p->T - bi + p->nj - 1) / p->nj;
    int64_t cr = chunk_rows;
    if (cr == 0) {
        const int64_t want = ceil_div(kGmmMomTargetWaves, (int64_t)K * p->items);
        cr = ceil_div(N, want);
        const int64_t least = N < kGmmMomMinChunk ? N : kGmmMomMinChunk;
        if (cr < least) cr = least;
        cr = ceil_div(cr, kGmmMomRows) * kGmmMomRows;
    }
    p->chunk_rows = cr;
    p->chunks = ceil_div(N, cr);
    p->ws_bytes = (size_t)K * p->chunks * p->nblk * 1024 * sizeof(float);
}

inline size_t gmm_moments_workspace_bytes(int64_t N, int K, int d, int chunk_rows) {
    if (!gmm_moments_shape_ok(N, K, d, chunk_rows) || N == 0) return 0;
    GmmMomentsPlan p;
    gmm_moments_split(N, K, d, chunk_rows, &p);
    return p.chunks < 65536 ? p.ws_bytes : 0;
}

inline int gmm_moments_plan(const char* op, int64_t N, int K, int d, int chunk_rows, GmmMomentsPlan* p) {
    DINV_REQUIRE(K >= 1 && K < 65536, "%s: K = %d components, expected 1 to 65535", op, K);
    DINV_REQUIRE(d >= 1 && d <= kGmmMomMaxD, "%s: dimension d = %d, expected 1 to %d", op, d, kGmmMomMaxD);
    DINV_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), "%s: %lld rows, the row count must be below 2^31", op, (long long)N);
    DINV_REQUIRE(chunk_rows >= 0 && chunk_rows % kGmmMomRows == 0, "%s: chunk_rows = %d is not a multiple of the row tile of %d "
                 "(0: automatic)", op, chunk_rows, kGmmMomRows);
    p->empty = N == 0;
    if (p->empty) return 0;
    gmm_moments_split(N, K, d, chunk_rows, p);
    DINV_REQUIRE(p->chunks < 65536, "%s: %lld chunks of %lld rows, at most 65535: raise chunk_rows", op, (long long)p->chunks,
                 (long long)p->chunk_rows);
    return 0;
}

// One instantiation per accumulator count.  A macro, because a launch is known by the spelling of its kernel expression (the launch
// log of the host emulation).
#define DINV_GMM_LAUNCH_MOMENTS(plan, grid, stream, args)                                                        \
    do {                                                                                                         \
        if ((plan).nj == 4) hipLaunchKernelGGL((gmm_moments_kernel<4>), grid, dim3(64), 0, stream, args);         \
        else if ((plan).nj == 2) hipLaunchKernelGGL((gmm_moments_kernel<2>), grid, dim3(64), 0, stream, args);    \
        else hipLaunchKernelGGL((gmm_moments_kernel<1>), grid, dim3(64), 0, stream, args);                        \
        DINV_CHECK_LAUNCH();                                                                                     \
    } while (0)

}  // namespace dinv
