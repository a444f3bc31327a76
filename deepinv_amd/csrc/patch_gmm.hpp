// Gaussian-mixture patch prior (EPLL) on the fp32 matrix cores (gfx950): the kernels and the host planning behind the dinv_gmm_*
// entry points of dense.hip.
//
// Replaces the ATen launches behind
//   GaussianMixtureModel.component_log_likelihoods / forward / classify     deepinv/optim/utils.py:261-312
//   EPLL._reconstruction_step                                              deepinv/optim/epll.py:167-229
//
// The model is held in its eigenbasis, Sigma_k = Q_k diag(lam_k) Q_k^T, so that the regularisation r of a half-quadratic step
// (Sigma_k + r I) is a runtime scalar per image and no matrix is rebuilt between steps:
//   Wt   [K dp, d]  the stacked Q_k^T: row k dp + i is eigenvector i of component k, dp = d rounded up to a multiple of 4;
//                   the dp - d padding rows of a component are zero
//   m    [K dp]     Q_k^T mu_k, zero in the padding
//   lam  [K dp]     eigenvalues, one in the padding (a padding row adds (0 - 0)^2 / (1 + r) = 0 and no log term)
//   logw [K]        log weights (null: not added, component_log_likelihoods)
//   t_k = Q_k^T x,   score_k = logw_k - 1/2 sum_i log(lam_ki + r) - 1/2 sum_i (t_ki - m_ki)^2 / (lam_ki + r) - d/2 log 2 pi
//   z   = Q_k* diag(lam_k*i / (lam_k*i + r)) Q_k*^T x          (the reference ignores mu here, epll.py:205-211)
//
// gmm_score_kernel<IMAGE, NP>: a workgroup of 4 waves; a wave owns NP tiles of 32 patches (the B side of
// v_mfma_f32_32x32x2_f32) and walks the K d rows of Wt in tiles of 32 (the A side), so D element e of lane l is row
// (e & 3) + 8 (e >> 2) + 4 (l >> 5) of the tile for patch l & 31.  T = Wt P is never stored: after each tile the lane folds its
// 16 rows into the quadratic form of the component(s) the tile covers, the two half waves are added once a component is complete
// and a component that straddles tiles is carried in a register.  Components start at multiples of 4 rows, so which half wave
// holds eigenvector i and the order in which a half adds its terms depend on i alone, not on where the component lies in a
// tile: identical components get identical bits, and a tie goes to the lowest index.  The padded work is dp / d - 1 (a third at
// d = 9, 4 % at d = 27, none at 16, 36, 108, 192), the last tile of K dp rows and an odd d's last k.
// Operand sources: rows [N, d] read from memory (patch n of a wave tile is row n), or an image [B, C, H, W] staged in LDS as a
// tile of (4 NP + p - 1) x (32 + p - 1) pixels per channel, where entry (c, dy, dx) of a patch is a constant offset and
// consecutive lanes are consecutive x0; the patch matrix never exists.  The per-image table
// c_k = logw_k - 1/2 sum_i log(lam_ki + r) - d/2 log 2 pi is computed by each workgroup into LDS in its prologue, in fp64 from the
// fp32 lam_ki + r, and kept as two floats c_k = hi_k + lo_k: score = hi + (lo - q / 2).  A single float at |c_k| of about 100
// is off by up to 8e-6, the same for every patch of a component, which does not average out in a mean log-likelihood (the
// objective of EM); with the pair the only roundings left are per patch.  Epilogues: SCORES
// stores [N, K]; ARGMAX keeps a running best over ascending k with strict > (the lowest index wins a tie, like torch.max) and
// stores int32 [N]; NLL keeps an online log-sum-exp and stores -log sum_k exp(score_k) [N]; POSTERIOR (rows mode, behind
// dinv_gmm_posterior only) is NLL that also stores the responsibilities exp(score_k - lse) [N, K]: the two half waves hold the
// same scores, so half h stores the scores of the components k = h mod 2 and rescales exactly those entries of its own row once
// lse is known - one launch, no exchange, and -lse is computed by the instructions of NLL.
// gmm_estimate_kernel: one wave per patch, z from the gathered Q_k* in two d x d matrix-vector products through LDS -> [N, d].
// gmm_aggregate_kernel: one thread per pixel adds the <= p^2 covering patch entries in ascending (y0, x0), divides by the closed-
// form multiplicity and applies out = a[b] x~ + cb[b] bias.  No atomics anywhere: results are bitwise reproducible, and a patch's
// score does not depend on NP or on the image it is batched with.
//
// Limits (DINV_REQUIRE): d = C p^2 (image mode); H, W >= p; K >= 1, d >= 1, K dp < 2^31; patches < 2^31; the LDS of a workgroup
// (4 (2 K + d + C (4 NP + p - 1)(32 + p - 1)) bytes) within 160 KB, which admits d = 192 (p = 8, C = 3) with K in the thousands.
// lam + r > 0 is the caller's contract (the Python layer checks it when it builds the operands).  Nothing is launched for an empty
// batch.
#pragma once
#include "dense_core.hpp"

namespace dinv {

constexpr int kGmmWaves = 4;             // waves per workgroup of the score kernel
constexpr int kGmmTargetGroups = 256;    // one workgroup per compute unit of an MI355X before a wave takes more patch tiles
constexpr int kGmmEstPatches = 4;        // patches per workgroup of the estimate kernel
constexpr double kLog2Pi = 1.8378770664093453;
constexpr int kGmmPosterior = DINV_GMM_NLL + 1;     // the epilogue of dinv_gmm_posterior: not one dinv_gmm_scores accepts

// rows per component in Wt, m and lam
__host__ __device__ inline int gmm_dp(int d) { return (d + 3) & ~3; }

struct GmmModel {
    const float* Wt;
    const float* m;
    const float* lam;
    const float* logw;
    int K, d;
};

struct GmmScoreArgs {
    GmmModel g;
    const float* src;      // rows [N, d] or image [B, C, H, W]
    const float* r;        // [B] (rows: [1]) or null
    void* out;
    float* nll;            // POSTERIOR: [N] beside the responsibilities in out
    int64_t N;             // rows mode: rows
    int C, H, W, p, PH, PW;
    int epilogue;
};

template <bool IMAGE, int NP>
__global__ __launch_bounds__(256) void gmm_score_kernel(GmmScoreArgs a) {
    DINV_DYN_LDS(float, lds);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 31, h = lane >> 5;
    const int d = a.g.d, K = a.g.K, dk = (d + 1) & ~1, dp = gmm_dp(d);
    float* cst = lds;                                      // [2, K]: hi, lo
    int* offk = reinterpret_cast<int*>(lds + 2 * K);       // [dk]
    float* tile = lds + 2 * K + dk;                        // [C, TYP, TXP]
    const int b = IMAGE ? (int)blockIdx.z : 0;
    const float r = a.r ? a.r[b] : 0.f;
    for (int k = tid; k < K; k += 256) {
        double s = 0.0;
        for (int i = 0; i < d; ++i) s += log((double)(a.g.lam[(int64_t)k * dp + i] + r));
        const double c = (a.g.logw ? (double)a.g.logw[k] : 0.0) - 0.5 * s - 0.5 * (double)d * kLog2Pi;
        const float hi = (float)c;
        cst[k] = hi;
        cst[K + k] = (float)(c - (double)hi);
    }
    const int TYP = kGmmWaves * NP + a.p - 1, TXP = 32 + a.p - 1;
    const int tx0 = (int)blockIdx.x * 32, ty0 = (int)blockIdx.y * kGmmWaves * NP;
    if (IMAGE) {
        const int pp = a.p * a.p;
        for (int k = tid; k < dk; k += 256) {
            const int c = k / pp, dy = (k % pp) / a.p, dx = k % a.p;
            offk[k] = k < d ? (c * TYP + dy) * TXP + dx : 0;
        }
        const int plane = TYP * TXP;
        for (int e = tid; e < a.C * plane; e += 256) {
            const int c = e / plane, yy = (e % plane) / TXP, xx = e % TXP;
            const int y = ty0 + yy, x = tx0 + xx;
            tile[e] = (y < a.H && x < a.W) ? a.src[(((int64_t)b * a.C + c) * a.H + y) * a.W + x] : 0.f;
        }
    }
    __syncthreads();

    // the patches of this lane, and how many of the wave's NP tiles hold any patch (wave-uniform)
    int64_t n[NP];
    bool valid[NP];
    int base[NP];
    int na;
    if (IMAGE) {
        const int y00 = ty0 + w * NP;
        na = a.PH - y00;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int y0 = y00 + q, x0 = tx0 + j;
            valid[q] = y0 < a.PH && x0 < a.PW;
            n[q] = ((int64_t)b * a.PH + y0) * a.PW + x0;
            base[q] = (w * NP + q) * TXP + j;
        }
    } else {
        const int64_t n00 = ((int64_t)blockIdx.x * kGmmWaves + w) * NP * 32;
        const int64_t left = a.N - n00;
        na = left <= 0 ? 0 : (int)((left + 31) / 32 > NP ? NP : (left + 31) / 32);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            n[q] = n00 + q * 32 + j;
            valid[q] = n[q] < a.N;
            base[q] = 0;
        }
    }
    if (na > NP) na = NP;
    if (na <= 0) return;

    const int64_t rows = (int64_t)K * dp;
    const int ntiles = (int)((rows + 31) / 32);
    float carry[NP], best[NP], sum[NP];
    int bestk[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) { carry[q] = 0.f; best[q] = -INFINITY; sum[q] = 0.f; bestk[q] = 0; }

    for (int t = 0; t < ntiles; ++t) {
        const int64_t g0 = (int64_t)t * 32;
        f32x16 acc[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
        const bool grow = g0 + j < rows;
        const float* wrow = a.g.Wt + (grow ? g0 + j : 0) * d;
        for (int s = 0; s < dk / 2; ++s) {
            const int kk = 2 * s + h;
            const bool ok = kk < d;
            const float av = (grow && ok) ? wrow[kk] : 0.f;
            const int off = IMAGE ? offk[kk] : kk;
#pragma unroll
            for (int q = 0; q < NP; ++q)
                if (q < na) {
                    float bv = 0.f;
                    if (IMAGE) bv = ok ? tile[base[q] + off] : 0.f;
                    else if (ok && valid[q]) bv = a.src[n[q] * d + off];
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[q], 0, 0, 0);
                }
        }
        // the 16 rows of this lane: mean and 1 / (lam + r)
        float mq[16], wq[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t ge = g0 + (e & 3) + 8 * (e >> 2) + 4 * h;
            const bool in = ge < rows;
            mq[e] = in ? a.g.m[ge] : 0.f;
            wq[e] = in ? 1.f / (a.g.lam[ge] + r) : 0.f;
        }
        const int k_lo = (int)(g0 / dp);
        int k_hi = (int)((g0 + 31) / dp);
        if (k_hi > K - 1) k_hi = K - 1;
        for (int k = k_lo; k <= k_hi; ++k) {
            const int64_t lo = (int64_t)k * dp - g0, hi = lo + dp;     // rows [lo, hi) of the tile belong to component k
            const bool ends = hi <= 32;
            const float chi = cst[k], clo = cst[K + k];
#pragma unroll
            for (int q = 0; q < NP; ++q)
                if (q < na) {
                    float qf = k == k_lo ? carry[q] : 0.f;
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int re = (e & 3) + 8 * (e >> 2) + 4 * h;
                        if (re >= lo && re < hi) {
                            const float df = acc[q][e] - mq[e];
                            qf = fmaf(df * df, wq[e], qf);
                        }
                    }
                    if (!ends) { carry[q] = qf; continue; }
                    carry[q] = 0.f;
                    const float score = chi + (clo - 0.5f * (qf + __shfl_xor(qf, 32)));
                    if (a.epilogue == DINV_GMM_SCORES) {
                        if (h == 0 && valid[q]) static_cast<float*>(a.out)[n[q] * K + k] = score;
                    } else if (a.epilogue == DINV_GMM_ARGMAX) {
                        if (score > best[q]) { best[q] = score; bestk[q] = k; }
                    } else {
                        if (a.epilogue == kGmmPosterior && (k & 1) == h && valid[q]) static_cast<float*>(a.out)[n[q] * K + k] = score;
                        if (score > best[q]) { sum[q] = sum[q] * expf(best[q] - score) + 1.f; best[q] = score; }
                        else if (score > -INFINITY) sum[q] += expf(score - best[q]);      // a zero weight adds nothing
                    }
                }
        }
    }
    if (a.epilogue == kGmmPosterior) {
#pragma unroll
        for (int q = 0; q < NP; ++q)
            if (q < na && valid[q]) {
                const float lse = best[q] + logf(sum[q]);
                float* row = static_cast<float*>(a.out) + n[q] * K;
                for (int k = h; k < K; k += 2) row[k] = expf(row[k] - lse);      // exp(-inf - lse) = 0: a zero weight
                if (h == 0) a.nll[n[q]] = -lse;
            }
        return;
    }
    if (h != 0) return;
#pragma unroll
    for (int q = 0; q < NP; ++q)
        if (q < na && valid[q]) {
            if (a.epilogue == DINV_GMM_ARGMAX) static_cast<int32_t*>(a.out)[n[q]] = bestk[q];
            else if (a.epilogue == DINV_GMM_NLL) static_cast<float*>(a.out)[n[q]] = -(best[q] + logf(sum[q]));
        }
}

struct GmmEstimateArgs {
    GmmModel g;
    const float* x;        // [B, C, H, W]
    const float* r;        // [B]
    const int32_t* kstar;  // [N]
    float* z;              // [N, d]
    int64_t N;
    int C, H, W, p, PH, PW;
};

__global__ __launch_bounds__(64) void gmm_estimate_kernel(GmmEstimateArgs a) {
    DINV_DYN_LDS(float, lds);
    const int lane = threadIdx.x, d = a.g.d, dp = gmm_dp(d), pp = a.p * a.p;
    float* xs = lds;       // [d] the patch
    float* ts = lds + d;   // [d] lam / (lam + r) Q^T x
    const int64_t per = (int64_t)a.PH * a.PW;
    for (int q = 0; q < kGmmEstPatches; ++q) {
        const int64_t n = (int64_t)blockIdx.x * kGmmEstPatches + q;
        if (n >= a.N) break;
        const int b = (int)(n / per), y0 = (int)((n % per) / a.PW), x0 = (int)(n % a.PW);
        int k = a.kstar[n];
        k = k < 0 ? 0 : (k > a.g.K - 1 ? a.g.K - 1 : k);
        const float r = a.r[b];
        for (int jj = lane; jj < d; jj += 64) {
            const int c = jj / pp, dy = (jj % pp) / a.p, dx = jj % a.p;
            xs[jj] = a.x[(((int64_t)b * a.C + c) * a.H + y0 + dy) * a.W + x0 + dx];
        }
        __syncthreads();
        const float* Q = a.g.Wt + (int64_t)k * dp * d;
        for (int i = lane; i < d; i += 64) {
            const float* row = Q + (int64_t)i * d;
            float t = 0.f;
            for (int jj = 0; jj < d; ++jj) t = fmaf(row[jj], xs[jj], t);
            const float l = a.g.lam[(int64_t)k * dp + i];
            ts[i] = t * (l / (l + r));
        }
        __syncthreads();
        for (int jj = lane; jj < d; jj += 64) {
            float z = 0.f;
            for (int i = 0; i < d; ++i) z = fmaf(Q[(int64_t)i * d + jj], ts[i], z);
            a.z[n * d + jj] = z;
        }
        __syncthreads();
    }
}

struct GmmAggregateArgs {
    const float* z;        // [N, d]
    const float* a;        // [B]
    const float* cb;       // [B] or null (1)
    const float* bias;     // [B, C, H, W] or null
    float* out;
    int64_t total;
    int d, C, H, W, p, PH, PW;
};

__global__ __launch_bounds__(256) void gmm_aggregate_kernel(GmmAggregateArgs a) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < a.total; idx += (int64_t)gridDim.x * 256) {
        const int x = (int)(idx % a.W), y = (int)((idx / a.W) % a.H);
        const int c = (int)((idx / ((int64_t)a.W * a.H)) % a.C), b = (int)(idx / ((int64_t)a.W * a.H * a.C));
        const int ylo = y - a.p + 1 > 0 ? y - a.p + 1 : 0, yhi = y < a.H - a.p ? y : a.H - a.p;
        const int xlo = x - a.p + 1 > 0 ? x - a.p + 1 : 0, xhi = x < a.W - a.p ? x : a.W - a.p;
        float s = 0.f;
        for (int y0 = ylo; y0 <= yhi; ++y0)
            for (int x0 = xlo; x0 <= xhi; ++x0) {
                const int64_t n = ((int64_t)b * a.PH + y0) * a.PW + x0;
                s += a.z[n * a.d + (c * a.p + (y - y0)) * a.p + (x - x0)];
            }
        const float xt = s / (float)((yhi - ylo + 1) * (xhi - xlo + 1));
        const float bias = a.bias ? (a.cb ? a.cb[b] : 1.f) * a.bias[idx] : 0.f;
        a.out[idx] = fmaf(a.a[b], xt, bias);
    }
}

// ---------------------------------------------------------------- host planning
struct GmmPlan {
    bool empty;
    int np;                // patch tiles per wave: 1, 2 or 4
    int PH, PW;
    int64_t N;             // patches of the call
    size_t lds;
    dim3 grid;
};

inline int gmm_check_model(const char* op, const GmmModel& g) {
    DINV_REQUIRE(g.K >= 1 && g.d >= 1, "%s: bad model K = %d, d = %d", op, g.K, g.d);
    DINV_REQUIRE((int64_t)g.K * gmm_dp(g.d) < ((int64_t)1 << 31), "%s: K d = %lld rows exceed 2^31", op, (long long)g.K * g.d);
    DINV_REQUIRE(g.Wt && g.m && g.lam, "%s: the model operands Wt, m and lam must be non-null", op);
    return 0;
}

// the largest NP of 4, 2 whose grid still has kGmmTargetGroups workgroups, else 1.  A function of the shape only.
inline int gmm_np(int64_t groups_at[3]) {
    if (groups_at[2] >= kGmmTargetGroups) return 4;
    if (groups_at[1] >= kGmmTargetGroups) return 2;
    return 1;
}

inline size_t gmm_score_lds(const GmmModel& g, int C, int p, int np, bool image) {
    const int dk = (g.d + 1) & ~1;
    size_t words = 2 * (size_t)g.K + dk;
    if (image) words += (size_t)C * (kGmmWaves * np + p - 1) * (32 + p - 1);
    return words * sizeof(float);
}

inline int gmm_plan_rows(const char* op, const GmmModel& g, int64_t N, GmmPlan* pl) {
    if (int e = gmm_check_model(op, g)) return e;
    DINV_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), "%s: %lld rows, the patch count must be below 2^31", op, (long long)N);
    pl->empty = N == 0;
    pl->N = N;
    pl->PH = pl->PW = 0;
    if (pl->empty) return 0;
    int64_t at[3];
    for (int i = 0; i < 3; ++i) at[i] = ceil_div(N, (int64_t)32 * kGmmWaves << i);
    pl->np = gmm_np(at);
    pl->grid = dim3((unsigned)at[pl->np == 4 ? 2 : pl->np == 2 ? 1 : 0]);
    pl->lds = gmm_score_lds(g, 0, 0, pl->np, false);
    DINV_REQUIRE(pl->lds <= kMaxLdsBytes, "%s: K = %d needs %zu bytes of LDS, a workgroup has %zu", op, g.K, pl->lds, kMaxLdsBytes);
    return 0;
}

inline int gmm_plan_image(const char* op, const GmmModel& g, int64_t B, int C, int H, int W, int p, GmmPlan* pl) {
    if (int e = gmm_check_model(op, g)) return e;
    DINV_REQUIRE(B >= 0 && C >= 1 && p >= 1 && H >= 1 && W >= 1, "%s: bad shape B = %lld, C = %d, H = %d, W = %d, p = %d", op,
                 (long long)B, C, H, W, p);
    DINV_REQUIRE((int64_t)C * p * p == g.d, "%s: patches of C p^2 = %lld entries, the model has dimension d = %d", op,
                 (long long)C * p * p, g.d);
    DINV_REQUIRE(H >= p && W >= p, "%s: a %d x %d image holds no %d x %d patch", op, H, W, p, p);
    pl->PH = H - p + 1;
    pl->PW = W - p + 1;
    DINV_REQUIRE(B < 65536 && B * pl->PH * pl->PW < ((int64_t)1 << 31), "%s: %lld patches, the patch count must be below 2^31", op,
                 (long long)(B * pl->PH * pl->PW));
    pl->N = B * pl->PH * pl->PW;
    pl->empty = B == 0;
    if (pl->empty) return 0;
    int64_t at[3];
    for (int i = 0; i < 3; ++i) at[i] = ceil_div(pl->PW, 32) * ceil_div(pl->PH, kGmmWaves << i) * B;
    pl->np = gmm_np(at);
    const int64_t gy = ceil_div(pl->PH, kGmmWaves * pl->np);
    DINV_REQUIRE(gy < 65536, "%s: image too tall", op);
    pl->grid = dim3((unsigned)ceil_div(pl->PW, 32), (unsigned)gy, (unsigned)B);
    pl->lds = gmm_score_lds(g, C, p, pl->np, true);
    DINV_REQUIRE(pl->lds <= kMaxLdsBytes, "%s: K = %d, C = %d, p = %d need %zu bytes of LDS, a workgroup has %zu", op, g.K, C, p,
                 pl->lds, kMaxLdsBytes);
    return 0;
}

inline int gmm_check_epilogue(const char* op, int epilogue) {
    DINV_REQUIRE(epilogue >= DINV_GMM_SCORES && epilogue <= DINV_GMM_NLL, "%s: unknown epilogue %d", op, epilogue);
    return 0;
}

// One instantiation of the score kernel.  A macro, because a launch is known by the spelling of its kernel expression (the launch
// log of the host emulation).
#define DINV_GMM_LAUNCH_ONE(IMAGE, NP, plan, stream, args)                                                          \
    do {                                                                                                            \
        if ((plan).lds > kDefaultLdsBytes)                                                                          \
            if (int e = raise_lds_cap<gmm_score_kernel<IMAGE, NP>>(kMaxLdsBytes)) return e;                         \
        hipLaunchKernelGGL((gmm_score_kernel<IMAGE, NP>), (plan).grid, dim3(256), (plan).lds, stream, args);        \
        DINV_CHECK_LAUNCH();                                                                                        \
    } while (0)

#define DINV_GMM_LAUNCH_SCORE(IMAGE, plan, stream, args)                                   \
    do {                                                                                   \
        if ((plan).np == 4) DINV_GMM_LAUNCH_ONE(IMAGE, 4, plan, stream, args);             \
        else if ((plan).np == 2) DINV_GMM_LAUNCH_ONE(IMAGE, 2, plan, stream, args);        \
        else DINV_GMM_LAUNCH_ONE(IMAGE, 1, plan, stream, args);                            \
    } while (0)

inline size_t gmm_epll_workspace_bytes(int64_t B, int C, int H, int W, int p) {
    if (B < 1 || C < 1 || p < 1 || H < p || W < p) return 0;
    const int64_t N = B * (H - p + 1) * (W - p + 1);
    return (size_t)N * ((size_t)C * p * p + 1) * sizeof(float);     // z [N, d] and k* [N]
}

}  // namespace dinv
