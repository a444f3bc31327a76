// Total variation on hand-written kernels (gfx950): the over-relaxed Chambolle-Pock iteration of TVDenoiser /
// TVL1Denoiser, the finite differences and their adjoint, and the TVPrior value and subgradient.
//
// Replaces the ATen launches behind
//   TVDenoiser.forward                 deepinv/models/tv.py:86-152 (about 20 small kernels and one host sync per iteration)
//   TVDenoiser.nabla / nabla_adjoint   deepinv/models/tv.py:154-218
//   TVL1Denoiser.prox_sigma_g_conj     deepinv/models/tv.py:221-240
//   TVPrior.fn / grad, TVL1Prior.fn    deepinv/optim/prior.py:485-612
//
// Layout: the image is [planes, D, H, W] (D = 1 for 2-D images; planes = batch * channels), the gradient field
// [planes, D, H, W, nd] with the component last (nd = 2: (h, w); nd = 3: (d, h, w)), as the reference stores it.
// Forward differences with a zero last row / column / slice; the adjoint ignores the components on those faces.
//
// One iteration is two launches: tv_cp_step_kernel (the whole pixel update, each thread recomputing the primal values
// of its +1 neighbours from the L2-resident x2, y, u2) and tv_cp_check_kernel (one workgroup: fixed-order sum of the
// per-workgroup partials, the stopping test, the device iteration counter).  Which buffer of each ping-pong pair is
// current is decided on the device from that counter, so launches enqueued after convergence are no-ops and the result
// is the iterate at which the reference breaks.  No float atomics: every reduction is fixed-order (bit-reproducible).
#include "tv_common.hpp"

#include <cmath>

using namespace dinv;

namespace {

// (nabla^T v)[p] in the reference's order (tv.py:199-216): per axis, minus the own component (not on the last face),
// plus the -1 neighbour's component (not on the first face)
template <int ND>
__device__ __forceinline__ float div_at(const Geo& g, const float* __restrict__ v, int64_t p, int d, int h, int w) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        int n, c; int64_t s;
        axis<ND>(g, k, d, h, w, n, c, s);
        if (c < n - 1) acc -= v[p * ND + k];
        if (c > 0) acc += v[(p - s) * ND + k];
    }
    return acc;
}

// primal step x = (x2 - tau nabla^T u2 + tau y) / (1 + tau) at pixel p (tv.py:73-77, 133)
template <int ND>
__device__ __forceinline__ float primal_at(const Geo& g, const float* __restrict__ x2, const float* __restrict__ y,
                                           const float* __restrict__ u2, float tau, float opt, int64_t p, int d, int h, int w) {
    const float t = x2[p] - tau * div_at<ND>(g, u2, p, d, h, w);
    return (t + tau * y[p]) / opt;
}

// One over-relaxed Chambolle-Pock iteration (tv.py:131-139) on the current buffers (index st[1] & 1), written to the
// other ones; per-workgroup partial sums of |x2_prev - x2|^2 and |x2 + 1e-12|^2 (tv.py:141-143).  No-op once st[0] is set.
template <int ND>
__global__ __launch_bounds__(kThreads) void tv_cp_step_kernel(Geo g, int64_t n, float* __restrict__ xa, float* __restrict__ xb,
                                                              float* __restrict__ ua, float* __restrict__ ub,
                                                              const float* __restrict__ y, const float* __restrict__ lam,
                                                              int aniso, float tau, float opt, float sigma, float rho,
                                                              float* __restrict__ partial, const int32_t* __restrict__ st) {
    if (st[0]) return;
    const bool odd = st[1] & 1;
    const float* __restrict__ x2 = odd ? xb : xa;
    const float* __restrict__ u2 = odd ? ub : ua;
    float* __restrict__ xo = odd ? xa : xb;
    float* __restrict__ uo = odd ? ua : ub;
    float sd = 0.f, sn = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads) {
        int pl, d, h, w;
        coords(g, p, pl, d, h, w);
        const float l = lam[pl / g.planes_per_sample];
        const float xc = x2[p];
        const float x = primal_at<ND>(g, x2, y, u2, tau, opt, p, d, h, w);
        const float z = 2.f * x - xc;
        float v[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            int nk, c; int64_t s;
            axis<ND>(g, k, d, h, w, nk, c, s);
            float gk = 0.f;
            if (c < nk - 1) {
                int dd = d, hh = h, ww = w;
                if (k + (3 - ND) == 0) ++dd; else if (k + (3 - ND) == 1) ++hh; else ++ww;
                const float xn = primal_at<ND>(g, x2, y, u2, tau, opt, p + s, dd, hh, ww);
                gk = (2.f * xn - x2[p + s]) - z;
            }
            v[k] = u2[p * ND + k] + sigma * gk;
        }
        if (aniso) {
#pragma unroll
            for (int k = 0; k < ND; ++k) v[k] = fminf(fmaxf(v[k], -l), l);           // tv.py:239-240
        } else {
            float s2 = 0.f;
#pragma unroll
            for (int k = 0; k < ND; ++k) s2 += v[k] * v[k];
            const float den = fmaxf(sqrtf(s2) / l, 1.0f);                           // tv.py:79-84
#pragma unroll
            for (int k = 0; k < ND; ++k) v[k] = v[k] / den;
        }
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            const float uc = u2[p * ND + k];
            uo[p * ND + k] = uc + rho * (v[k] - uc);
        }
        const float xn = xc + rho * (x - xc);
        xo[p] = xn;
        const float e = xc - xn, q = xn + 1e-12f;
        sd += e * e;
        sn += q * q;
    }
    __shared__ float red[2][kThreads / 64];
    sd = wave_sum(sd);
    sn = wave_sum(sn);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sd; red[1][threadIdx.x >> 6] = sn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        partial[2 * blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// st[1] += 1 (the iteration of index st[1] has run); st[0] = 1 when that index is > 1 and
// sqrt(sum d) / sqrt(sum n) < crit (tv.py:141-148).  One workgroup, fixed order, double accumulators.
__global__ __launch_bounds__(kThreads) void tv_cp_check_kernel(int nblk, const float* __restrict__ partial, float crit,
                                                               int32_t* __restrict__ st) {
    if (st[0]) return;
    double sd = 0.0, sn = 0.0;
    for (int k = threadIdx.x; k < nblk; k += kThreads) {
        sd += (double)partial[2 * k];
        sn += (double)partial[2 * k + 1];
    }
    __shared__ double red[2][kThreads / 64];
    sd = wave_sum_d(sd);
    sn = wave_sum_d(sn);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sd; red[1][threadIdx.x >> 6] = sn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        const double b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const float rel = (float)sqrt(a) / (float)sqrt(b);
        const int it = st[1];
        st[1] = it + 1;
        if (it > 1 && rel < crit) st[0] = 1;
    }
}

// out[p, k] = x[p + e_k] - x[p] (0 on the last face of axis k)   (tv.py:154-184)
template <int ND>
__global__ __launch_bounds__(kThreads) void tv_nabla_kernel(Geo g, int64_t n, const float* __restrict__ x, float* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads) {
        int pl, d, h, w;
        coords(g, p, pl, d, h, w);
        const float xc = x[p];
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            int nk, c; int64_t s;
            axis<ND>(g, k, d, h, w, nk, c, s);
            out[p * ND + k] = c < nk - 1 ? x[p + s] - xc : 0.f;
        }
    }
}

// out[p] = (nabla^T v)[p]   (tv.py:186-218)
template <int ND>
__global__ __launch_bounds__(kThreads) void tv_nabla_adjoint_kernel(Geo g, int64_t n, const float* __restrict__ v, float* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads) {
        int pl, d, h, w;
        coords(g, p, pl, d, h, w);
        out[p] = div_at<ND>(g, v, p, d, h, w);
    }
}

// component k of Dx / |Dx| at pixel p (0 where |Dx| = 0)   (prior.py:565-580)
template <int ND>
__device__ __forceinline__ float normalized_grad(const Geo& g, const float* __restrict__ x, int64_t p, int d, int h, int w, int kk) {
    float v[ND];
    float s2 = 0.f;
    const float xc = x[p];
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        int nk, c; int64_t s;
        axis<ND>(g, k, d, h, w, nk, c, s);
        v[k] = c < nk - 1 ? x[p + s] - xc : 0.f;
        s2 += v[k] * v[k];
    }
    const float nrm = sqrtf(s2);
    return nrm > 0.f ? v[kk] / nrm : 0.f;
}

// out = nabla^T (Dx / |Dx|), each output recomputing the normalised gradients it reads   (prior.py:554-582)
template <int ND>
__global__ __launch_bounds__(kThreads) void tv_grad_kernel(Geo g, int64_t n, const float* __restrict__ x, float* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads) {
        int pl, d, h, w;
        coords(g, p, pl, d, h, w);
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            int nk, c; int64_t s;
            axis<ND>(g, k, d, h, w, nk, c, s);
            if (c < nk - 1) acc -= normalized_grad<ND>(g, x, p, d, h, w, k);
            if (c > 0) {
                int dd = d, hh = h, ww = w;
                if (k + (3 - ND) == 0) --dd; else if (k + (3 - ND) == 1) --hh; else --ww;
                acc += normalized_grad<ND>(g, x, p - s, dd, hh, ww, k);
            }
        }
        out[p] = acc;
    }
}

// partial[b][blk] = sum over this workgroup's pixels of sample b of |Dx|_2 (mode 0) or |Dx|_1 (mode 1)
template <int ND>
__global__ __launch_bounds__(kThreads) void tv_fn_partial_kernel(Geo g, int64_t per_sample, int mode, const float* __restrict__ x,
                                                                 float* __restrict__ partial) {
    const int b = blockIdx.y;
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < per_sample; i += (int64_t)gridDim.x * kThreads) {
        const int64_t p = (int64_t)b * per_sample + i;
        int pl, d, h, w;
        coords(g, p, pl, d, h, w);
        const float xc = x[p];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            int nk, c; int64_t st;
            axis<ND>(g, k, d, h, w, nk, c, st);
            const float v = c < nk - 1 ? x[p + st] - xc : 0.f;
            s += mode ? fabsf(v) : v * v;
        }
        acc += mode ? s : sqrtf(s);
    }
    __shared__ float red[kThreads / 64];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[b] = sum_k partial[b][k] in fixed order (one wave per sample)
__global__ __launch_bounds__(64) void tv_fn_final_kernel(int nblk, const float* __restrict__ partial, float* __restrict__ out) {
    const int b = blockIdx.x;
    float acc = 0.f;
    for (int k = threadIdx.x; k < nblk; k += 64) acc += partial[(int64_t)b * nblk + k];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) out[b] = acc;
}

int make_geo(int32_t nd, int64_t planes, int32_t D, int32_t H, int32_t W, Geo& g, int64_t& n) {
    DINV_REQUIRE(nd == 2 || nd == 3, "tv: nd must be 2 or 3 (got %d)", nd);
    DINV_REQUIRE(planes > 0 && D > 0 && H > 0 && W > 0 && (nd == 3 || D == 1), "tv: bad shape");
    g.D = D; g.H = H; g.W = W;
    g.plane = (int64_t)D * H * W;
    g.planes_per_sample = 1;
    n = planes * g.plane;
    DINV_REQUIRE(n * nd < ((int64_t)1 << 31), "tv: tensor too large (n * nd must stay below 2^31)");
    return 0;
}

}  // namespace

extern "C" int32_t dinv_tv_cp_partials(int64_t n) { return (int32_t)grid_for(n); }

extern "C" int dinv_tv_cp_iter(int32_t nd, int32_t batch, int32_t channels, int32_t D, int32_t H, int32_t W, float* xa, float* xb,
                               float* ua, float* ub, const float* y, const float* lam, int32_t aniso, float tau,
                               float sigma, float rho, float crit, float* partial, int32_t* state, dinv_stream_t stream) {
    Geo g;
    int64_t n;
    DINV_REQUIRE(batch > 0 && channels > 0, "tv: bad batch / channels");
    if (int rc = make_geo(nd, (int64_t)batch * channels, D, H, W, g, n)) return rc;
    DINV_REQUIRE(xa && xb && ua && ub && y && lam && partial && state, "tv: null operand");
    DINV_REQUIRE(xa != xb && ua != ub && (const float*)xa != y && (const float*)xb != y, "tv: ping-pong buffers must be distinct");
    g.planes_per_sample = channels;
    const unsigned nblk = grid_for(n);
    const float opt = 1.0f + tau;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (nd == 2)
        hipLaunchKernelGGL(tv_cp_step_kernel<2>, dim3(nblk), dim3(kThreads), 0, s, g, n, xa, xb, ua, ub, y, lam, aniso ? 1 : 0,
                           tau, opt, sigma, rho, partial, (const int32_t*)state);
    else
        hipLaunchKernelGGL(tv_cp_step_kernel<3>, dim3(nblk), dim3(kThreads), 0, s, g, n, xa, xb, ua, ub, y, lam, aniso ? 1 : 0,
                           tau, opt, sigma, rho, partial, (const int32_t*)state);
    hipLaunchKernelGGL(tv_cp_check_kernel, dim3(1), dim3(kThreads), 0, s, (int)nblk, (const float*)partial, crit, state);
    DINV_CHECK_LAUNCH();
    return 0;
}

extern "C" int dinv_tv_nabla(int32_t nd, int64_t planes, int32_t D, int32_t H, int32_t W, const float* x, float* out,
                             dinv_stream_t stream) {
    Geo g;
    int64_t n;
    if (int rc = make_geo(nd, planes, D, H, W, g, n)) return rc;
    DINV_REQUIRE(x && out && (const float*)out != x, "tv: bad operands");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (nd == 2) hipLaunchKernelGGL(tv_nabla_kernel<2>, dim3(grid_for(n)), dim3(kThreads), 0, s, g, n, x, out);
    else hipLaunchKernelGGL(tv_nabla_kernel<3>, dim3(grid_for(n)), dim3(kThreads), 0, s, g, n, x, out);
    DINV_CHECK_LAUNCH();
    return 0;
}

extern "C" int dinv_tv_nabla_adjoint(int32_t nd, int64_t planes, int32_t D, int32_t H, int32_t W, const float* v, float* out,
                                     dinv_stream_t stream) {
    Geo g;
    int64_t n;
    if (int rc = make_geo(nd, planes, D, H, W, g, n)) return rc;
    DINV_REQUIRE(v && out && (const float*)out != v, "tv: bad operands");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (nd == 2) hipLaunchKernelGGL(tv_nabla_adjoint_kernel<2>, dim3(grid_for(n)), dim3(kThreads), 0, s, g, n, v, out);
    else hipLaunchKernelGGL(tv_nabla_adjoint_kernel<3>, dim3(grid_for(n)), dim3(kThreads), 0, s, g, n, v, out);
    DINV_CHECK_LAUNCH();
    return 0;
}

extern "C" int dinv_tv_grad(int32_t nd, int64_t planes, int32_t D, int32_t H, int32_t W, const float* x, float* out,
                            dinv_stream_t stream) {
    Geo g;
    int64_t n;
    if (int rc = make_geo(nd, planes, D, H, W, g, n)) return rc;
    DINV_REQUIRE(x && out && (const float*)out != x, "tv: bad operands");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (nd == 2) hipLaunchKernelGGL(tv_grad_kernel<2>, dim3(grid_for(n)), dim3(kThreads), 0, s, g, n, x, out);
    else hipLaunchKernelGGL(tv_grad_kernel<3>, dim3(grid_for(n)), dim3(kThreads), 0, s, g, n, x, out);
    DINV_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t dinv_tv_fn_blocks(int64_t per_sample) {
    return (int32_t)std::min<int64_t>(std::max<int64_t>(ceil_div(per_sample, 4 * kThreads), 1), 256);
}

extern "C" int dinv_tv_fn(int32_t nd, int32_t mode, int32_t batch, int32_t channels, int32_t D, int32_t H, int32_t W,
                          const float* x, float* out, float* partial, dinv_stream_t stream) {
    Geo g;
    int64_t n;
    DINV_REQUIRE(batch > 0 && batch <= 65535 && channels > 0 && (mode == 0 || mode == 1), "tv: bad batch / channels / mode");
    if (int rc = make_geo(nd, (int64_t)batch * channels, D, H, W, g, n)) return rc;
    DINV_REQUIRE(x && out && partial, "tv: null operand");
    const int64_t per = n / batch;
    const int nblk = dinv_tv_fn_blocks(per);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (nd == 2) hipLaunchKernelGGL(tv_fn_partial_kernel<2>, dim3(nblk, batch), dim3(kThreads), 0, s, g, per, mode, x, partial);
    else hipLaunchKernelGGL(tv_fn_partial_kernel<3>, dim3(nblk, batch), dim3(kThreads), 0, s, g, per, mode, x, partial);
    hipLaunchKernelGGL(tv_fn_final_kernel, dim3(batch), dim3(64), 0, s, nblk, (const float*)partial, out);
    DINV_CHECK_LAUNCH();
    return 0;
}
