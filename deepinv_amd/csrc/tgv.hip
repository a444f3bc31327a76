// Total generalized variation (second order) on hand-written kernels (gfx950): the over-relaxed Chambolle-Pock iteration
// of TGVDenoiser and the symmetrised-Jacobian pair epsilon / epsilon^T.
//
// Replaces the ATen launches behind
//   TGVDenoiser.forward                      deepinv/models/tgv.py:93-214 (Python slice loops over nd^2 components, about
//                                            60 small kernels and one host sync per iteration)
//   TGVDenoiser.epsilon / epsilon_adjoint    deepinv/models/tgv.py:230-310
//
// Layout (the reference's): the image x2 and y are [planes, D, H, W] (D = 1 for 2-D images; planes = batch * channels),
// r2 is [planes, D, H, W, nd] and u2 [planes, D, H, W, nd^2] with the component last; component i * nd + j of u2 is the
// derivative of the vector field's component i along spatial axis j.  nabla is TV's forward difference (zero on the last
// face), epsilon a backward difference per component, zero on the first face:
//   eps(I)[p, i nd + j] = I_i(p) - I_i(p - e_j)   (p_j >= 1)
//
// One iteration is three launches:
//   tgv_cp_primal_kernel  t = tau eps^T(u2) at p and p - e_k, x, r, their relaxations x2', r2', and z = 2x - x2,
//                         w = 2r - r2 for the dual step; per-workgroup partials of |x2 - x2'|^2 and |x2'|^2
//   tgv_cp_dual_kernel    u = P(u2 + sigma eps(nabla z - w)) and its relaxation u2'
//   tgv_cp_check_kernel   one workgroup: fixed-order sum of the partials, the stopping test, the device iteration counter
// The two-pass split costs z and w as an extra write and read (25 floats per pixel in 2-D instead of the 15 of one fused
// LDS-tiled launch); DESIGN.md 3.9 has the byte model.  (x2, r2, u2) ping-pong between two buffer sets, the current one
// chosen on the device from the counter, so launches enqueued after convergence are no-ops and the result is the iterate
// at which the reference breaks.  No float atomics: every reduction is fixed-order (bit-reproducible).
#include "tv_common.hpp"

#include <cmath>

using namespace dinv;

namespace {

// per-axis coordinate, extent and pixel stride of pixel p (index k: nd = 2 -> (h, w), nd = 3 -> (d, h, w))
template <int ND>
struct Pix {
    int c[ND], n[ND];
    int64_t s[ND];
    int pl;
};

template <int ND>
__device__ __forceinline__ Pix<ND> pix(const Geo& g, int64_t p) {
    Pix<ND> q;
    int d, h, w;
    coords(g, p, q.pl, d, h, w);
#pragma unroll
    for (int k = 0; k < ND; ++k) axis<ND>(g, k, d, h, w, q.n[k], q.c[k], q.s[k]);
    return q;
}

// a per-pixel record of N floats at p (u2: N = nd^2, r2 / w: N = nd); 16- and 8-byte accesses where the record is
// (the entry points require 16-byte aligned 2-D fields)
template <int N>
__device__ __forceinline__ void load_rec(const float* __restrict__ a, int64_t p, float (&v)[N]) {
    if constexpr (N == 4) {
        const float4 t = *reinterpret_cast<const float4*>(a + p * 4);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else if constexpr (N == 2) {
        const float2 t = *reinterpret_cast<const float2*>(a + p * 2);
        v[0] = t.x; v[1] = t.y;
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = a[p * N + k];
    }
}
template <int N>
__device__ __forceinline__ void store_rec(float* __restrict__ a, int64_t p, const float (&v)[N]) {
    if constexpr (N == 4) {
        *reinterpret_cast<float4*>(a + p * 4) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (N == 2) {
        *reinterpret_cast<float2*>(a + p * 2) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) a[p * N + k] = v[k];
    }
}

// component i of eps^T(u) at pixel q with per-axis coordinates cq, in the reference's order (tgv.py:273-310): per axis j,
// minus the +e_j neighbour's component i nd + j (not on the last face), plus the own one (not on the first face)
template <int ND>
__device__ __forceinline__ float eps_adj_at(const float* __restrict__ u, int64_t q, const int (&cq)[ND], const int (&n)[ND],
                                            const int64_t (&s)[ND], int i) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        if (cq[j] <= n[j] - 2) acc -= u[(q + s[j]) * (ND * ND) + i * ND + j];
        if (cq[j] >= 1) acc += u[q * (ND * ND) + i * ND + j];
    }
    return acc;
}

// The primal half of one iteration (tgv.py:148-151, 158-159) on the current set (index st[1] & 1):
//   t = tau eps^T(u2);  x = (x2 - nabla^T t + tau y) / (1 + tau);  r = s - s / max(|s|_2 / (tau lam1), 1), s = r2 + t
// writes x2' = x2 + rho (x - x2), r2' = r2 + rho (r - r2) to the other set, z = 2x - x2 and w = 2r - r2 for the dual
// half, and per-workgroup partials of |x2 - x2'|^2, |x2'|^2 (tgv.py:162-164).  No-op once st[0] is set.
template <int ND>
__global__ __launch_bounds__(kThreads) void tgv_cp_primal_kernel(Geo g, int64_t n, float* __restrict__ xa, float* __restrict__ xb,
                                                                 float* __restrict__ ra, float* __restrict__ rb,
                                                                 const float* __restrict__ ua, const float* __restrict__ ub,
                                                                 const float* __restrict__ y, const float* __restrict__ lam1,
                                                                 float tau, float opt, float rho, float* __restrict__ z,
                                                                 float* __restrict__ wz, float* __restrict__ partial,
                                                                 const int32_t* __restrict__ st) {
    if (st[0]) return;
    const bool odd = st[1] & 1;
    const float* __restrict__ x2 = odd ? xb : xa;
    const float* __restrict__ r2 = odd ? rb : ra;
    const float* __restrict__ u2 = odd ? ub : ua;
    float* __restrict__ xo = odd ? xa : xb;
    float* __restrict__ ro = odd ? ra : rb;
    float sd = 0.f, sn = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads) {
        const Pix<ND> q = pix<ND>(g, p);
        float t[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) t[i] = tau * eps_adj_at<ND>(u2, p, q.c, q.n, q.s, i);
        // nabla^T t at p in TV's order (tv.py:199-216): component k of t at p - e_k is needed only where p_k >= 1
        float div = 0.f;
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            if (q.c[k] < q.n[k] - 1) div -= t[k];
            if (q.c[k] > 0) {
                int cm[ND];
#pragma unroll
                for (int a = 0; a < ND; ++a) cm[a] = q.c[a] - (a == k);
                div += tau * eps_adj_at<ND>(u2, p - q.s[k], cm, q.n, q.s, k);
            }
        }
        const float xc = x2[p];
        const float x = ((xc - div) + tau * y[p]) / opt;
        float rc[ND], sv[ND], s2 = 0.f;
        load_rec<ND>(r2, p, rc);
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            sv[i] = rc[i] + t[i];
            s2 += sv[i] * sv[i];
        }
        const float den = fmaxf(sqrtf(s2) / (tau * lam1[q.pl / g.planes_per_sample]), 1.0f);   // tgv.py:76-83
        float rn[ND], wv[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const float r = sv[i] - sv[i] / den;
            wv[i] = 2.f * r - rc[i];
            rn[i] = rc[i] + rho * (r - rc[i]);
        }
        store_rec<ND>(ro, p, rn);
        store_rec<ND>(wz, p, wv);
        z[p] = 2.f * x - xc;
        const float xn = xc + rho * (x - xc);
        xo[p] = xn;
        const float e = xc - xn;
        sd += e * e;
        sn += xn * xn;
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

// component i of G = nabla z - w at pixel q (ci: q's coordinate along axis i): TV's forward difference, zero on the last face
template <int ND>
__device__ __forceinline__ float g_at(const float* __restrict__ z, const float* __restrict__ wz, int64_t q, int ci, int ni,
                                      int64_t si, int i) {
    const float dz = ci <= ni - 2 ? z[q + si] - z[q] : 0.f;
    return dz - wz[q * ND + i];
}

// The dual half of one iteration (tgv.py:152-156, 160): u = P(u2 + sigma eps(G)), P(v) = v / max(|v|_2 / lam2, 1) over the
// nd^2 components (tgv.py:85-91); writes u2' = u2 + rho (u - u2) to the other set.  No-op once st[0] is set.
template <int ND>
__global__ __launch_bounds__(kThreads) void tgv_cp_dual_kernel(Geo g, int64_t n, float* __restrict__ ua, float* __restrict__ ub,
                                                               const float* __restrict__ z, const float* __restrict__ wz,
                                                               const float* __restrict__ lam2, float sigma, float rho,
                                                               const int32_t* __restrict__ st) {
    if (st[0]) return;
    const bool odd = st[1] & 1;
    const float* __restrict__ u2 = odd ? ub : ua;
    float* __restrict__ uo = odd ? ua : ub;
    constexpr int NC = ND * ND;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads) {
        const Pix<ND> q = pix<ND>(g, p);
        float gp[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) gp[i] = g_at<ND>(z, wz, p, q.c[i], q.n[i], q.s[i], i);
        float uc[NC], v[NC], s2 = 0.f;
        load_rec<NC>(u2, p, uc);
#pragma unroll
        for (int i = 0; i < ND; ++i) {
#pragma unroll
            for (int j = 0; j < ND; ++j) {
                float e = 0.f;
                if (q.c[j] >= 1) e = gp[i] - g_at<ND>(z, wz, p - q.s[j], q.c[i] - (i == j), q.n[i], q.s[i], i);
                v[i * ND + j] = uc[i * ND + j] + sigma * e;
                s2 += v[i * ND + j] * v[i * ND + j];
            }
        }
        const float den = fmaxf(sqrtf(s2) / lam2[q.pl / g.planes_per_sample], 1.0f);
#pragma unroll
        for (int k = 0; k < NC; ++k) v[k] = uc[k] + rho * (v[k] / den - uc[k]);
        store_rec<NC>(uo, p, v);
    }
}

// st[1] += 1 (the iteration of index st[1] has run); st[0] = 1 when that index is > 1 and
// sqrt(sum d) / (sqrt(sum n) + 1e-12) < crit (tgv.py:162-171).  One workgroup, fixed order, double accumulators.
__global__ __launch_bounds__(kThreads) void tgv_cp_check_kernel(int nblk, const float* __restrict__ partial, float crit,
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
        const float rel = (float)sqrt(a) / ((float)sqrt(b) + 1e-12f);
        const int it = st[1];
        st[1] = it + 1;
        if (it > 1 && rel < crit) st[0] = 1;
    }
}

// out[p, i nd + j] = v_i(p) - v_i(p - e_j), 0 on the first face of axis j   (tgv.py:230-271)
template <int ND>
__global__ __launch_bounds__(kThreads) void tgv_epsilon_kernel(Geo g, int64_t n, const float* __restrict__ v, float* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads) {
        const Pix<ND> q = pix<ND>(g, p);
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const float vc = v[p * ND + i];
#pragma unroll
            for (int j = 0; j < ND; ++j)
                out[p * (ND * ND) + i * ND + j] = q.c[j] >= 1 ? vc - v[(p - q.s[j]) * ND + i] : 0.f;
        }
    }
}

// out[p, i] = (eps^T u)_i(p)   (tgv.py:273-310)
template <int ND>
__global__ __launch_bounds__(kThreads) void tgv_epsilon_adjoint_kernel(Geo g, int64_t n, const float* __restrict__ u, float* __restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kThreads) {
        const Pix<ND> q = pix<ND>(g, p);
#pragma unroll
        for (int i = 0; i < ND; ++i) out[p * ND + i] = eps_adj_at<ND>(u, p, q.c, q.n, q.s, i);
    }
}

int make_geo(int32_t nd, int64_t planes, int32_t D, int32_t H, int32_t W, Geo& g, int64_t& n) {
    DINV_REQUIRE(nd == 2 || nd == 3, "tgv: nd must be 2 or 3 (got %d)", nd);
    DINV_REQUIRE(planes > 0 && D > 0 && H > 0 && W > 0 && (nd == 3 || D == 1), "tgv: bad shape");
    g.D = D; g.H = H; g.W = W;
    g.plane = (int64_t)D * H * W;
    g.planes_per_sample = 1;
    n = planes * g.plane;
    DINV_REQUIRE(n * nd * nd < ((int64_t)1 << 31), "tgv: tensor too large (n * nd^2 must stay below 2^31)");
    return 0;
}


}  // namespace

extern "C" int32_t dinv_tgv_cp_partials(int64_t n) { return (int32_t)grid_for(n); }

extern "C" int dinv_tgv_cp_iter(int32_t nd, int32_t batch, int32_t channels, int32_t D, int32_t H, int32_t W, float* xa, float* xb,
                                float* ra, float* rb, float* ua, float* ub, const float* y, const float* lam1, const float* lam2,
                                float tau, float sigma, float rho, float crit, float* z, float* w, float* partial, int32_t* state,
                                dinv_stream_t stream) {
    Geo g;
    int64_t n;
    DINV_REQUIRE(batch > 0 && channels > 0, "tgv: bad batch / channels");
    if (int rc = make_geo(nd, (int64_t)batch * channels, D, H, W, g, n)) return rc;
    DINV_REQUIRE(xa && xb && ra && rb && ua && ub && y && lam1 && lam2 && z && w && partial && state, "tgv: null operand");
    DINV_REQUIRE(xa != xb && ra != rb && ua != ub && (const float*)xa != y && (const float*)xb != y,
                 "tgv: ping-pong buffers must be distinct");
    DINV_REQUIRE(nd == 3 || (aligned16(ua) && aligned16(ub) && aligned16(ra) && aligned16(rb) && aligned16(w)),
                 "tgv: 2-D u2 / r2 / w buffers must be 16-byte aligned");
    g.planes_per_sample = channels;
    const unsigned nblk = grid_for(n);
    const float opt = (float)(1.0 + (double)tau);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int32_t* cst = state;
    if (nd == 2) {
        hipLaunchKernelGGL(tgv_cp_primal_kernel<2>, dim3(nblk), dim3(kThreads), 0, s, g, n, xa, xb, ra, rb, (const float*)ua,
                           (const float*)ub, y, lam1, tau, opt, rho, z, w, partial, cst);
        hipLaunchKernelGGL(tgv_cp_dual_kernel<2>, dim3(nblk), dim3(kThreads), 0, s, g, n, ua, ub, (const float*)z, (const float*)w,
                           lam2, sigma, rho, cst);
    } else {
        hipLaunchKernelGGL(tgv_cp_primal_kernel<3>, dim3(nblk), dim3(kThreads), 0, s, g, n, xa, xb, ra, rb, (const float*)ua,
                           (const float*)ub, y, lam1, tau, opt, rho, z, w, partial, cst);
        hipLaunchKernelGGL(tgv_cp_dual_kernel<3>, dim3(nblk), dim3(kThreads), 0, s, g, n, ua, ub, (const float*)z, (const float*)w,
                           lam2, sigma, rho, cst);
    }
    hipLaunchKernelGGL(tgv_cp_check_kernel, dim3(1), dim3(kThreads), 0, s, (int)nblk, (const float*)partial, crit, state);
    DINV_CHECK_LAUNCH();
    return 0;
}

extern "C" int dinv_tgv_epsilon(int32_t nd, int64_t planes, int32_t D, int32_t H, int32_t W, const float* v, float* out,
                                dinv_stream_t stream) {
    Geo g;
    int64_t n;
    if (int rc = make_geo(nd, planes, D, H, W, g, n)) return rc;
    DINV_REQUIRE(v && out && (const float*)out != v, "tgv: bad operands");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (nd == 2) hipLaunchKernelGGL(tgv_epsilon_kernel<2>, dim3(grid_for(n)), dim3(kThreads), 0, s, g, n, v, out);
    else hipLaunchKernelGGL(tgv_epsilon_kernel<3>, dim3(grid_for(n)), dim3(kThreads), 0, s, g, n, v, out);
    DINV_CHECK_LAUNCH();
    return 0;
}

extern "C" int dinv_tgv_epsilon_adjoint(int32_t nd, int64_t planes, int32_t D, int32_t H, int32_t W, const float* u, float* out,
                                        dinv_stream_t stream) {
    Geo g;
    int64_t n;
    if (int rc = make_geo(nd, planes, D, H, W, g, n)) return rc;
    DINV_REQUIRE(u && out && (const float*)out != u, "tgv: bad operands");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (nd == 2) hipLaunchKernelGGL(tgv_epsilon_adjoint_kernel<2>, dim3(grid_for(n)), dim3(kThreads), 0, s, g, n, u, out);
    else hipLaunchKernelGGL(tgv_epsilon_adjoint_kernel<3>, dim3(grid_for(n)), dim3(kThreads), 0, s, g, n, u, out);
    DINV_CHECK_LAUNCH();
    return 0;
}
