// The whole of A = prod_i (F D_i) [F] with F the orthonormal 2-D DFT and D_i complex diagonals as one launch (gfx950): the
// structured operator of phase retrieval, y = |Bx|^2.
//
// Replaces the ATen launches behind
//   StructuredRandomPhaseRetrieval.A / B / B_adjoint / B_dagger / A_vjp   deepinv/physics/phase_retrieval.py:183-296 over
//                          structured_random.py:172-202 (F.pad, then per layer a complex multiply and an fft2, then a slicing
//                          view, then abs and square or a multiply)
//   AmplitudeLoss.grad and spectral_methods on that operator (distance.py:353-369, optim/phase_retrieval.py:174-177)
//
// cstructured_plane_kernel: a workgroup owns one whole working plane (H x W, the larger of the two sides).  The plane is loaded
// once - the centred pad is an index map on the load, the first diagonal is applied on the way - and every layer runs with the
// plane in LDS: the row transform on H lines of length W (tile_fft of csrc/fft_core.hpp with the plan of W), a transposing
// scatter into the other buffer, the column transform on W lines of length H (the plan of H), and on the way back to the row
// layout the scale and the next diagonal.  It is stored once, with the trim as an index map and the epilogue on the store.
// The adjoint runs the inverse transforms with the conjugated diagonals in reverse order.  HBM traffic: x once, the diagonals
// once, the output once.  No atomics, fixed order: bit-reproducible.
//
// LDS: the tables of both plans and two buffers of max(H LS(W), W LS(H)) complex values, LS the odd line stride of fft_core.hpp.
// A plane fits when that is within kMaxLdsBytes (dinv_cstructured_fits).
#include "fft_core.hpp"

#include <cmath>

using namespace dinv;

namespace {

constexpr int kThreads = 512;

struct CStructArgs {
    const float2* x;
    float* out;            // complex [planes, H_out, W_out] as pairs, or real for DINV_CDENSE_ABS2
    const float2* diag;    // [layers, diag_planes, H, W]
    const float* aux;      // w or y, real, of the output's shape
    int64_t diag_planes;
    int h_in, w_in, h_out, w_out, H, W;
    int top_in, left_in, top_out, left_out;   // work (h, w) is input (h - top_in, w - left_in) and output (h - top_out, w - left_out)
    int layers, half, adjoint, epilogue;
    int buf_elems;
    float eps;
    float scale, scale_lo; // 1 / sqrt(H W) as an unevaluated sum of two floats, as in dst.hip: the rounding of the constant would be
                           // a bias common to every output, which an iteration over the operator accumulates coherently
};

size_t buf_elems(int H, int W) {
    const size_t a = (size_t)H * fft_line_stride(W), b = (size_t)W * fft_line_stride(H);
    return a > b ? a : b;
}

size_t lds_bytes(int H, int W) { return fft_table_lds_bytes(W) + fft_table_lds_bytes(H) + 2 * buf_elems(H, W) * sizeof(float2); }

// diagonal applied before / after 2-D transform t of T = layers + half (-1: none).  A: [F] then (D_i, F) for i = 0 .. L - 1;
// A_adjoint: (F^-1, conj D_{L-1-i}) for i = 0 .. L - 1, then [F^-1]
__device__ __forceinline__ int diag_before(const CStructArgs& a, int t) { return a.adjoint ? -1 : (t >= a.half ? t - a.half : -1); }
__device__ __forceinline__ int diag_after(const CStructArgs& a, int t) { return a.adjoint ? (t < a.layers ? a.layers - 1 - t : -1) : -1; }

__device__ __forceinline__ float2 apply_diag(const CStructArgs& a, float2 v, float2 d) { return a.adjoint ? cmulc(v, d) : cmul(v, d); }

template <bool INV>
__device__ __forceinline__ void run_layers(const CStructArgs& a, const dinv_fft_plan& pw, const dinv_fft_plan& ph, float2* cur, float2* oth,
                                           const float2* tww, const int* permw, const float2* twh, const int* permh,
                                           const float2* dplane, int64_t dstride, int64_t plane, int tid) {
    const int H = a.H, W = a.W, LSW = fft_line_stride(W), LSH = fft_line_stride(H);
    const int T = a.layers + a.half, total = H * W;
    for (int t = 0; t < T; ++t) {
        // rows: H lines of length W
        float2* res = tile_fft<INV>(pw, cur, oth, tww, H, LSW, tid, kThreads);
        float2* spare = res == cur ? oth : cur;
        for (int e = tid; e < total; e += kThreads) {
            const int h = e / W, w = e - h * W;
            spare[w * LSH + permh[h]] = res[h * LSW + w];
        }
        // columns: W lines of length H
        float2* col = tile_fft<INV>(ph, spare, res, twh, W, LSH, tid, kThreads);
        float2* next = col == spare ? res : spare;
        const int da = diag_after(a, t), db = t + 1 < T ? diag_before(a, t + 1) : -1;
        const float2* dga = da >= 0 ? dplane + da * dstride : nullptr;
        const float2* dgb = db >= 0 ? dplane + db * dstride : nullptr;
        const bool last = t + 1 == T;
        for (int e = tid; e < total; e += kThreads) {
            const int h = e / W, w = e - h * W;
            const float2 z = col[w * LSH + h];
            float2 v = make_float2(fmaf(z.x, a.scale, z.x * a.scale_lo), fmaf(z.y, a.scale, z.y * a.scale_lo));
            if (dga) v = apply_diag(a, v, dga[e]);
            if (dgb) v = apply_diag(a, v, dgb[e]);
            if (!last) {
                next[h * LSW + permw[w]] = v;
                continue;
            }
            const int ho = h - a.top_out, wo = w - a.left_out;
            if (ho < 0 || ho >= a.h_out || wo < 0 || wo >= a.w_out) continue;
            const int64_t o = (plane * a.h_out + ho) * a.w_out + wo;
            if (a.epilogue == DINV_CDENSE_ABS2) {
                a.out[o] = v.x * v.x + v.y * v.y;
                continue;
            }
            float f = 1.f;
            if (a.epilogue == DINV_CDENSE_WEIGHT) f = a.aux[o];
            if (a.epilogue == DINV_CDENSE_AMPLITUDE) f = 1.f - sqrtf(a.aux[o] / ((v.x * v.x + v.y * v.y) + a.eps));
            reinterpret_cast<float2*>(a.out)[o] = a.epilogue == DINV_CDENSE_NONE ? v : make_float2(v.x * f, v.y * f);
        }
        oth = col;          // the next transform may ping-pong into the buffer the result was read from
        cur = next;
    }
}

__global__ __launch_bounds__(kThreads) void cstructured_plane_kernel(CStructArgs a, dinv_fft_plan pw, dinv_fft_plan ph, const void* table_w,
                                                                     const void* table_h) {
    DINV_DYN_LDS(unsigned char, smem);
    const int H = a.H, W = a.W, LSW = fft_line_stride(W);
    const int tid = threadIdx.x;
    // [tables of W][tables of H][cur][oth]
    const LdsCarve Tw = carve_lds(smem, W, 0, 0, false);
    const LdsCarve Th = carve_lds(reinterpret_cast<unsigned char*>(Tw.buf), H, 0, 0, false);
    float2* tww = Tw.tw;
    int* permw = Tw.perm;
    float2* twh = Th.tw;
    int* permh = Th.perm;
    float2* cur = Th.buf;
    float2* oth = cur + a.buf_elems;
    load_tables(tww, permw, table_w, W, tid, kThreads);
    load_tables(twh, permh, table_h, H, tid, kThreads);
    __syncthreads();
    const int64_t plane = blockIdx.x;
    const int64_t dstride = a.diag_planes * H * W;
    const float2* dplane = a.diag ? a.diag + (plane % a.diag_planes) * H * W : nullptr;
    // load: pad as an index map, the first diagonal on the way, into the row layout
    {
        const int d0 = diag_before(a, 0);
        const float2* dg = d0 >= 0 ? dplane + d0 * dstride : nullptr;
        const float2* xp = a.x + plane * a.h_in * a.w_in;
        for (int e = tid; e < H * W; e += kThreads) {
            const int h = e / W, w = e - h * W;
            const int hi = h - a.top_in, wi = w - a.left_in;
            float2 v = make_float2(0.f, 0.f);
            if (hi >= 0 && hi < a.h_in && wi >= 0 && wi < a.w_in) {
                v = xp[hi * a.w_in + wi];
                if (dg) v = apply_diag(a, v, dg[e]);
            }
            cur[h * LSW + permw[w]] = v;
        }
    }
    if (a.adjoint) run_layers<true>(a, pw, ph, cur, oth, tww, permw, twh, permh, dplane, dstride, plane, tid);
    else run_layers<false>(a, pw, ph, cur, oth, tww, permw, twh, permh, dplane, dstride, plane, tid);
}

}  // namespace

extern "C" int dinv_cstructured_fits(int32_t H_work, int32_t W_work) {
    return H_work >= 1 && W_work >= 1 && (int64_t)H_work * W_work < (1 << 24) && lds_bytes(H_work, W_work) <= kMaxLdsBytes;
}

extern "C" int dinv_cstructured_apply(const float* x, float* out, const float* diag, const float* aux, int64_t planes, int32_t H_in,
                                      int32_t W_in, int32_t H_out, int32_t W_out, int32_t H_work, int32_t W_work, int32_t top,
                                      int32_t left, int64_t diag_planes, int32_t layers, int32_t half, int32_t adjoint, int32_t epilogue,
                                      float eps, const dinv_fft_plan* plan_w, const void* table_w, const dinv_fft_plan* plan_h,
                                      const void* table_h, dinv_stream_t stream) {
    DINV_REQUIRE(planes >= 0 && planes < ((int64_t)1 << 31), "cstructured: bad plane count");
    DINV_REQUIRE(epilogue >= DINV_CDENSE_NONE && epilogue <= DINV_CDENSE_AMPLITUDE, "cstructured: unknown epilogue %d", epilogue);
    if (planes == 0) return 0;
    DINV_REQUIRE(x && out && (const void*)x != (const void*)out, "cstructured: x and out must be non-null and distinct");
    DINV_REQUIRE(layers >= 0 && (half == 0 || half == 1) && layers + half >= 1, "cstructured: needs at least one transform "
                 "(layers = %d, half = %d)", layers, half);
    DINV_REQUIRE(layers == 0 || (diag && diag_planes >= 1), "cstructured: %d layers without diagonals", layers);
    const bool needs_aux = epilogue == DINV_CDENSE_WEIGHT || epilogue == DINV_CDENSE_AMPLITUDE;
    DINV_REQUIRE(!needs_aux || (aux && aux != out), "cstructured: epilogue %d needs a real array of the output's shape that is not the "
                 "output", epilogue);
    DINV_REQUIRE(H_in >= 1 && W_in >= 1 && H_out >= 1 && W_out >= 1, "cstructured: empty side");
    DINV_REQUIRE(H_work == (H_in > H_out ? H_in : H_out) && W_work == (W_in > W_out ? W_in : W_out),
                 "cstructured: the working size must be the larger of the two sides (got %d x %d for %d x %d -> %d x %d)", H_work,
                 W_work, H_in, W_in, H_out, W_out);
    const int h_small = H_in < H_out ? H_in : H_out, w_small = W_in < W_out ? W_in : W_out;
    DINV_REQUIRE(top >= 0 && left >= 0 && top + h_small <= H_work && left + w_small <= W_work,
                 "cstructured: offsets (%d, %d) put the small side outside the working one", top, left);
    DINV_REQUIRE(dinv_cstructured_fits(H_work, W_work), "cstructured: a working plane of %d x %d needs %zu bytes of LDS for its two "
                 "buffers and tables, a workgroup has %zu (dinv_cstructured_fits)", H_work, W_work, lds_bytes(H_work, W_work), kMaxLdsBytes);
    DINV_REQUIRE(plan_w && table_w && plan_h && table_h, "cstructured: null plan / table");
    DINV_REQUIRE(plan_w->n == W_work && plan_h->n == H_work, "cstructured: the plans are for lengths %d and %d, the working plane is "
                 "%d x %d", plan_h->n, plan_w->n, H_work, W_work);
    CStructArgs a{};
    a.x = (const float2*)x; a.out = out; a.diag = layers ? (const float2*)diag : nullptr; a.aux = needs_aux ? aux : nullptr;
    a.diag_planes = layers ? diag_planes : 1;
    a.h_in = H_in; a.w_in = W_in; a.h_out = H_out; a.w_out = W_out; a.H = H_work; a.W = W_work;
    a.top_in = H_in < H_work ? top : 0;
    a.left_in = W_in < W_work ? left : 0;
    a.top_out = H_out < H_work ? top : 0;
    a.left_out = W_out < W_work ? left : 0;
    a.layers = layers; a.half = half; a.adjoint = adjoint ? 1 : 0; a.epilogue = epilogue; a.eps = eps;
    a.buf_elems = (int)buf_elems(H_work, W_work);
    const double sc = 1.0 / std::sqrt((double)H_work * (double)W_work);
    a.scale = (float)sc;
    a.scale_lo = (float)(sc - (double)a.scale);
    const size_t lds = lds_bytes(H_work, W_work);
    if (lds > kDefaultLdsBytes)
        if (int e = raise_lds_cap<cstructured_plane_kernel>(kMaxLdsBytes)) return e;
    hipLaunchKernelGGL(cstructured_plane_kernel, dim3((unsigned)planes), dim3(kThreads), lds, (hipStream_t)stream, a, *plan_w, *plan_h,
                       table_w, table_h);
    DINV_CHECK_LAUNCH();
    return 0;
}
