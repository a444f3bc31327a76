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
//
// ptycho_kernel: the operator of Ptychography, B = [F diag(p_l)]_l with L probe planes p_l (phase_retrieval.py:317-395), on the
// same plane-in-LDS scheme.  Forward fans image plane b out to L output planes (one workgroup each, the probe on the load, the
// epilogue on the store).  Adjoint and normal (x -> sum_l conj(p_l) F^-1 f(F p_l x, aux_l), the amplitude-loss gradient and the
// spectral iteration) give a workgroup image b and a group of G consecutive positions: it runs them one after another, the
// epilogue f between the two transforms in LDS, and sums conj(p_l) times the result in registers, H W / 512 complex values a
// thread.  One group: the workgroup stores the image.  Several: each stores a partial plane and ptycho_reduce_kernel adds them in
// group order.  No atomics, fixed order: bit-reproducible for a given G.
//
// The layer schedule, the two-float scale and the pad / trim validation are those of structured_common.hpp (with dst.hip); the host
// check of the epilogue is that of common.hpp (with cdense.hip).  The device epilogue is this file's own: fp32 on a finished fp32
// value, where cdense.hip evaluates in double on an exact sum.
#include "structured_common.hpp"

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
    LayerSchedule sched;   // the adjoint runs the inverse transforms with the conjugated diagonals
    int epilogue;
    int buf_elems;
    float eps;
    TwoFloat scale;        // 1 / sqrt(H W)
};

size_t buf_elems(int H, int W) {
    const size_t a = (size_t)H * fft_line_stride(W), b = (size_t)W * fft_line_stride(H);
    return a > b ? a : b;
}

size_t lds_bytes(int H, int W) { return fft_table_lds_bytes(W) + fft_table_lds_bytes(H) + 2 * buf_elems(H, W) * sizeof(float2); }

// the tables of both plans and the two plane buffers: [tables of W][tables of H][cur][oth]
struct PlaneLds {
    float2 *tww, *twh, *cur, *oth;
    int *permw, *permh;
};

__device__ __forceinline__ PlaneLds carve_plane(unsigned char* smem, int H, int W, int buf_elems, const void* table_w, const void* table_h,
                                                int tid) {
    const LdsCarve Tw = carve_lds(smem, W, 0, 0, false);
    const LdsCarve Th = carve_lds(reinterpret_cast<unsigned char*>(Tw.buf), H, 0, 0, false);
    PlaneLds p;
    p.tww = Tw.tw; p.permw = Tw.perm; p.twh = Th.tw; p.permh = Th.perm;
    p.cur = Th.buf;
    p.oth = p.cur + buf_elems;
    load_tables(p.tww, p.permw, table_w, W, tid, kThreads);
    load_tables(p.twh, p.permh, table_h, H, tid, kThreads);
    __syncthreads();
    return p;
}

// One 2-D transform of the plane in `cur` (row layout, cur[h LS(W) + perm_w(w)]): the row transform on H lines of length W, a
// transposing scatter, the column transform on W lines of length H.  Returns the buffer that holds the unscaled result in the
// column layout, col[w LS(H) + h]; `other` is the one that may be written while it is read.
template <bool INV>
__device__ __forceinline__ float2* plane_fft2(const dinv_fft_plan& pw, const dinv_fft_plan& ph, float2* cur, float2* oth, const float2* tww,
                                              const float2* twh, const int* permh, int H, int W, int tid, float2*& other) {
    const int LSW = fft_line_stride(W), LSH = fft_line_stride(H), total = H * W;
    float2* res = tile_fft<INV>(pw, cur, oth, tww, H, LSW, tid, kThreads);
    float2* spare = res == cur ? oth : cur;
    for (int e = tid; e < total; e += kThreads) {
        const int h = e / W, w = e - h * W;
        spare[w * LSH + permh[h]] = res[h * LSW + w];
    }
    float2* col = tile_fft<INV>(ph, spare, res, twh, W, LSH, tid, kThreads);
    other = col == spare ? res : spare;
    return col;
}

// the real factor of DINV_CDENSE_WEIGHT / AMPLITUDE on the finished value v; `aux` is read for these two only
__device__ __forceinline__ float epilogue_factor(int epilogue, float2 v, const float* aux, int64_t o, float eps) {
    float f = 1.f;
    if (epilogue == DINV_CDENSE_WEIGHT) f = aux[o];
    if (epilogue == DINV_CDENSE_AMPLITUDE) f = 1.f - sqrtf(aux[o] / ((v.x * v.x + v.y * v.y) + eps));
    return f;
}

// the store of every epilogue: `out` is real for DINV_CDENSE_ABS2, complex pairs otherwise
__device__ __forceinline__ void store_epilogue(int epilogue, float2 v, float* out, const float* aux, int64_t o, float eps) {
    if (epilogue == DINV_CDENSE_ABS2) {
        out[o] = v.x * v.x + v.y * v.y;
        return;
    }
    const float f = epilogue_factor(epilogue, v, aux, o, eps);
    reinterpret_cast<float2*>(out)[o] = epilogue == DINV_CDENSE_NONE ? v : make_float2(v.x * f, v.y * f);
}

__device__ __forceinline__ float2 apply_diag(const CStructArgs& a, float2 v, float2 d) { return a.sched.adjoint ? cmulc(v, d) : cmul(v, d); }

template <bool INV>
__device__ __forceinline__ void run_layers(const CStructArgs& a, const dinv_fft_plan& pw, const dinv_fft_plan& ph, float2* cur, float2* oth,
                                           const float2* tww, const int* permw, const float2* twh, const int* permh,
                                           const float2* dplane, int64_t dstride, int64_t plane, int tid) {
    const int H = a.H, W = a.W, LSW = fft_line_stride(W), LSH = fft_line_stride(H);
    const int T = a.sched.layers + a.sched.half, total = H * W;
    for (int t = 0; t < T; ++t) {
        float2* next;
        float2* col = plane_fft2<INV>(pw, ph, cur, oth, tww, twh, permh, H, W, tid, next);
        const int da = a.sched.diag_after(t), db = t + 1 < T ? a.sched.diag_before(t + 1) : -1;
        const float2* dga = da >= 0 ? dplane + da * dstride : nullptr;
        const float2* dgb = db >= 0 ? dplane + db * dstride : nullptr;
        const bool last = t + 1 == T;
        for (int e = tid; e < total; e += kThreads) {
            const int h = e / W, w = e - h * W;
            float2 v = scaled(col[w * LSH + h], a.scale);
            if (dga) v = apply_diag(a, v, dga[e]);
            if (dgb) v = apply_diag(a, v, dgb[e]);
            if (!last) {
                next[h * LSW + permw[w]] = v;
                continue;
            }
            const int ho = h - a.top_out, wo = w - a.left_out;
            if (ho < 0 || ho >= a.h_out || wo < 0 || wo >= a.w_out) continue;
            store_epilogue(a.epilogue, v, a.out, a.aux, (plane * a.h_out + ho) * a.w_out + wo, a.eps);
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
    const PlaneLds s = carve_plane(smem, H, W, a.buf_elems, table_w, table_h, tid);
    float2 *tww = s.tww, *twh = s.twh, *cur = s.cur, *oth = s.oth;
    int *permw = s.permw, *permh = s.permh;
    const int64_t plane = blockIdx.x;
    const int64_t dstride = a.diag_planes * H * W;
    const float2* dplane = a.diag ? a.diag + (plane % a.diag_planes) * H * W : nullptr;
    // load: pad as an index map, the first diagonal on the way, into the row layout
    {
        const int d0 = a.sched.diag_before(0);
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
    if (a.sched.adjoint) run_layers<true>(a, pw, ph, cur, oth, tww, permw, twh, permh, dplane, dstride, plane, tid);
    else run_layers<false>(a, pw, ph, cur, oth, tww, permw, twh, permh, dplane, dstride, plane, tid);
}

// ---------------------------------------------------------------- ptychography
constexpr int kMaxAcc = 20;   // complex values a thread accumulates: kThreads kMaxAcc covers every plane that fits the LDS
constexpr int kSmallAcc = 8;  // the instantiation for planes up to 64 x 64: few enough registers for two workgroups a compute unit

struct PtychoArgs {
    const float2* x;       // forward, normal: [B, H, W]; adjoint: [B, L, H, W]
    float* out;            // forward: [B, L, H, W] (real for DINV_CDENSE_ABS2); adjoint, normal: [B, groups, H, W] complex
    const void* probe;     // [L, H, W], float2 or float
    const float* aux;      // w or y, real, [B, L, H, W]
    int H, W, L, G, groups;
    int probe_complex, epilogue, buf_elems;
    float eps;
    TwoFloat scale;        // 1 / sqrt(H W)
};

template <bool CONJ>
__device__ __forceinline__ float2 mul_probe(const PtychoArgs& a, float2 v, int64_t i) {
    if (!a.probe_complex) return cscale(v, static_cast<const float*>(a.probe)[i]);
    const float2 p = static_cast<const float2*>(a.probe)[i];
    return CONJ ? cmulc(v, p) : cmul(v, p);
}

// Thread tid sums elements tid + i kThreads of the plane, so the sum stays in registers across the positions of a group.  x is
// read again for every position: after the first it comes from L2, and registers are what bounds the workgroups per compute unit
// here.
template <int OP, int ACC>
__global__ __launch_bounds__(kThreads) void ptycho_kernel(PtychoArgs a, dinv_fft_plan pw, dinv_fft_plan ph, const void* table_w,
                                                          const void* table_h) {
    DINV_DYN_LDS(unsigned char, smem);
    const int H = a.H, W = a.W, LSW = fft_line_stride(W), LSH = fft_line_stride(H), total = H * W;
    const int tid = threadIdx.x;
    const PlaneLds s = carve_plane(smem, H, W, a.buf_elems, table_w, table_h, tid);
    int64_t b;
    int l0, l1;
    if (OP == DINV_PTYCHO_FORWARD) {
        b = blockIdx.x / a.L;
        l0 = blockIdx.x % a.L;
        l1 = l0 + 1;
    } else {
        b = blockIdx.x / a.groups;
        l0 = (blockIdx.x % a.groups) * a.G;
        l1 = l0 + a.G < a.L ? l0 + a.G : a.L;
    }
    float2 acc[ACC];
#pragma unroll
    for (int i = 0; i < ACC; ++i) acc[i] = make_float2(0.f, 0.f);
    for (int l = l0; l < l1; ++l) {
        if (l > l0) __syncthreads();     // the last reads of the previous position's result
        const int64_t pl = (int64_t)l * total, ol = (b * a.L + l) * total;
        for (int e = tid; e < total; e += kThreads) {
            const int h = e / W, w = e - h * W;
            s.cur[h * LSW + s.permw[w]] = OP == DINV_PTYCHO_ADJOINT ? a.x[ol + e] : mul_probe<false>(a, a.x[b * total + e], pl + e);
        }
        float2 *col, *next;
        if (OP == DINV_PTYCHO_ADJOINT) col = plane_fft2<true>(pw, ph, s.cur, s.oth, s.tww, s.twh, s.permh, H, W, tid, next);
        else col = plane_fft2<false>(pw, ph, s.cur, s.oth, s.tww, s.twh, s.permh, H, W, tid, next);
        if (OP == DINV_PTYCHO_FORWARD) {
            for (int e = tid; e < total; e += kThreads) {
                const int h = e / W, w = e - h * W;
                store_epilogue(a.epilogue, scaled(col[w * LSH + h], a.scale), a.out, a.aux, ol + e, a.eps);
            }
            return;
        }
        if (OP == DINV_PTYCHO_NORMAL) {
            // f(F p_l x, aux_l) back into the row layout, then the inverse transform of the same plane
            for (int e = tid; e < total; e += kThreads) {
                const int h = e / W, w = e - h * W;
                const float2 v = scaled(col[w * LSH + h], a.scale);
                const float f = epilogue_factor(a.epilogue, v, a.aux, ol + e, a.eps);
                next[h * LSW + s.permw[w]] = make_float2(v.x * f, v.y * f);
            }
            float2* unused;
            col = plane_fft2<true>(pw, ph, next, col, s.tww, s.twh, s.permh, H, W, tid, unused);
        }
#pragma unroll
        for (int i = 0; i < ACC; ++i) {
            const int e = tid + i * kThreads;
            if (e < total) {
                const int h = e / W, w = e - h * W;
                acc[i] = cadd(acc[i], mul_probe<true>(a, scaled(col[w * LSH + h], a.scale), pl + e));
            }
        }
    }
    float2* o = reinterpret_cast<float2*>(a.out) + (int64_t)blockIdx.x * total;     // block (b, group) -> plane b groups + group
#pragma unroll
    for (int i = 0; i < ACC; ++i) {
        const int e = tid + i * kThreads;
        if (e < total) o[e] = acc[i];
    }
}

// out[b] = sum over groups of part[b, g], in group order
__global__ __launch_bounds__(256) void ptycho_reduce_kernel(const float2* part, float2* out, int64_t total, int groups, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t b = i / total, e = i - b * total;
    const float2* p = part + b * groups * total + e;
    float2 sum = p[0];
    for (int g = 1; g < groups; ++g) sum = cadd(sum, p[g * total]);
    out[i] = sum;
}

// Positions per workgroup of the adjoint and the normal operation.  Forced (group > 0): that many, at most L.  Automatic: the
// largest group that still fills the device, batch ceil(L / G) >= the workgroups it holds at once, or G = 1 where L cannot.  A
// compute unit holds two workgroups of the small-plane instantiation when two planes fit its LDS, one otherwise.
int ptycho_group(int64_t batch, int L, int H, int W, int group) {
    if (group > 0) return group < L ? group : L;
    const int per_cu = H * W <= kThreads * kSmallAcc && 2 * lds_bytes(H, W) <= kMaxLdsBytes ? 2 : 1;
    int64_t groups = ceil_div((int64_t)compute_units() * per_cu, batch);
    if (groups > L) groups = L;
    return (int)ceil_div(L, groups);
}

template <int OP, int ACC>
int ptycho_launch_acc(const PtychoArgs& a, int64_t blocks, const dinv_fft_plan* pw, const void* tw, const dinv_fft_plan* ph, const void* th,
                      hipStream_t stream) {
    constexpr auto kern = ptycho_kernel<OP, ACC>;
    const size_t lds = lds_bytes(a.H, a.W);
    if (lds > kDefaultLdsBytes)
        if (int e = raise_lds_cap<kern>(kMaxLdsBytes)) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kThreads), lds, stream, a, *pw, *ph, tw, th);
    DINV_CHECK_LAUNCH();
    return 0;
}

template <int OP>
int ptycho_launch(const PtychoArgs& a, int64_t blocks, const dinv_fft_plan* pw, const void* tw, const dinv_fft_plan* ph, const void* th,
                  hipStream_t stream) {
    // the forward operation sums nothing: one instantiation
    if constexpr (OP != DINV_PTYCHO_FORWARD)
        if (a.H * a.W <= kThreads * kSmallAcc) return ptycho_launch_acc<OP, kSmallAcc>(a, blocks, pw, tw, ph, th, stream);
    return ptycho_launch_acc<OP, kMaxAcc>(a, blocks, pw, tw, ph, th, stream);
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
    if (int e = check_epilogue("cstructured", epilogue)) return e;
    if (planes == 0) return 0;
    DINV_REQUIRE(x && out && (const void*)x != (const void*)out, "cstructured: x and out must be non-null and distinct");
    DINV_REQUIRE(layers >= 0 && (half == 0 || half == 1) && layers + half >= 1, "cstructured: needs at least one transform "
                 "(layers = %d, half = %d)", layers, half);
    DINV_REQUIRE(layers == 0 || (diag && diag_planes >= 1), "cstructured: %d layers without diagonals", layers);
    if (int e = check_aux("cstructured", epilogue, aux, out, "of the output's shape")) return e;
    if (int e = check_pad_trim("cstructured", H_in, W_in, H_out, W_out, H_work, W_work, top, left)) return e;
    DINV_REQUIRE(dinv_cstructured_fits(H_work, W_work), "cstructured: a working plane of %d x %d needs %zu bytes of LDS for its two "
                 "buffers and tables, a workgroup has %zu (dinv_cstructured_fits)", H_work, W_work, lds_bytes(H_work, W_work), kMaxLdsBytes);
    DINV_REQUIRE(plan_w && table_w && plan_h && table_h, "cstructured: null plan / table");
    DINV_REQUIRE(plan_w->n == W_work && plan_h->n == H_work, "cstructured: the plans are for lengths %d and %d, the working plane is "
                 "%d x %d", plan_h->n, plan_w->n, H_work, W_work);
    CStructArgs a{};
    a.x = (const float2*)x; a.out = out; a.diag = layers ? (const float2*)diag : nullptr; a.aux = needs_aux(epilogue) ? aux : nullptr;
    a.diag_planes = layers ? diag_planes : 1;
    a.h_in = H_in; a.w_in = W_in; a.h_out = H_out; a.w_out = W_out; a.H = H_work; a.W = W_work;
    a.top_in = H_in < H_work ? top : 0;
    a.left_in = W_in < W_work ? left : 0;
    a.top_out = H_out < H_work ? top : 0;
    a.left_out = W_out < W_work ? left : 0;
    a.sched = {layers, half, adjoint ? 1 : 0};
    a.epilogue = epilogue; a.eps = eps;
    a.buf_elems = (int)buf_elems(H_work, W_work);
    a.scale = make_two_float(1.0 / std::sqrt((double)H_work * (double)W_work));
    const size_t lds = lds_bytes(H_work, W_work);
    if (lds > kDefaultLdsBytes)
        if (int e = raise_lds_cap<cstructured_plane_kernel>(kMaxLdsBytes)) return e;
    hipLaunchKernelGGL(cstructured_plane_kernel, dim3((unsigned)planes), dim3(kThreads), lds, (hipStream_t)stream, a, *plan_w, *plan_h,
                       table_w, table_h);
    DINV_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t dinv_ptycho_workspace_bytes(int64_t batch, int32_t n_img, int32_t H, int32_t W, int32_t op, int32_t group) {
    if (batch < 1 || n_img < 1 || H < 1 || W < 1 || op == DINV_PTYCHO_FORWARD) return 0;
    const int64_t groups = ceil_div(n_img, ptycho_group(batch, n_img, H, W, group));
    return groups > 1 ? (size_t)batch * groups * H * W * sizeof(float2) : 0;
}

extern "C" int dinv_ptycho_apply(const float* x, float* out, const void* probe, int32_t probe_complex, const float* aux, int64_t batch,
                                 int32_t n_img, int32_t H, int32_t W, int32_t op, int32_t epilogue, float eps, int32_t group,
                                 const dinv_fft_plan* plan_w, const void* table_w, const dinv_fft_plan* plan_h, const void* table_h,
                                 void* workspace, size_t workspace_bytes, dinv_stream_t stream) {
    DINV_REQUIRE(op >= DINV_PTYCHO_FORWARD && op <= DINV_PTYCHO_NORMAL, "ptycho: unknown operation %d", op);
    if (int e = check_epilogue("ptycho", epilogue)) return e;
    DINV_REQUIRE(op != DINV_PTYCHO_ADJOINT || epilogue == DINV_CDENSE_NONE, "ptycho: the adjoint has no epilogue (got %d)", epilogue);
    DINV_REQUIRE(op != DINV_PTYCHO_NORMAL || needs_aux(epilogue), "ptycho: the normal operation applies DINV_CDENSE_WEIGHT or _AMPLITUDE between "
                 "its transforms (got epilogue %d)", epilogue);
    DINV_REQUIRE(n_img >= 1 && H >= 1 && W >= 1, "ptycho: empty shape (n_img = %d, plane %d x %d)", n_img, H, W);
    DINV_REQUIRE(batch >= 0 && batch * n_img < ((int64_t)1 << 31), "ptycho: bad plane count (%lld x %d)", (long long)batch, n_img);
    DINV_REQUIRE(group >= 0, "ptycho: group %d (0 = automatic, > 0 = positions per workgroup, at most n_img)", group);
    if (batch == 0) return 0;
    DINV_REQUIRE(x && out && probe && (const void*)x != (const void*)out, "ptycho: x, out and probe must be non-null, x and out distinct");
    if (int e = check_aux("ptycho", epilogue, aux, out, "[batch, n_img, H, W]")) return e;
    DINV_REQUIRE(dinv_cstructured_fits(H, W), "ptycho: a plane of %d x %d needs %zu bytes of LDS for its two buffers and tables, a "
                 "workgroup has %zu (dinv_cstructured_fits)", H, W, lds_bytes(H, W), kMaxLdsBytes);
    DINV_REQUIRE((int64_t)H * W <= (int64_t)kThreads * kMaxAcc, "ptycho: a plane of %d x %d exceeds the %d values a workgroup sums in "
                 "registers", H, W, kThreads * kMaxAcc);
    DINV_REQUIRE(plan_w && table_w && plan_h && table_h, "ptycho: null plan / table");
    DINV_REQUIRE(plan_w->n == W && plan_h->n == H, "ptycho: the plans are for lengths %d and %d, the plane is %d x %d", plan_h->n,
                 plan_w->n, H, W);
    PtychoArgs a{};
    a.x = (const float2*)x; a.out = out; a.probe = probe; a.aux = needs_aux(epilogue) ? aux : nullptr;
    a.H = H; a.W = W; a.L = n_img; a.G = 1; a.groups = n_img;
    a.probe_complex = probe_complex ? 1 : 0; a.epilogue = epilogue; a.eps = eps;
    a.buf_elems = (int)buf_elems(H, W);
    a.scale = make_two_float(1.0 / std::sqrt((double)H * (double)W));
    hipStream_t st = (hipStream_t)stream;
    if (op == DINV_PTYCHO_FORWARD) return ptycho_launch<DINV_PTYCHO_FORWARD>(a, batch * n_img, plan_w, table_w, plan_h, table_h, st);
    a.G = ptycho_group(batch, n_img, H, W, group);
    a.groups = (int)ceil_div(n_img, a.G);
    if (a.groups > 1) {
        const size_t need = dinv_ptycho_workspace_bytes(batch, n_img, H, W, op, group);
        DINV_REQUIRE(workspace && workspace_bytes >= need && workspace != (void*)x && workspace != (void*)out,
                     "ptycho: %d groups of %d positions need a workspace of %zu bytes that is neither x nor out (got %zu)", a.groups,
                     a.G, need, workspace_bytes);
        a.out = (float*)workspace;
    }
    const int64_t blocks = batch * a.groups;
    if (int e = op == DINV_PTYCHO_ADJOINT ? ptycho_launch<DINV_PTYCHO_ADJOINT>(a, blocks, plan_w, table_w, plan_h, table_h, st)
                                          : ptycho_launch<DINV_PTYCHO_NORMAL>(a, blocks, plan_w, table_w, plan_h, table_h, st))
        return e;
    if (a.groups > 1) {
        const int64_t total = (int64_t)H * W, n = batch * total;
        hipLaunchKernelGGL(ptycho_reduce_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, (const float2*)workspace, (float2*)out,
                           total, a.groups, n);
        DINV_CHECK_LAUNCH();
    }
    return 0;
}
