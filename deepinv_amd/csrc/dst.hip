// Orthonormal DST-I of the last axis and the whole of StructuredRandom's A / A_adjoint as one launch (gfx950).
//
// Replaces the ATen launches behind
//   dst1                   deepinv/physics/compressed_sensing.py:9-29 (two zero columns, a flip and a cat build the odd extension
//                          in HBM, rfft of length 2 (n + 1), view_as_real and a strided slice: five passes for one transform)
//   StructuredRandom       deepinv/physics/structured_random.py:172-202 (F.pad, then per layer a broadcast multiply and the five
//                          passes of dst1, then a slicing view)
//
// The reference's value is dst1(x)_k = -sqrt(2 / (n + 1)) sum_j x_j sin(pi (j + 1)(k + 1) / (n + 1)): the imaginary part of the
// ortho rfft of the odd extension e = [0, x, 0, -flip(x)] of length P = 2 (n + 1).  It is symmetric and its own inverse.
//
// Two real rows ride one complex transform.  For odd-extended rows a, b the spectrum of a real odd sequence is purely imaginary, so
//   Z = FFT(e_a + i e_b) = i Im FFT(e_a) - Im FFT(e_b):   dst1(a)_k = Im Z_{k+1} / sqrt(P),   dst1(b)_k = -Re Z_{k+1} / sqrt(P)
// and no untangling pass exists.  The transform is tile_fft of csrc/fft_core.hpp on length P (any length: P = 2050 = 2 5^2 41 for a
// flattened 32 x 32 image takes the generic radix-41 stage).
//
// dst_tile_kernel: a 256-thread workgroup owns a tile of 2 `lines` rows.  The transform mixes along W only, so a row never
// leaves its workgroup: it is loaded once (column pad = an index map on the load, first diagonal applied), every (diagonal,
// transform) layer runs with the row in LDS - between two layers the natural-order result of one buffer is scaled, multiplied
// by the next diagonal and scattered as the permuted odd extension into the other buffer - and it is stored once (column trim on
// the store).  The row pad / trim is a row-index map: only the rows present on both sides are transformed, the padded output
// rows of a forward oversampling call are written as zeros by the same launch and the trimmed ones are never read.
// HBM traffic: x once, the diagonals once, y once.  No atomics, fixed order: bit-reproducible.
// The layer schedule, the two-float scale and the pad / trim validation are those of structured_common.hpp (with cstructured.hip).
#include "structured_common.hpp"

using namespace dinv;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLines = 32;             // complex lines (pairs of rows) per workgroup
constexpr size_t kTileBudget = 32 * 1024; // LDS for the two line buffers while more than one line fits

struct DstArgs {
    const float* x;
    float* out;
    const float* diag;
    int64_t rows;          // rows that are transformed: planes * h_tr
    int64_t zero_total;    // floats of the padded output rows (forward oversampling), written as zeros
    int64_t diag_rows;     // rows of one diagonal: the diagonal row of work row r is r % diag_rows
    int64_t diag_layer;    // floats of one diagonal
    int h_tr, h_in, h_out, h_work;
    int w_in, w_out, n;    // n = W_work, the transform length
    int row_in0, row_out0, row_work0;   // row of transformed row t inside its plane, on each side
    int col_in0, col_out0;              // work column c is input column c - col_in0 and output column c - col_out0
    LayerSchedule sched;   // the transform is its own inverse and the diagonals are real: the adjoint only reverses the order
    int lines;
    TwoFloat scale;        // 1 / sqrt(P)
};

struct RowRef {
    int64_t in, out, diag;  // float offsets of the row's first work column on each side (in / out: may point before the row)
    bool live;
};

__device__ __forceinline__ RowRef row_ref(const DstArgs& a, int64_t g) {
    RowRef r;
    r.live = g < a.rows;
    if (!r.live) g = 0;
    const int64_t p = g / a.h_tr;
    const int t = (int)(g - p * a.h_tr);
    r.in = (p * a.h_in + t + a.row_in0) * a.w_in - a.col_in0;
    r.out = (p * a.h_out + t + a.row_out0) * a.w_out - a.col_out0;
    r.diag = ((p * a.h_work + t + a.row_work0) % a.diag_rows) * a.n;
    return r;
}

// one value of the odd extension pair: both rows of complex line `base` at work column c go to positions c + 1 and P - 1 - c
__device__ __forceinline__ void put_odd(float2* __restrict__ base, const int* __restrict__ perm, int c, int n, float va, float vb) {
    const int P = 2 * (n + 1);
    base[perm[c + 1]] = make_float2(va, vb);
    base[perm[P - 1 - c]] = make_float2(-va, -vb);
    if (c == 0) {
        base[perm[0]] = make_float2(0.f, 0.f);
        base[perm[n + 1]] = make_float2(0.f, 0.f);
    }
}

__global__ __launch_bounds__(kThreads) void dst_tile_kernel(DstArgs a, dinv_fft_plan plan, const void* table) {
    DINV_DYN_LDS(unsigned char, smem);
    const int n = a.n, P = plan.n, LS = fft_line_stride(P);
    const int tid = threadIdx.x;
    LdsCarve L = carve_lds(smem, P, a.lines, LS, true);
    load_tables(L.tw, L.perm, table, P, tid, kThreads);
    // the padded output rows of forward oversampling: zeros, nothing transformed
    if (a.zero_total > 0) {
        const int64_t per_plane = (int64_t)(a.h_out - a.h_tr) * a.w_out;
        for (int64_t z = (int64_t)blockIdx.x * kThreads + tid; z < a.zero_total; z += (int64_t)gridDim.x * kThreads) {
            const int64_t p = z / per_plane, rem = z - p * per_plane;
            const int zr = (int)(rem / a.w_out), c = (int)(rem - (int64_t)zr * a.w_out);
            const int ho = zr < a.row_out0 ? zr : zr + a.h_tr;
            a.out[(p * a.h_out + ho) * a.w_out + c] = 0.f;
        }
    }
    __syncthreads();
    const int64_t g0 = (int64_t)blockIdx.x * 2 * a.lines;
    if (g0 >= a.rows) return;
    const int64_t left = a.rows - g0;
    const int nrows = (int)(left < 2 * a.lines ? left : 2 * a.lines);
    const int nl = (nrows + 1) / 2;
    const int T = a.sched.layers + a.sched.half;

    // a group of tpl threads (the power of two that covers a row, at most the workgroup) walks the columns of one line, so the row
    // references - two 64-bit divisions each - are worked out once per line, not per element
    int tpl = 1;
    while (tpl < n && tpl < kThreads) tpl <<= 1;
    const int lc = tid & (tpl - 1), lg = tid / tpl, G = kThreads / tpl;

    // load: column pad as an index map, the first diagonal on the way
    float2* cur = L.buf;
    float2* oth = L.alt;
    {
        const int d0 = a.sched.diag_before(0);
        const float* dg = d0 >= 0 ? a.diag + (int64_t)d0 * a.diag_layer : nullptr;
        for (int l = lg; l < nl; l += G) {
            const RowRef ra = row_ref(a, g0 + 2 * l), rb = row_ref(a, g0 + 2 * l + 1);
            for (int c = lc; c < n; c += tpl) {
                const int ci = c - a.col_in0;
                const bool cv = ci >= 0 && ci < a.w_in;
                float va = cv ? a.x[ra.in + c] : 0.f;
                float vb = (cv && rb.live) ? a.x[rb.in + c] : 0.f;
                if (dg) {
                    va *= dg[ra.diag + c];
                    if (rb.live) vb *= dg[rb.diag + c];
                }
                put_odd(cur + l * LS, L.perm, c, n, va, vb);
            }
        }
    }
    for (int t = 0; t < T; ++t) {
        float2* res = tile_fft<false>(plan, cur, oth, L.tw, nl, LS, tid, kThreads);
        float2* free_buf = res == cur ? oth : cur;
        const int da = a.sched.diag_after(t), db = t + 1 < T ? a.sched.diag_before(t + 1) : -1;
        const float* dga = da >= 0 ? a.diag + (int64_t)da * a.diag_layer : nullptr;
        const float* dgb = db >= 0 ? a.diag + (int64_t)db * a.diag_layer : nullptr;
        const bool last = t + 1 == T;
        for (int l = lg; l < nl; l += G) {
            const RowRef ra = row_ref(a, g0 + 2 * l), rb = row_ref(a, g0 + 2 * l + 1);
            for (int c = lc; c < n; c += tpl) {
                const float2 z = res[l * LS + c + 1];
                float va = scaled(z.y, a.scale), vb = -scaled(z.x, a.scale);
                if (dga) {
                    va *= dga[ra.diag + c];
                    if (rb.live) vb *= dga[rb.diag + c];
                }
                if (dgb) {
                    va *= dgb[ra.diag + c];
                    if (rb.live) vb *= dgb[rb.diag + c];
                }
                if (!last) {
                    put_odd(free_buf + l * LS, L.perm, c, n, va, vb);
                } else {
                    const int co = c - a.col_out0;
                    if (co >= 0 && co < a.w_out) {
                        a.out[ra.out + c] = va;
                        if (rb.live) a.out[rb.out + c] = vb;
                    }
                }
            }
        }
        oth = res;          // the next transform may ping-pong into the buffer the result was read from
        cur = free_buf;
    }
}

// the tables and both line buffers: the kernel always carves for a generic stage
size_t carve_bytes(int P, int lines) { return fft_lds_bytes(P, lines, true); }

int launch(DstArgs a, const dinv_fft_plan* plan, const void* table, hipStream_t s) {
    DINV_REQUIRE(plan && table, "dst: null plan / table");
    DINV_REQUIRE(a.n >= 1 && a.n <= DINV_DST_MAX_N, "dst: the row length %d is outside 1..%d: the odd extension of length 2 (n + 1) "
                 "with its tables and two line buffers must fit the %zu bytes of LDS of a workgroup", a.n, DINV_DST_MAX_N,
                 kMaxLdsBytes);
    const int P = 2 * (a.n + 1);
    DINV_REQUIRE(plan->n == P, "dst: the plan is for length %d, a row of %d needs 2 (n + 1) = %d", plan->n, a.n, P);
    DINV_REQUIRE(carve_bytes(P, 1) <= kMaxLdsBytes, "dst: the LDS carve for P = %d (%zu bytes) exceeds %zu", P, carve_bytes(P, 1),
                 kMaxLdsBytes);
    // pairs of rows per workgroup: what fits the tile budget, but no more than leaves a workgroup for each of 256 compute units
    int lines = (int)(kTileBudget / ((size_t)2 * fft_line_stride(P) * 8));
    lines = lines < 1 ? 1 : (lines > kMaxLines ? kMaxLines : lines);
    const int64_t pairs = ceil_div(a.rows, 2);
    const int64_t want = ceil_div(pairs, 256);
    if (want < lines) lines = (int)(want < 1 ? 1 : want);
    a.lines = lines;
    a.scale = make_two_float(1.0 / std::sqrt((double)P));
    int64_t blocks = ceil_div(pairs, lines);
    if (blocks < 1) blocks = 1;      // zero rows only
    DINV_REQUIRE(blocks < ((int64_t)1 << 31), "dst: too many rows");
    const size_t lds = carve_bytes(P, lines);
    if (lds > kDefaultLdsBytes)
        if (int e = raise_lds_cap<dst_tile_kernel>(kMaxLdsBytes)) return e;
    hipLaunchKernelGGL(dst_tile_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, s, a, *plan, table);
    DINV_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t dinv_dst_workspace_bytes(int64_t rows, int32_t n) {
    (void)rows; (void)n;
    return 0;   // every layer runs in LDS
}

extern "C" int dinv_dst1(const float* x, float* out, int64_t rows, int32_t n, const dinv_fft_plan* plan, const void* table,
                         dinv_stream_t stream) {
    DINV_REQUIRE(rows >= 0, "dst: bad row count");
    if (rows == 0) return 0;
    DINV_REQUIRE(x && out, "dst: null operand");
    DstArgs a{};
    a.x = x; a.out = out;
    a.rows = rows; a.diag_rows = 1;
    a.h_tr = a.h_in = a.h_out = a.h_work = 1;
    a.w_in = a.w_out = a.n = n;
    a.sched.half = 1;
    return launch(a, plan, table, (hipStream_t)stream);
}

extern "C" int dinv_structured_apply(const float* x, float* out, const float* diag, int64_t planes, int32_t H_in, int32_t W_in,
                                     int32_t H_out, int32_t W_out, int32_t H_work, int32_t W_work, int32_t top, int32_t left,
                                     int64_t diag_rows, int32_t layers, int32_t half, int32_t adjoint, const dinv_fft_plan* plan,
                                     const void* table, dinv_stream_t stream) {
    DINV_REQUIRE(planes >= 0, "structured: bad plane count");
    if (planes == 0) return 0;
    DINV_REQUIRE(x && out && x != out, "structured: x and out must be non-null and distinct");
    DINV_REQUIRE(layers >= 0 && (half == 0 || half == 1) && layers + half >= 1, "structured: needs at least one transform "
                 "(layers = %d, half = %d)", layers, half);
    DINV_REQUIRE(layers == 0 || diag, "structured: %d layers without diagonals", layers);
    if (int e = check_pad_trim("structured", H_in, W_in, H_out, W_out, H_work, W_work, top, left)) return e;
    const int h_tr = H_in < H_out ? H_in : H_out;
    DINV_REQUIRE((H_in == H_work || top + H_in <= H_work) && diag_rows >= 1, "structured: bad geometry");
    DstArgs a{};
    a.x = x; a.out = out; a.diag = diag;
    a.rows = planes * h_tr;
    a.diag_rows = diag_rows;
    a.diag_layer = diag_rows * W_work;
    a.h_tr = h_tr; a.h_in = H_in; a.h_out = H_out; a.h_work = H_work;
    a.w_in = W_in; a.w_out = W_out; a.n = W_work;
    // transformed row t of a plane: row t of the small side, row top + t of the working one
    a.row_in0 = H_in < H_work ? 0 : (H_out < H_work ? top : 0);
    a.row_out0 = H_out < H_work ? 0 : (H_in < H_work ? top : 0);
    a.row_work0 = (H_in < H_work || H_out < H_work) ? top : 0;
    a.col_in0 = W_in < W_work ? left : 0;
    a.col_out0 = W_out < W_work ? left : 0;
    a.zero_total = planes * (int64_t)(H_out - h_tr) * W_out;
    a.sched = {layers, half, adjoint ? 1 : 0};
    return launch(a, plan, table, (hipStream_t)stream);
}
