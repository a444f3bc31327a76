// The host side of out[I, R] = in[I, K] op(M) on the fp32 matrix cores, shared by dense.hip (fp32) and cdense.hip (complex64): the
// tile constants, the K-slice rule, the workspace rule, every check of an apply call that does not depend on the scalar type, the
// alignment flags, the grid and the three-way dispatch on the number of accumulator tiles.  A scalar is described by DenseScalar.
// The two __global__ bodies stay in their files: they follow one scheme (a wave owns 32 output columns, one slice of K and up to
// 32 NI input rows; kMaxNI / NI accumulators per tile fed in turn; partial tiles to the workspace [S, I, R], added in index order
// by a reduce kernel), but a body shared through a traits type compiled to slower loads (profiles/README.md).
#pragma once
#include "common.hpp"

namespace dinv {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 32;           // rows of M (output columns) per wave, and input rows per accumulator
constexpr int kMaxNI = 4;           // accumulators per wave: up to 128 input rows stream M once
constexpr int kTargetWaves = 1024;  // 4 per compute unit of an MI355X
constexpr int kMinSliceK = 64;      // the shortest slice of K, unless the scalar allows shorter ones for few rows

struct DenseScalar {
    const char* op;        // "dense" / "cdense": the prefix of every message and the infix of dinv_<op>_workspace_bytes
    int elem_bytes;        // 4 (float) or 8 (float2); a 16-byte load along k is aligned when lengths are multiples of 16 / elem_bytes
    int block_k;           // k's per step of the kernel: a slice is a multiple of it
    bool short_slices;     // a slice may be as short as 2 I k's (at least one block): a slice costs 2 I values of workspace traffic
                           // per output column against the k's it reads of M, and short chains of products keep a small batch
                           // accurate where the slices meet in double
};

// slices of K: enough waves for the chip, none shorter than the scalar's minimum, each a multiple of block_k.  A function of the
// shape only.
inline void split_k(const DenseScalar& sc, int64_t I, int64_t K, int64_t R, int64_t* S, int64_t* kchunk) {
    const int64_t tiles = ceil_div(R, kTile) * ceil_div(I, (int64_t)kTile * kMaxNI);
    int64_t s = kTargetWaves / tiles;
    int64_t min_k = kMinSliceK;
    if (sc.short_slices) {
        const int64_t rows = ceil_div(2 * I, (int64_t)sc.block_k) * sc.block_k;
        if (rows < min_k) min_k = rows;
    }
    const int64_t most = ceil_div(K, min_k);
    if (s > most) s = most;
    if (s < 1) s = 1;
    const int64_t c = ceil_div(ceil_div(K, s), (int64_t)sc.block_k) * sc.block_k;
    *kchunk = c;
    *S = ceil_div(K, c);
}

// every slice of several writes its partial tile: [S, I, R] elements; one slice needs no workspace
inline size_t dense_workspace_bytes(const DenseScalar& sc, int64_t I, int64_t K, int64_t R) {
    if (I < 1 || K < 1 || R < 1) return 0;
    int64_t S, kchunk;
    split_k(sc, I, K, R, &S, &kchunk);
    return S > 1 ? (size_t)S * I * R * sc.elem_bytes : 0;
}

struct DensePlan {
    bool empty;            // no rows: nothing to launch
    int64_t S, kchunk, total;
    int ni;                // accumulator tiles of the partial kernel: 1, 2 or 4
    int vec_in, vec_m;     // 16-byte loads along k are aligned
    dim3 grid, reduce_grid;
};

// the checks of an apply call and everything the launches need
inline int dense_plan(const DenseScalar& sc, const void* in, const void* M, const void* out, int64_t I, int64_t K, int64_t R, int64_t ldm,
                      int32_t transposed, const void* workspace, size_t workspace_bytes, DensePlan* p) {
    const char* op = sc.op;
    DINV_REQUIRE(I >= 0 && K >= 1 && R >= 1, "%s: bad shape I = %lld, K = %lld, R = %lld", op, (long long)I, (long long)K, (long long)R);
    p->empty = I == 0;
    if (p->empty) return 0;
    DINV_REQUIRE(in && M && out && in != out, "%s: operands must be non-null and out must not alias in", op);
    DINV_REQUIRE(ldm >= (transposed ? R : K), "%s: row stride %lld of M is below its row length %lld", op, (long long)ldm,
                 (long long)(transposed ? R : K));
    DINV_REQUIRE(I * R < ((int64_t)1 << 40) && K < ((int64_t)1 << 31) && R < ((int64_t)1 << 31), "%s: shape too large", op);
    split_k(sc, I, K, R, &p->S, &p->kchunk);
    const size_t need = p->S > 1 ? (size_t)p->S * I * R * sc.elem_bytes : 0;
    DINV_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "%s: the workspace holds %zu bytes, %zu are needed "
                 "(dinv_%s_workspace_bytes)", op, workspace_bytes, need, op);
    const int vec = 16 / sc.elem_bytes;
    p->vec_in = aligned16(in) && K % vec == 0;
    p->vec_m = !transposed && aligned16(M) && ldm % vec == 0;
    p->ni = I > 2 * kTile ? 4 : (I > kTile ? 2 : 1);
    const int64_t chunks = p->ni == 4 ? ceil_div(I, (int64_t)kTile * kMaxNI) : 1;
    DINV_REQUIRE(chunks < 65536 && p->S < 65536, "%s: too many row chunks", op);
    p->grid = dim3((unsigned)ceil_div(R, kTile), (unsigned)p->S, (unsigned)chunks);
    p->total = I * R;
    const int64_t blocks = ceil_div(p->total, 256);
    p->reduce_grid = dim3((unsigned)(blocks > 1024 ? 1024 : blocks));
    return 0;
}

// The partial kernel with 4, 2 or 1 accumulator tiles.  A macro, because a launch is known by the spelling of its kernel expression
// (the launch log of the host emulation): `kernel` is the template's name, dense_partial_kernel or cdense_partial_kernel.
#define DINV_DENSE_LAUNCH_PARTIAL(kernel, plan, stream, args)                                          \
    do {                                                                                               \
        if ((plan).ni == 4) hipLaunchKernelGGL(kernel<4>, (plan).grid, dim3(64), 0, stream, args);     \
        else if ((plan).ni == 2) hipLaunchKernelGGL(kernel<2>, (plan).grid, dim3(64), 0, stream, args); \
        else hipLaunchKernelGGL(kernel<1>, (plan).grid, dim3(64), 0, stream, args);                    \
        DINV_CHECK_LAUNCH();                                                                           \
    } while (0)

}  // namespace dinv
