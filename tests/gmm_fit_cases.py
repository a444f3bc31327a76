"""Shared by tests/test_gmm_fit_kernels_gpu.py (the gfx950 library) and tests/test_emu_gmm_fit_cases.py (the same kernel sources on
the host emulation): one table of cases for the EM kernels of the Gaussian mixture (dinv_gmm_posterior: gmm_score_kernel with the
POSTERIOR epilogue, csrc/patch_gmm.hpp; dinv_gmm_moments: csrc/gmm_moments.hpp), the Python restatement of the launcher's rules
(tiles per side, blocks, accumulators per wave, waves per chunk, the automatic chunk length, workspace bytes, kernel names and
launch counts), the runner that calls the C entry points on guarded buffers (tests/fft_cases.py Guarded) and the checks.

Moments, exact.  x and c are integers in [-4, 4] and beta is drawn from {0, 1, 1/2, 1/4}: every product beta (x - c)_i (x - c)_j is
a multiple of 1/4 of magnitude at most 64, so every partial sum over at most a few hundred rows is a multiple of 1/4 below 2^22
that fp32 holds without rounding in any order; S0, S1, S2 (started from 3, so that `+=` shows) and obj (nll multiples of 1/4) must
equal integer arithmetic bit for bit, a second call into the same accumulators adds the same again, and a signed permutation of the
columns of x and c permutes S1 and S2.  On hardware this is the test of the accumulator-to-row map, of the block index of the upper
triangle and of the mirror.

Moments, rounding, per element.  Rows drawn from a random mixture (gmm_cases.random_model), beta the fp64 posterior rounded to
fp32 (prescribed to the kernel), the truth fp64 arithmetic on those fp32 inputs.  With u = 2^-24, gamma_n = n u / (1 - n u):
  y_i = fl(x_i - c_i) (u), a = fl(beta y_i) (u), y_j = fl(x_j - c_j) (u): every term beta y_i y_j is off by at most gamma_3 relative;
  a chunk of L = chunk_rows rows is a chain of L fused multiply-adds (the padding rows add exact zeros): gamma_L;
  the reduce adds `chunks` partials and the running accumulator in fp64: (chunks + 1) 2^-53.
  a responsibility may be denormal or underflow against its row (K = 200: most are): where a = fl(beta y_i) or a partial sum is
  below 2^-126 the relative bounds do not hold and the error of the operation is at most 2^-150 absolute, for a carried on by
  |y_j|: at most N (1 + max |y|) 2^-149 per entry.
      E_ij = (gamma_{L + 3} + (chunks + 1) 2^-53) sum_n |beta_n y_ni y_nj| + 2^-53 |G_ij| + N (1 + max |y|) 2^-149
Posterior, rounding, per element.  E_nk is the score bound of gmm_cases.score_bounds (weights, r = 0), E_nll that of its
run_rounding.  beta = expf(fl(s - lse)): the argument is off by at most delta = E_nk + E_nll_n + u |s - lse|, expf is within EXP_ULP
ulp and a result below 2^-126 is denormal (2^-149 absolute):
      E_beta = beta (expm1(delta) (1 + 2 EXP_ULP u) + 2 EXP_ULP u) + 2^-149
  On the MI355X the worst ratio of the table, 0.98, is the last term alone: a responsibility of 1.39e-45, just under the smallest
  denormal, comes back as 0 (a whole denormal ulp).  A ratio above 1 there would mean expf lost more than one denormal ulp; the
  relative terms stay below 0.03 of their bound.  Every check prints the element at which beta is tightest.
nll is compared with its fp64 value within E_nll and must be bitwise what dinv_gmm_scores gives with the NLL epilogue, in every
case; K = 1 gives beta == 1 exactly.  Derived, not measured; every check prints the worst error / bound it saw.

Every call is made twice and must give the same bits.  Every buffer is guarded."""
import ctypes
from dataclasses import dataclass

import torch

import gmm_cases as GC
from fft_cases import POISON, Guarded

U = GC.U
ROWS, TARGET_WAVES, MIN_CHUNK, MAX_D = 32, 4096, 128, 1023


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    K: int
    d: int
    N: int
    chunk_rows: int = 0        # 0 = automatic, else forced
    emu: bool = True

    @property
    def id(self):
        return f"k{self.K}-d{self.d}-n{self.N}-" + (f"chunk{self.chunk_rows}" if self.chunk_rows else "auto") + f"-nj{accumulators(self)}"

    @property
    def score_case(self):
        """the rows-mode case of gmm_cases whose launcher rules, truth and score bounds the posterior shares"""
        return GC.Case("rows", self.K, d_rows=self.d, N_rows=self.N, r=None)


# ------------------------------------------------------------------ the launcher's rules, restated
def tiles(c):
    """tiles of 32 per side of [x - c, 1]^T diag(beta) [x - c, 1]"""
    return cdiv(c.d + 1, 32)


def blocks(c):
    return tiles(c) * (tiles(c) + 1) // 2


def accumulators(c):
    """NJ of gmm_moments_kernel<NJ>"""
    return {1: 1, 2: 2}.get(tiles(c), 4)


def waves_per_chunk(c):
    T, nj = tiles(c), accumulators(c)
    return sum(cdiv(T - bi, nj) for bi in range(T))


def chunk_rows(c):
    if c.chunk_rows:
        return c.chunk_rows
    want = cdiv(TARGET_WAVES, c.K * waves_per_chunk(c))
    return cdiv(max(cdiv(c.N, want), min(c.N, MIN_CHUNK)), ROWS) * ROWS


def chunks(c):
    return cdiv(c.N, chunk_rows(c))


def workspace_bytes(c):
    return c.K * chunks(c) * blocks(c) * 4096


def block_index(T, bi, bj):
    return bi * T - bi * (bi - 1) // 2 + (bj - bi)


def posterior_launches(c):
    return [GC.score_kernel(c.score_case)]


def moments_launches(c):
    return [f"(gmm_moments_kernel<{accumulators(c)}>)", "gmm_moments_reduce_kernel"]


CASES = [
    # one tile per side (d + 1 <= 32, NJ = 1): one row; one row short of a forced chunk, exactly one and one past it; d = 31 fills the
    # tile exactly
    Case(3, 1, 1),
    Case(8, 9, 31, chunk_rows=32),
    Case(3, 16, 32, chunk_rows=32),
    Case(3, 31, 33, chunk_rows=32),
    # automatic chunks: 129 rows of one component are chunks of 128 and of 1
    Case(1, 9, 129),
    # two tiles per side (NJ = 2): d = 32 puts the appended one alone in the second tile
    Case(1, 32, 33),
    Case(8, 36, 129, chunk_rows=64),           # three chunks, the last ragged (one row)
    Case(3, 37, 129),
    Case(200, 36, 33),
    # four tiles per side (NJ = 4): tile rows of 4, 3, 2 and 1 blocks, one wave each
    Case(3, 108, 33, chunk_rows=32),
    # seven tiles per side: the tile rows of 7, 6 and 5 blocks are split over two waves
    Case(3, 192, 129, chunk_rows=64),
    # the largest: GPU only
    Case(200, 192, 129, emu=False),
    Case(200, 108, 129, chunk_rows=32, emu=False),
]
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"


# ------------------------------------------------------------------ the runner
def _p(g):
    return ctypes.c_void_p(0 if g is None else g.t.data_ptr())


class Accumulators:
    """guarded fp64 device accumulators S0 [K], S1 [K, d], S2 [K, d, d], obj [1], every entry set to `start`"""

    def __init__(self, r, K, d, start):
        self.K, self.d = K, d
        self.g = [Guarded(2 * n, r.device) for n in (K, K * d, K * d * d, 1)]
        for g in self.g:
            g.t.view(torch.float64).fill_(start)

    def values(self):
        """(S0, S1, S2, obj) on the host"""
        S0, S1, S2, obj = (g.t.view(torch.float64).cpu().clone() for g in self.g)
        return S0, S1.view(self.K, self.d), S2.view(self.K, self.d, self.d), obj

    def intact(self):
        return all(g.guards_intact() for g in self.g)

    def untouched_since(self, start):
        return self.intact() and all(bool((g.t.view(torch.float64) == start).all()) for g in self.g)


def fbuf(r, t):
    """a guarded device copy of t as fp32"""
    return r.buf(t)


def call_posterior(r, c, ops, xb, beta=None, nll=None, N=None, K=None, d=None):
    """one dinv_gmm_posterior call: (rc, beta, nll) guarded"""
    beta = beta or Guarded(max(c.N * c.K, 1), r.device)
    nll = nll or Guarded(max(c.N, 1), r.device)
    Wt, m, lam, lw, _ = ops
    if r.reset:
        r.reset()
    rc = r.lib.dinv_gmm_posterior(_p(xb), c.N if N is None else N, _p(Wt), _p(m), _p(lam), _p(lw), c.K if K is None else K,
                                  c.d if d is None else d, _p(beta), _p(nll), r._stream())
    return rc, beta, nll


def call_moments(r, c, xb, bb, cb, nb, acc, ws=None, ws_bytes=None, ws_off=0, N=None, K=None, d=None, chunk=None):
    """one dinv_gmm_moments call: (rc, the guarded workspace)"""
    N, K, d = (c.N if N is None else N), (c.K if K is None else K), (c.d if d is None else d)
    chunk = c.chunk_rows if chunk is None else chunk
    nbytes = int(r.lib.dinv_gmm_moments_workspace_bytes(N, K, d, chunk))
    ws = ws or Guarded(max(nbytes // 4, 4) + (ws_off + 3) // 4, r.device)
    S0, S1, S2, obj = acc.g if acc is not None else (None,) * 4
    if r.reset:
        r.reset()
    rc = r.lib.dinv_gmm_moments(_p(xb), _p(bb), _p(cb), _p(nb), N, K, d, chunk, _p(S0), _p(S1), _p(S2), _p(obj),
                                ctypes.c_void_p(ws.t.data_ptr() + ws_off), nbytes if ws_bytes is None else ws_bytes, r._stream())
    return rc, ws


def _logged(r, c, want, what):
    if r.launches is not None:
        got = r.launches()
        assert got == want, f"{c.id}: {what} launched {got}, the restated dispatch expects {want}"


def _seed(c):
    return c.K * 7919 + c.d * 131 + c.N * 17 + c.chunk_rows


def run_moments(r, c, x, beta, cen, nll, start=3.0):
    """dinv_gmm_moments on guarded buffers, twice into the same accumulators and once more into fresh ones: returns the sums of one
    call (S0, S1, S2, obj) without `start`; asserts the restated workspace size and launches, the guards, that two identical calls
    give equal bits, and that the second call into the same accumulators adds exactly what the first did where that is exact"""
    assert int(r.lib.dinv_gmm_moments_workspace_bytes(c.N, c.K, c.d, c.chunk_rows)) == workspace_bytes(c), \
        f"{c.id}: workspace of {r.lib.dinv_gmm_moments_workspace_bytes(c.N, c.K, c.d, c.chunk_rows)} bytes, restated {workspace_bytes(c)}"
    xb, bb, cb, nb = (fbuf(r, t) for t in (x, beta, cen, nll))
    before = [g.bits().clone() for g in (xb, bb, cb, nb)]
    acc, acc2 = Accumulators(r, c.K, c.d, start), Accumulators(r, c.K, c.d, start)
    rc, ws = call_moments(r, c, xb, bb, cb, nb, acc)
    assert rc == 0, f"{c.id}: moments: error {rc}: {r.err()}"
    _logged(r, c, moments_launches(c), "moments")
    assert ws.guards_intact() and acc.intact(), f"{c.id}: moments: write outside a buffer"
    assert not bool((ws.bits()[:workspace_bytes(c) // 4] == POISON).any()), f"{c.id}: a workspace entry was never written"
    one = acc.values()
    rc, ws2 = call_moments(r, c, xb, bb, cb, nb, acc2)
    assert rc == 0, r.err()
    two = acc2.values()
    assert all(torch.equal(a, b) for a, b in zip(one, two)) and torch.equal(ws.bits(), ws2.bits()), f"{c.id}: two identical calls differ"
    rc, _ = call_moments(r, c, xb, bb, cb, nb, acc, ws=ws)
    assert rc == 0, r.err()
    twice = acc.values()
    assert acc.intact() and all(g.guards_intact() for g in (xb, bb, cb, nb)), f"{c.id}: moments: write outside a buffer"
    assert all(torch.equal(g.bits(), b) for g, b in zip((xb, bb, cb, nb), before)), f"{c.id}: a call modified an operand"
    return [a - start for a in one], [a - start for a in twice]


def moments_truth(x, beta, cen, weight_abs=False):
    """fp64: G [K, d + 1, d + 1] = sum_n beta_nk y_n y_n^T with y_n = [x_n - c_k, 1]; weight_abs: sum_n |beta y_i y_j|"""
    N, d = x.shape
    y = torch.cat([x[None] - cen[:, None, :], torch.ones(cen.shape[0], N, 1, dtype=torch.float64)], 2)        # [K, N, d + 1]
    if weight_abs:
        y = y.abs()
    return torch.einsum("nk,kni,knj->kij", beta.abs() if weight_abs else beta, y, y)


def split(G):
    d = G.shape[1] - 1
    return G[:, d, d], G[:, :d, d], G[:, :d, :d]


def run_exact_moments(r, c):
    gen = torch.Generator().manual_seed(_seed(c))
    x = torch.randint(-4, 5, (c.N, c.d), generator=gen).double()
    cen = torch.randint(-4, 5, (c.K, c.d), generator=gen).double()
    beta = torch.tensor([0.0, 1.0, 0.5, 0.25], dtype=torch.float64)[torch.randint(0, 4, (c.N, c.K), generator=gen)]
    nll = torch.randint(-40, 41, (c.N,), generator=gen).double() / 4
    want = (*split(moments_truth(x, beta, cen)), nll.sum().reshape(1))
    once, twice = run_moments(r, c, x, beta, cen, nll)
    for name, got, got2, w in zip(("S0", "S1", "S2", "obj"), once, twice, want):
        bad = got != w
        assert not bool(bad.any()), (f"{c.id}: {int(bad.sum())} of {bad.numel()} entries of {name} are wrong, the first at "
                                     f"{tuple(int(v) for v in bad.nonzero()[0])}: {float(got[bad][0])} for {float(w[bad][0])}")
        assert torch.equal(got2, 2 * w), f"{c.id}: a second call into the same accumulators did not add {name} again"
    assert torch.equal(once[2], once[2].transpose(1, 2)), f"{c.id}: S2 is not symmetric"
    # a signed permutation of the columns permutes the result
    perm = torch.randperm(c.d, generator=gen)
    sign = (torch.randint(0, 2, (c.d,), generator=gen) * 2 - 1).double()
    (S0p, S1p, S2p, _), _ = run_moments(r, c, x[:, perm] * sign, beta, cen[:, perm] * sign, nll)
    S0, S1, S2, _ = once
    assert torch.equal(S0p, S0) and torch.equal(S1p, S1[:, perm] * sign), f"{c.id}: S0 / S1 under a signed column permutation"
    assert torch.equal(S2p, S2[:, perm][:, :, perm] * sign[:, None] * sign[None, :]), f"{c.id}: S2 under a signed column permutation"


def mixture_rows(c, model, gen):
    """[N, d] rows drawn from the mixture, rounded to fp32 (as fp64 copies)"""
    Wt, m, lam, logw, _ = model
    K, d = c.K, c.d
    k = torch.multinomial(torch.exp(logw), c.N, replacement=True, generator=gen)
    z = torch.randn(c.N, d, generator=gen, dtype=torch.float64)
    t = m.reshape(K, d)[k] + lam.reshape(K, d)[k].sqrt() * z                     # the row in the eigenbasis of its component
    return torch.einsum("nij,ni->nj", Wt.reshape(K, d, d)[k], t).float().double()


def rounding_inputs(c):
    """(model, x, truth, score bound E [N, K]) of the rounding checks"""
    gen = torch.Generator().manual_seed(_seed(c) + 1)
    sc = c.score_case
    model = GC.random_model(sc, gen)
    x = mixture_rows(c, model, gen)
    tr = GC.truth(sc, model, x)
    E, _ = GC.score_bounds(sc, model, tr)
    return model, x, tr, E


def run_posterior(r, c, model, x, tr, E):
    """dinv_gmm_posterior twice on guarded buffers against fp64 and the NLL epilogue; returns (beta fp32, nll fp32, worst ratios)"""
    sc = c.score_case
    ops = GC._device_model(r, model)
    xb = fbuf(r, x)
    rc, bb, nb = call_posterior(r, c, ops, xb)
    assert rc == 0, f"{c.id}: posterior: error {rc}: {r.err()}"
    _logged(r, c, posterior_launches(c), "posterior")
    beta = GC._written(sc, "beta", bb).view(torch.float32).view(c.N, c.K).clone()
    nll = GC._written(sc, "nll", nb).view(torch.float32).clone()
    rc, bb2, nb2 = call_posterior(r, c, ops, xb)
    assert rc == 0 and torch.equal(bb2.bits(), bb.bits()) and torch.equal(nb2.bits(), nb.bits()), f"{c.id}: two identical posteriors differ"
    rc, out = r.scores(sc, ops, xb, GC.NLL)
    assert rc == 0, r.err()
    assert torch.equal(GC._written(sc, "nll epilogue", out), nb.bits()), f"{c.id}: nll is not bitwise the NLL epilogue's"
    GC._clean(sc, "posterior operands", xb, *[g for g in ops if g is not None])
    if c.K == 1:
        assert bool((beta == 1.0).all()), f"{c.id}: one component, but beta != 1"
    s = tr["scores"]
    M = s.max(1).values
    logS = torch.log(torch.exp(s - M[:, None]).sum(1))
    lse = M + logS
    Enll = (E.max(1).values + GC.gamma(c.K * (2 * GC.EXP_ULP + 3)) + 2 * GC.LOG_ULP * U * logS.abs() + 2 * U * (M.abs() + logS.abs()))
    want = torch.exp(s - lse[:, None])
    delta = E + Enll[:, None] + U * (s - lse[:, None]).abs()
    Eb = want * (torch.expm1(delta) * (1 + 2 * GC.EXP_ULP * U) + 2 * GC.EXP_ULP * U) + 2.0 ** -149
    assert not bool(torch.isnan(beta).any() | torch.isnan(nll).any()), f"{c.id}: NaN"
    rb = (beta.double() - want).abs() / Eb
    worst = {"beta": float(rb.max()), "nll": float(((nll.double() + lse).abs() / Enll).max())}
    at = int(rb.argmax())
    print(f"{c.id}: beta is tightest at a responsibility of {float(want.reshape(-1)[at]):.3g} (kernel {float(beta.reshape(-1)[at]):.3g}), "
          f"whose bound is {float(Eb.reshape(-1)[at]):.3g} with delta {float(delta.reshape(-1)[at]):.3g}")
    return beta, nll, worst


def run_rounding(r, c):
    model, x, tr, E = rounding_inputs(c)
    beta, nll, worst = run_posterior(r, c, model, x, tr, E)
    # the moments of the kernel's own responsibilities about the model's means, as fit calls them
    Wt, m, _, _, _ = model
    cen = torch.einsum("kij,ki->kj", Wt.reshape(c.K, c.d, c.d), m.reshape(c.K, c.d)).float().double()
    b64, n64 = beta.double(), nll.double()
    (S0, S1, S2, obj), _ = run_moments(r, c, x, b64, cen, n64, start=0.0)
    G, Gabs = moments_truth(x, b64, cen), moments_truth(x, b64, cen, weight_abs=True)
    L, nch = chunk_rows(c), chunks(c)
    ymax = float((x[None] - cen[:, None, :]).abs().max())
    Eg = (GC.gamma(L + 3) + (nch + 1) * 2.0 ** -53) * Gabs + 2.0 ** -53 * G.abs() + c.N * (1 + ymax) * 2.0 ** -149
    for name, got, want, bound in zip(("S0", "S1", "S2"), (S0, S1, S2), split(G), split(Eg)):
        ratio = (got - want).abs() / bound.clamp_min(1e-300)
        assert not bool(torch.isnan(got).any()), f"{c.id}: {name}: NaN"
        worst[name] = float(ratio.max())
    # obj: fp64 additions of N fp32 values in a fixed order, against torch's fp64 sum in another: gamma_N of sum |nll| each
    worst["obj"] = float((obj[0] - n64.sum()).abs() / (2 * (c.N + 1) * 2.0 ** -53 * n64.abs().sum()).clamp_min(1e-300))
    assert torch.equal(S2, S2.transpose(1, 2)), f"{c.id}: S2 is not symmetric"
    print(f"{c.id}: worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= 1.0, f"{c.id}: {name}: an element is {v:.3g} times its bound"
    return worst


def run_case(r, c):
    run_exact_moments(r, c)
    return run_rounding(r, c)


# ------------------------------------------------------------------ underflow, large grids, refusals (shared by both test files)
def run_underflow(r):
    """two components 40 apart with unit covariances: the far component's exp underflows and its responsibility is exactly 0"""
    c = Case(2, 4, 33)
    K, d = c.K, c.d
    gen = torch.Generator().manual_seed(3)
    Wt = torch.eye(d, dtype=torch.float64)[None].repeat(K, 1, 1).reshape(K * d, d)
    m = torch.zeros(K, d, dtype=torch.float64)
    m[1] += 40.0
    model = (Wt, m.reshape(-1), torch.ones(K * d, dtype=torch.float64), torch.log(torch.tensor([0.5, 0.5], dtype=torch.float64)), None)
    x = torch.randn(c.N, d, generator=gen).float().double()
    x[::2] += 40.0
    rc, bb, nb = call_posterior(r, c, GC._device_model(r, model), fbuf(r, x))
    assert rc == 0, r.err()
    beta = GC._written(c.score_case, "beta", bb).view(torch.float32).view(c.N, K)
    near = torch.arange(c.N) % 2 == 0
    assert bool((beta[near, 0] == 0).all() and (beta[near, 1] == 1).all() and (beta[~near, 1] == 0).all() and (beta[~near, 0] == 1).all())


def run_patch_tiles(r):
    """the POSTERIOR epilogue with two and four patch tiles per wave (257 workgroups of 256 and of 512 rows): one component, so beta
    is exactly 1, and nll is bitwise the NLL epilogue's.  GPU only: the emulation takes minutes over these rows."""
    for N in (256 * 256 + 1, 256 * 512 + 1):
        c = Case(1, 9, N)
        sc = c.score_case
        assert GC.patch_tiles(sc) == (2 if N < 100000 else 4)
        gen = torch.Generator().manual_seed(N)
        model = GC.random_model(sc, gen)
        ops = GC._device_model(r, model)
        xb = fbuf(r, torch.randn(N, c.d, generator=gen))
        rc, bb, nb = call_posterior(r, c, ops, xb)
        assert rc == 0, r.err()
        assert bool((GC._written(sc, "beta", bb).view(torch.float32) == 1.0).all()), f"{c.id}: beta != 1"
        rc, out = r.scores(sc, ops, xb, GC.NLL)
        assert rc == 0 and torch.equal(GC._written(sc, "nll epilogue", out), GC._written(sc, "nll", nb)), f"{c.id}: nll differs"


def run_refusals(r):
    """every DINV_REQUIRE of the two entry points (csrc/dense.hip, csrc/gmm_moments.hpp, gmm_plan_rows of csrc/patch_gmm.hpp), each
    by words of its own message, and the empty batch launching nothing.  Every refusal returns before a launch."""
    c = Case(3, 9, 40, chunk_rows=32)
    gen = torch.Generator().manual_seed(11)
    model = GC.random_model(c.score_case, gen)
    ops = GC._device_model(r, model)
    xb = fbuf(r, torch.randn(c.N, c.d, generator=gen))
    bb, cb, nb = fbuf(r, torch.rand(c.N, c.K, generator=gen)), fbuf(r, torch.zeros(c.K, c.d)), fbuf(r, torch.zeros(c.N))

    def refused(rc, word, *outs):
        assert rc == 2 and word in r.err(), f"expected a refusal naming '{word}', got {rc}: {r.err()}"
        for o in outs:
            assert o.untouched(), f"refusal '{word}' wrote to an output"

    # the posterior
    for kw, word in ((dict(K=0), "bad model"), (dict(d=0), "bad model"), (dict(K=1 << 29), "rows exceed 2^31"),
                     (dict(N=1 << 31), "2^31"), (dict(N=-1), "2^31"), (dict(K=1 << 20), "K = 1048576 needs")):
        rc, b, n = call_posterior(r, c, ops, xb, **kw); refused(rc, word, b, n)
    rc, b, n = call_posterior(r, c, (None, *ops[1:]), xb); refused(rc, "operands Wt, m and lam must be non-null", b, n)
    rc, b, n = call_posterior(r, c, (*ops[:3], None, None), xb); refused(rc, "log weights must be non-null", b, n)
    rc, b, n = call_posterior(r, c, ops, None); refused(rc, "x, beta and nll must be non-null", b, n)
    before = xb.bits().clone()
    rc, b, n = call_posterior(r, c, ops, xb, beta=xb); refused(rc, "must not alias", n)
    assert torch.equal(xb.bits(), before)
    rc, b, n = call_posterior(r, c, ops, xb, N=(1 << 31) - 1, K=1000); refused(rc, "responsibility matrix", b, n)
    rc, b, n = call_posterior(r, c, ops, xb, N=0)
    assert rc == 0 and b.untouched() and n.untouched()
    _logged(r, c, [], "an empty posterior")

    # the moments
    acc = Accumulators(r, c.K, c.d, 5.0)

    def moments(word, x=xb, b=bb, cen=cb, nll=nb, a=acc, **kw):
        rc, ws = call_moments(r, c, x, b, cen, nll, a, **kw)
        refused(rc, word, ws)
        assert acc.untouched_since(5.0), f"refusal '{word}' wrote to an accumulator"

    moments("K = 0 components", K=0)
    moments("K = 65536 components", K=65536)
    moments("dimension d = 0", d=0)
    moments(f"dimension d = {MAX_D + 1}", d=MAX_D + 1)
    moments("row count must be below 2^31", N=1 << 31)
    moments("row count must be below 2^31", N=-1)
    moments("chunk_rows = 48 is not a multiple", chunk=48)
    moments("chunk_rows = -32 is not a multiple", chunk=-32)
    moments("chunks of 32 rows, at most 65535", N=32 * 65536, chunk=32, ws_bytes=0)
    moments("x, beta and c must be non-null", x=None)
    moments("x, beta and c must be non-null", b=None)
    moments("x, beta and c must be non-null", cen=None)
    rc, ws = call_moments(r, c, xb, bb, cb, nb, None); refused(rc, "accumulators S0, S1 and S2 must be non-null", ws)
    half = Accumulators(r, c.K, c.d, 5.0)
    half.g[3] = None
    rc, ws = call_moments(r, c, xb, bb, cb, nb, half); refused(rc, "obj must be non-null", ws)
    assert all(bool((g.t.view(torch.float64) == 5.0).all()) for g in half.g[:3])
    moments("are needed", ws_bytes=workspace_bytes(c) - 1)
    moments("16-byte aligned", ws_off=4)
    assert int(r.lib.dinv_gmm_moments_workspace_bytes(c.N, c.K, c.d, 48)) == 0, "a refused shape needs no workspace"
    # nll null: obj is left alone and may be null; the sums are still added
    rc, ws = call_moments(r, c, xb, bb, cb, None, half)
    assert rc == 0 and not bool((half.g[0].t.view(torch.float64) == 5.0).any()), r.err()
    # the empty batch launches nothing and leaves the accumulators as they are
    rc, ws = call_moments(r, c, xb, bb, cb, nb, acc, N=0)
    assert rc == 0 and ws.untouched() and acc.untouched_since(5.0)
    _logged(r, c, [], "an empty batch of moments")
