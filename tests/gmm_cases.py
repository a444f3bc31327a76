"""Shared by tests/test_gmm_kernels_gpu.py (the gfx950 library) and tests/test_emu_gmm_cases.py (the same kernel sources on the
host emulation): one table of cases for the Gaussian-mixture kernels of csrc/patch_gmm.hpp (dinv_gmm_scores, dinv_gmm_epll_step),
the Python restatement of the launcher's rules (patch tiles per wave NP, grid, LDS bytes, kernel names and launch counts), the
runner that calls the C entry points on guarded buffers (tests/fft_cases.py Guarded, NaN poison) and the checks of every case.

Exact.  Q_k are signed permutation matrices, the means in the eigenbasis and the data are small integers, lam + r are powers of two
(several r per batch: lam = 1 and r in {1, 3, 7}), every component has the same eigenvalues and the same weight.  Then every
quadratic form is a small dyadic number that fp32 holds without rounding in any order, the log terms are the same bits for every
component, and k* is prescribed: the first component of the smallest exact quadratic form (two forms differ by at least 2^-3, far
above an ulp of the score).  z = Q diag(lam / (lam + r)) Q^T x, the aggregated x~ = sum / multiplicity (one correctly rounded
division) and a x~ + cb bias with dyadic a, cb must equal the exact result as fp32 numbers; the stored scores must equal
c - q / 2 with q exact and c the log terms in fp64, within the bound of c alone.  On hardware this is the test of the
accumulator-to-row map of v_mfma_f32_32x32x2_f32, of the carry of a component across tiles and of the LDS patch offsets.

Rounding, per element.  Random SPD covariances (QR of randn, eigenvalues logspace(-3, 0) times a factor per component), randn
data, the operands rounded to fp32 once (hip.gmm.eigen_pack); the truth is fp64 arithmetic on those fp32 operands.  With
u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1):
  T_i = sum_j W_ij x_j by d fused multiply-adds:           eT_i = gamma_d sum_j |W_ij| |x_j|
  df_i = fl(T_i - m_i):                                      dd_i = eT_i + u (|df_i| + eT_i)
  w_i = fl(1 / fl(lam_i + r)): one addition (u) and one division (at most DIV_ULP = 2.5 ulp where it is not correctly rounded)
  q = sum_i fl(df_i^2) w_i by fused multiply-adds per half wave, one addition of the halves:
      E_q = sum_i w_i (2 |df_i| dd_i + dd_i^2) (1 + gamma_8) + gamma_{d + 8} q
  c = logw - s / 2 - d log(2 pi) / 2, s = sum_i logf(fl(lam_i + r)): the argument's rounding moves a log by at most u / (1 - u),
      logf is within LOG_ULP ulp, d - 1 additions:
      E_c = (d u (1 + 2u) + (2 LOG_ULP u + gamma_d) sum_i |log_i|) / 2 + 4 u (|logw| + |s| / 2 + d log(2 pi) / 2)
  score = fl(c - q / 2):  E = E_c + E_q / 2 + u |score| (1 + 2u)
  nll = -(M + log S) by an online log-sum-exp: log-sum-exp is 1-Lipschitz in the max norm (max_k E_k); every term of S passes
      at most K rescale-or-add steps, each an expf within EXP_ULP ulp whose rounded argument moves the term by at most u t e^-t
      <= u relative to S >= 1, one multiplication and one addition:  rel S <= gamma_{K (2 EXP_ULP + 3)};  then logf and the sum:
      E_nll = max_k E_k + rel S + 2 LOG_ULP u |log S| + 2 u (|M| + |log S|)
  z:  t_i as above, ratio_i = fl(lam_i / fl(lam_i + r)) within (1 + 2 DIV_ULP) u relative, ts_i = fl(t_i ratio_i):
      dts_i = ratio_i (eT_i + (2 + 2 DIV_ULP) u (|t_i| + eT_i)),   E_z_j = sum_i |W_ij| dts_i + gamma_d sum_i |W_ij| |ts_i|
  x~ = (sum of n <= p^2 entries) / n:  E_x = (sum E_z + gamma_{n - 1} sum |z|) / n + 2 DIV_ULP u |x~|
  out = fma(a, x~, fl(cb bias)):  E_out = |a| E_x + u |cb bias| + u |out|
LOG_ULP = EXP_ULP = 2: the HIP math API reference gives logf and expf of the device library at 1 ulp (as glibc's are below 1 on
the host); the bound allows 2.  Derived, not measured; every check prints the worst error / bound it saw (on the MI355X the worst
of the table is 0.39, on the host emulation 0.09).

Classification.  Where the fp64 gap between the best and the second score exceeds twice the largest score bound of the patch, k*
must be the fp64 argmax; elsewhere it may be any component whose fp64 score is within that of the maximum.  The share of
"elsewhere" patches is asserted to be at most 1 % when a case's data are built, from fp64 alone.  z and x~ are then compared for
the k* the kernel chose.

Every buffer is guarded: operands, outputs and the workspace; outputs must hold no poison afterwards."""
import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from deepinv_amd.hip import gmm as G
from fft_cases import POISON, Guarded

U = 2.0 ** -24
LOG_ULP = EXP_ULP = 2
DIV_ULP = 2.5
WAVES, TARGET_GROUPS, EST_PATCHES, MAX_LDS, DEFAULT_LDS = 4, 256, 4, 160 * 1024, 48 * 1024
SCORES, ARGMAX, NLL = 0, 1, 2


def cdiv(a, b):
    return -(-a // b)


def gamma(n):
    return n * U / (1 - n * U)


# ------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    mode: str                  # "rows": src is [N, d];  "image": src is [B, C, H, W] with patch size p
    K: int
    d_rows: int = 0
    N_rows: int = 0
    C: int = 1
    p: int = 0
    B: int = 1
    H: int = 0
    W: int = 0
    r: tuple = None            # per image (rows: one value), None = the unregularised model
    emu: bool = True

    @property
    def image(self):
        return self.mode == "image"

    @property
    def d(self):
        return self.d_rows or self.C * self.p * self.p        # (image mode with d_rows set: a model of another dimension)

    @property
    def PH(self):
        return self.H - self.p + 1

    @property
    def PW(self):
        return self.W - self.p + 1

    @property
    def N(self):
        return self.B * self.PH * self.PW if self.image else self.N_rows

    @property
    def id(self):
        shape = f"b{self.B}-c{self.C}-p{self.p}-{self.H}x{self.W}" if self.image else f"n{self.N_rows}"
        return f"{self.mode}-np{patch_tiles(self)}-k{self.K}-d{self.d}-{shape}-" + ("r0" if self.r is None else f"r{len(set(self.r))}")


# ------------------------------------------------------------------ the launcher's rules, restated
def groups_at(c, np_):
    if c.image:
        return cdiv(c.PW, 32) * cdiv(c.PH, WAVES * np_) * c.B
    return cdiv(c.N, 32 * WAVES * np_)


def patch_tiles(c):
    """NP of gmm_score_kernel<IMAGE, NP>: the largest of 4, 2 that still leaves TARGET_GROUPS workgroups, else 1"""
    return 4 if groups_at(c, 4) >= TARGET_GROUPS else (2 if groups_at(c, 2) >= TARGET_GROUPS else 1)


def lds_bytes(c):
    np_ = patch_tiles(c)
    words = c.K + (c.d + 1) // 2 * 2
    if c.image:
        words += c.C * (WAVES * np_ + c.p - 1) * (32 + c.p - 1)
    return 4 * words


def score_kernel(c):
    return f"(gmm_score_kernel<{'true' if c.image else 'false'}, {patch_tiles(c)}>)"


def expected_launches(c, step):
    return [score_kernel(c)] + (["gmm_estimate_kernel", "gmm_aggregate_kernel"] if step else [])


def workspace_bytes(c):
    return c.N * (c.d + 1) * 4


R1, R3 = (0.05,), (0.05, 0.2, 0.0125)
CASES = [
    # image mode.  One patch (H = W = p); one row of patches (H = p) with 31 patches and the unregularised model
    Case("image", 3, C=1, p=3, B=1, H=3, W=3, r=R1),
    Case("image", 1, C=1, p=3, B=1, H=3, W=33, r=None),
    # the LDS tile of NP = 1 is 4 x 32 patch origins: one short of it, exactly it and one past it in each direction; d = 16 with
    # K d = 128 a multiple of the row tile; three images with three r
    Case("image", 8, C=1, p=4, B=3, H=6, W=34, r=R3),
    Case("image", 8, C=1, p=4, B=3, H=7, W=35, r=R3),
    Case("image", 8, C=1, p=4, B=1, H=8, W=36, r=R1),
    # colour, d = 27 (odd: the last k of a row is padding; K d = 81 ends inside a tile), non-square
    Case("image", 3, C=3, p=3, B=3, H=5, W=34, r=R3),
    # d = 36: every component straddles row tiles; K d = 288 = 9 tiles
    Case("image", 8, C=1, p=6, B=1, H=9, W=11, r=R1),
    # d = 108: a component spans four tiles
    Case("image", 3, C=3, p=6, B=1, H=8, W=7, r=R1),
    # K = 200 (225 row tiles), one full row of 32 patches
    Case("image", 200, C=1, p=6, B=1, H=6, W=37, r=R1),
    # d = 192 (p = 8, C = 3), the largest the limits name: a component spans six tiles, 96 k steps
    Case("image", 3, C=3, p=8, B=1, H=9, W=10, r=R1),
    # 100 channels: an LDS tile of 66 KB, above the 48 KB a launch gets without the opt-in (raise_lds_cap) and above the 64 KB at
    # which the emulation refuses a launch that forgot it; d = 400
    Case("image", 1, C=100, p=2, B=1, H=3, W=4, r=R1),
    # NP = 2 and NP = 4: 258 workgroups of 8 x 32 and of 16 x 32 patch origins, ragged in both directions
    Case("image", 1, C=1, p=3, B=3, H=346, W=35, r=R3, emu=False),
    Case("image", 1, C=1, p=3, B=3, H=682, W=35, r=R3, emu=False),
    # rows mode: N on both sides of a tile of 32 rows and of a workgroup of 128; d as above
    Case("rows", 3, d_rows=9, N_rows=1, r=R1),
    Case("rows", 8, d_rows=16, N_rows=31, r=None),
    Case("rows", 3, d_rows=27, N_rows=33, r=None),
    Case("rows", 8, d_rows=36, N_rows=129, r=R1),
    Case("rows", 1, d_rows=108, N_rows=33, r=None),
    Case("rows", 200, d_rows=36, N_rows=33, r=R1),
    # K = 17000: 68 KB of dynamic LDS, above the 48 KB a launch gets without the opt-in (raise_lds_cap); the emulation, which
    # refuses a launch above 64 KB that forgot it, takes half a minute over 17000 components and runs the image case above instead
    Case("rows", 17000, d_rows=4, N_rows=33, r=R1, emu=False),
    # NP = 2 and NP = 4 in rows mode: 257 workgroups of 256 and of 512 rows, one row in the last
    Case("rows", 1, d_rows=9, N_rows=256 * 256 + 1, r=None, emu=False),
    Case("rows", 1, d_rows=9, N_rows=256 * 512 + 1, r=None, emu=False),
]
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"


# ------------------------------------------------------------------ models and data
def _seed(c):
    return c.K * 7919 + c.d * 131 + c.N * 17 + c.B


def exact_model(c, gen):
    """(Wt, m, lam, logw, r): signed permutations, integer means in the eigenbasis, lam + r powers of two, equal weights"""
    K, d = c.K, c.d
    Wt = torch.zeros(K, d, d, dtype=torch.float64)
    for k in range(K):
        perm = torch.randperm(d, generator=gen)
        sign = torch.randint(0, 2, (d,), generator=gen) * 2 - 1
        Wt[k, torch.arange(d), perm] = sign.double()
    m = torch.randint(-2, 3, (K, d), generator=gen).double()
    nr = c.B if c.image else 1
    if c.r is None:
        r, lam = None, 2.0 ** torch.randint(-1, 3, (d,), generator=gen).double()
    elif nr == 1:
        r, lam = torch.ones(1, dtype=torch.float64), 2.0 ** torch.randint(1, 4, (d,), generator=gen).double() - 1
    else:
        r, lam = torch.tensor([1.0, 3.0, 7.0][:nr], dtype=torch.float64), torch.ones(d, dtype=torch.float64)
    return Wt.reshape(K * d, d), m.reshape(-1), lam[None].repeat(K, 1).reshape(-1), torch.full((K,), -math.log(K), dtype=torch.float64), r


def random_model(c, gen):
    """random SPD covariances through hip.gmm.eigen_pack, rounded to fp32 once (returned as fp64 copies of the fp32 values)"""
    K, d = c.K, c.d
    Q = torch.linalg.qr(torch.randn(K, d, d, generator=gen, dtype=torch.float64))[0]
    lam = torch.logspace(-3, 0, d, dtype=torch.float64)[None] * (0.5 + torch.rand(K, 1, generator=gen, dtype=torch.float64))
    cov = Q @ torch.diag_embed(lam) @ Q.transpose(1, 2)
    mu = 0.1 * torch.randn(K, d, generator=gen, dtype=torch.float64)
    w = torch.rand(K, generator=gen, dtype=torch.float64) + 0.1
    ops = [t.float().double() for t in G.eigen_pack(cov, mu, w / w.sum())]
    nr = c.B if c.image else 1
    r = None if c.r is None else torch.tensor(c.r[:nr], dtype=torch.float32).double()
    return (*ops, r)


def patches_of(c, src):
    """[N, d] patch matrix (the truth's only: the kernels never build it), entries in the order (c, dy, dx)"""
    if not c.image:
        return src
    cols = torch.nn.functional.unfold(src, c.p)                      # [B, C p p, PH PW]
    return cols.transpose(1, 2).reshape(c.N, c.d)


def image_of_patch(c):
    """[N] the image (the index into r) of every patch"""
    return torch.arange(c.B).repeat_interleave(c.PH * c.PW) if c.image else torch.zeros(c.N, dtype=torch.long)


def truth(c, model, src):
    """fp64: T [N, K, d], df, w [N, K, d], q [N, K], cst [nr, K] with its parts, scores [N, K]"""
    Wt, m, lam, logw, r = model
    K, d = c.K, c.d
    X = patches_of(c, src.double())
    b = image_of_patch(c)
    rr = torch.zeros(1, dtype=torch.float64) if r is None else r
    lr = (lam[None, :].float() + rr[:, None].float()).double().reshape(-1, K, d)       # fl(lam + r), per image
    T = (X @ Wt.t()).reshape(c.N, K, d)
    df = T - m.reshape(1, K, d)
    w = 1.0 / lr[b]
    q = (df * df * w).sum(2)
    logs = torch.log(lr)
    cst = logw[None] - 0.5 * logs.sum(2) - 0.5 * d * G.LOG_2PI
    return dict(X=X, b=b, T=T, df=df, w=w, q=q, lr=lr, logs=logs, cst=cst, scores=cst[b] - 0.5 * q)


def score_bounds(c, model, tr):
    """E [N, K] of the module docstring"""
    Wt, m, lam, logw, r = model
    K, d = c.K, c.d
    eT = gamma(d) * (tr["X"].abs() @ Wt.abs().t()).reshape(c.N, K, d)
    dd = eT + U * (tr["df"].abs() + eT)
    Eq = (tr["w"] * (2 * tr["df"].abs() * dd + dd * dd)).sum(2) * (1 + gamma(8)) + gamma(d + 8) * tr["q"]
    labs = tr["logs"].abs().sum(2)
    s = tr["logs"].sum(2)
    Ec = 0.5 * (d * U * (1 + 2 * U) + (2 * LOG_ULP * U + gamma(d)) * labs) + 4 * U * (logw.abs()[None] + 0.5 * s.abs() + 0.5 * d * G.LOG_2PI)
    return Ec[tr["b"]] + 0.5 * Eq + U * tr["scores"].abs() * (1 + 2 * U), Ec


def ambiguous(tr, E):
    """[N] bool: the fp64 gap between best and second score is within twice the largest score bound of the patch"""
    if tr["scores"].shape[1] == 1:
        return torch.zeros(tr["scores"].shape[0], dtype=torch.bool)
    top = tr["scores"].topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) <= 2 * E.max(1).values


# ------------------------------------------------------------------ the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.gmm), `device` of its buffers,
    `stream()` -> the stream argument and - on the emulation - `reset()` / `launches()`"""

    def __init__(self, lib, device, stream, reset=None, launches=None):
        self.lib, self.device, self._stream = lib, torch.device(device), stream
        self.reset, self.launches = reset, launches

    def err(self):
        return self.lib.dinv_last_error().decode()

    def buf(self, t):
        """a guarded device copy of the fp64 / fp32 tensor t as fp32 (None stays None)"""
        if t is None:
            return None
        g = Guarded(t.numel(), self.device)
        g.t.copy_(t.reshape(-1).float())
        return g

    def _expect(self, c, step):
        if self.launches is not None:
            got, want = self.launches(), expected_launches(c, step)
            assert got == want, f"{c.id}: launched {got}, the restated dispatch expects {want}"

    def scores(self, c, ops, src, epilogue, logw=True, out=None):
        """one dinv_gmm_scores call; returns (rc, the guarded output)"""
        out = out or Guarded(c.N * (c.K if epilogue == SCORES else 1), self.device)
        Wt, m, lam, lw, r = ops
        if self.reset:
            self.reset()
        rc = self.lib.dinv_gmm_scores(_p(src), int(c.image), c.B if c.image else c.N, c.C, c.H, c.W, c.p, _p(Wt), _p(m), _p(lam),
                                      _p(lw if logw else None), c.K, c.d, _p(r), epilogue, _p(out), self._stream())
        return rc, out

    def step(self, c, ops, src, a, cb, bias, ws=None, ws_bytes=None, ws_off=0):
        """one dinv_gmm_epll_step call; returns (rc, the guarded output, the guarded workspace)"""
        nbytes = int(self.lib.dinv_gmm_epll_workspace_bytes(c.B, c.C, c.H, c.W, c.p))
        assert nbytes == workspace_bytes(c), f"{c.id}: workspace of {nbytes} bytes, restated {workspace_bytes(c)}"
        ws = ws or Guarded(nbytes // 4 + (ws_off + 3) // 4, self.device)
        out = Guarded(c.B * c.C * c.H * c.W, self.device)
        Wt, m, lam, lw, r = ops
        if self.reset:
            self.reset()
        rc = self.lib.dinv_gmm_epll_step(_p(src), c.B, c.C, c.H, c.W, c.p, _p(Wt), _p(m), _p(lam), _p(lw), c.K, c.d, _p(r), _p(a),
                                         _p(cb), _p(bias), _p(out), ctypes.c_void_p(ws.t.data_ptr() + ws_off), nbytes if ws_bytes is None else ws_bytes,
                                         self._stream())
        return rc, out, ws


def _p(g):
    return ctypes.c_void_p(0 if g is None else g.t.data_ptr())


def _clean(c, what, *bufs):
    for g in bufs:
        assert g.guards_intact(), f"{c.id}: {what}: write outside a buffer"
    return bufs


def _written(c, what, g):
    bits = g.bits()
    assert g.guards_intact(), f"{c.id}: {what}: write outside the output"
    assert not bool((bits == POISON).any()), (f"{c.id}: {what}: {int((bits == POISON).sum())} outputs hold the guard pattern: never "
                                              "written, or computed from a read outside the operands")
    return bits


def _source(c, gen, integers):
    shape = (c.B, c.C, c.H, c.W) if c.image else (c.N, c.d)
    return torch.randint(-8, 9, shape, generator=gen).double() if integers else torch.randn(shape, generator=gen).float().double()


def _device_model(r, model):
    """guarded device copies of the model, its rows padded per component as the kernels read them (hip.gmm.pad_rows)"""
    Wt, m, lam, logw, rr = model
    K = logw.numel()
    return tuple(r.buf(t) for t in (*G.pad_rows(Wt, m, lam, K, Wt.shape[1]), logw, rr))


def _run_all(r, c, model, src, a, cb, bias):
    """every entry point on guarded buffers: returns the scores [N, K], k* [N], nll [N] and - image mode - (z [N, d], k* of the
    step, out) as CPU tensors; asserts guards, poison, launch logs and the bitwise repeat of the step"""
    ops = _device_model(r, model)
    sb = r.buf(src)
    before = [g.bits().clone() for g in (*ops, sb) if g is not None]
    res = {}
    for name, epi in (("scores", SCORES), ("kstar", ARGMAX), ("nll", NLL)):
        rc, out = r.scores(c, ops, sb, epi)
        assert rc == 0, f"{c.id}: {name}: error {rc}: {r.err()}"
        r._expect(c, False)
        bits = _written(c, name, out)
        res[name] = bits.clone() if epi == ARGMAX else bits.view(torch.float32).clone()
    res["scores"] = res["scores"].view(c.N, c.K)
    rc, out = r.scores(c, ops, sb, SCORES, logw=False)
    assert rc == 0, f"{c.id}: scores without weights: error {rc}: {r.err()}"
    res["scores_now"] = _written(c, "scores without weights", out).view(torch.float32).view(c.N, c.K).clone()
    if c.image and model[4] is not None:
        ab, cbb, bb = r.buf(a), r.buf(cb), r.buf(bias)
        runs = []
        for _ in range(2):
            rc, out, ws = r.step(c, ops, sb, ab, cbb, bb)
            assert rc == 0, f"{c.id}: step: error {rc}: {r.err()}"
            r._expect(c, True)
            runs.append((_written(c, "step", out).clone(), _written(c, "workspace", ws).clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), f"{c.id}: two identical steps differ"
        wsb = runs[0][1]
        res["z"] = wsb[:c.N * c.d].view(torch.float32).view(c.N, c.d)
        res["kstep"] = wsb[c.N * c.d:]
        res["out"] = runs[0][0].view(torch.float32).view(c.B, c.C, c.H, c.W)
        _clean(c, "step", ab, cbb, bb)
    after = [g.bits() for g in (*ops, sb) if g is not None]
    assert all(torch.equal(x, y) for x, y in zip(before, after)), f"{c.id}: a call modified an operand"
    _clean(c, "operands", sb, *[g for g in ops if g is not None])
    return res


def _estimates(c, model, src, kstar, a, cb, bias):
    """fp64: z [N, d] for the given k*, the sum and count per pixel, x~ and out, with the pieces the bounds need"""
    Wt, m, lam, logw, r = model
    K, d = c.K, c.d
    X = patches_of(c, src)
    b = image_of_patch(c)
    Wk = Wt.reshape(K, d, d)[kstar]                                                       # [N, d, d]
    lamk = lam.reshape(K, d)[kstar]
    lr = (lamk.float() + r[b][:, None].float()).double()
    ratio = lamk / lr
    t = torch.einsum("nij,nj->ni", Wk, X)
    ts = t * ratio
    z = torch.einsum("nij,ni->nj", Wk, ts)
    return dict(Wk=Wk, X=X, t=t, ts=ts, ratio=ratio, z=z)


def fold(c, z):
    """[B, C, H, W] sum of the covering patch entries of z [N, d]"""
    cols = z.reshape(c.B, c.PH * c.PW, c.d).transpose(1, 2)
    return torch.nn.functional.fold(cols, (c.H, c.W), c.p)


def run_exact(r, c):
    gen = torch.Generator().manual_seed(_seed(c))
    model = exact_model(c, gen)
    Wt, m, lam, logw, rr = model
    src = _source(c, gen, True)
    a = 2.0 ** -torch.arange(1, c.B + 1).double()
    cb = 2.0 ** -torch.arange(c.B, 0, -1).double()
    bias = torch.randint(-8, 9, src.shape, generator=gen).double() if c.image else None
    tr = truth(c, model, src)
    res = _run_all(r, c, model, src, a, cb, bias)
    want_k = torch.from_numpy(np.argmin(tr["q"].numpy(), axis=1))
    bad = res["kstar"].long() != want_k
    assert not bool(bad.any()), f"{c.id}: {int(bad.sum())} of {c.N} patches are classified wrong, the first is patch {int(bad.nonzero()[0])}"
    # scores: q exact, c within its own bound
    _, Ec = score_bounds(c, model, tr)
    for name, cst in (("scores", tr["cst"]), ("scores_now", tr["cst"] - logw[None])):
        want = cst[tr["b"]] - 0.5 * tr["q"]
        ratio = (res[name].double() - want).abs() / (Ec[tr["b"]] + U * want.abs() * (1 + 2 * U))
        assert float(ratio.max()) <= 1.0, f"{c.id}: {name}: a score is {float(ratio.max()):.3g} times the bound of its log terms"
    if "z" in res:
        assert torch.equal(res["kstep"].long(), want_k), f"{c.id}: the step's k* differ from the prescribed ones"
        est = _estimates(c, model, src, want_k, a, cb, bias)
        wrong = res["z"].double() != est["z"]
        assert not bool(wrong.any()), f"{c.id}: {int(wrong.sum())} of {wrong.numel()} entries of z are wrong, the first at {tuple(int(v) for v in wrong.nonzero()[0])}"
        mult = G.multiplicity(c.H, c.W, c.p).double()
        xt = (fold(c, est["z"]) / mult).float().double()
        want = (a.view(-1, 1, 1, 1) * xt + cb.view(-1, 1, 1, 1) * bias).float().double()
        wrong = res["out"].double() != want
        assert not bool(wrong.any()), f"{c.id}: {int(wrong.sum())} of {wrong.numel()} pixels are wrong, the first at {tuple(int(v) for v in wrong.nonzero()[0])}"


def rounding_inputs(c):
    """(model, src, a, cb, bias, truth, E, ambiguous) of the rounding check; asserts the 1 % cap on ambiguous patches"""
    gen = torch.Generator().manual_seed(_seed(c) + 1)
    model = random_model(c, gen)
    src = _source(c, gen, False)
    a = (0.3 + torch.rand(c.B, generator=gen)).float().double()
    cb = (0.3 + torch.rand(c.B, generator=gen)).float().double()
    bias = torch.randn(src.shape, generator=gen).float().double() if c.image else None
    tr = truth(c, model, src)
    E, _ = score_bounds(c, model, tr)
    amb = ambiguous(tr, E)
    assert float(amb.double().mean()) <= 0.01, f"{c.id}: {int(amb.sum())} of {c.N} patches have an ambiguous class: choose other inputs"
    return model, src, a, cb, bias, tr, E, amb


def step_truth(c, model, src, k, a, cb, bias):
    """fp64 z [N, d] and out [B, C, H, W] of a step for the classes k, each with its bound E_z / E_out of the module docstring"""
    d = c.d
    est = _estimates(c, model, src, k, a, cb, bias)
    Wa = est["Wk"].abs()
    eT = gamma(d) * torch.einsum("nij,nj->ni", Wa, est["X"].abs())
    dts = est["ratio"] * (eT + (2 + 2 * DIV_ULP) * U * (est["t"].abs() + eT))
    Ez = torch.einsum("nij,ni->nj", Wa, dts) + gamma(d) * torch.einsum("nij,ni->nj", Wa, est["ts"].abs())
    mult = G.multiplicity(c.H, c.W, c.p).double()
    xt = fold(c, est["z"]) / mult
    Ex = (fold(c, Ez) + gamma(c.p * c.p - 1) * fold(c, est["z"].abs())) / mult + 2 * DIV_ULP * U * xt.abs()
    av, cv = a.view(-1, 1, 1, 1), cb.view(-1, 1, 1, 1)
    want = av * xt + cv * bias
    return est["z"], Ez, want, av.abs() * Ex + U * (cv * bias).abs() + U * want.abs()


def run_rounding(r, c):
    model, src, a, cb, bias, tr, E, amb = rounding_inputs(c)
    Wt, m, lam, logw, rr = model
    K, d = c.K, c.d
    res = _run_all(r, c, model, src, a, cb, bias)
    worst = {}
    for name, want in (("scores", tr["scores"]), ("scores_now", tr["scores"] - logw[None])):
        ratio = (res[name].double() - want).abs() / E
        assert not bool(torch.isnan(ratio).any()), f"{c.id}: {name}: NaN"
        worst[name] = float(ratio.max())
    # nll
    M = tr["scores"].max(1).values
    logS = torch.log(torch.exp(tr["scores"] - M[:, None]).sum(1))
    Enll = E.max(1).values + gamma(K * (2 * EXP_ULP + 3)) + 2 * LOG_ULP * U * logS.abs() + 2 * U * (M.abs() + logS.abs())
    worst["nll"] = float(((res["nll"].double() + (M + logS)).abs() / Enll).max())

    def check_class(k, what):
        best = tr["scores"].argmax(1)
        clear = ~amb
        bad = clear & (k != best)
        assert not bool(bad.any()), f"{c.id}: {what}: {int(bad.sum())} clear patches are classified wrong, the first is patch {int(bad.nonzero()[0])}"
        chosen = tr["scores"].gather(1, k[:, None])[:, 0]
        off = tr["scores"].max(1).values - chosen > 2 * E.max(1).values
        assert not bool(off.any()), f"{c.id}: {what}: {int(off.sum())} ambiguous patches got a component outside the bound"
    assert bool(((res["kstar"] >= 0) & (res["kstar"] < K)).all()), f"{c.id}: k* out of range"
    check_class(res["kstar"].long(), "argmax")
    if "z" in res:
        k = res["kstep"].long()
        assert torch.equal(k, res["kstar"].long()), f"{c.id}: the step's k* differ from the argmax call's"
        want_z, Ez, want, Eout = step_truth(c, model, src, k, a, cb, bias)
        worst["z"] = float(((res["z"].double() - want_z).abs() / Ez).max())
        worst["out"] = float(((res["out"].double() - want).abs() / Eout).max())
    print(f"{c.id}: worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f"; {int(amb.sum())} ambiguous patches")
    for name, v in worst.items():
        assert v <= 1.0, f"{c.id}: {name}: an element is {v:.3g} times its bound"
    return worst


def run_case(r, c):
    run_exact(r, c)
    return run_rounding(r, c)


# ------------------------------------------------------------------ ties and refusals (shared by both test files)
def run_ties(r):
    """components 1 and 3 are copies of 0 and 2: k* is never 1 or 3, in rows and in image mode"""
    for c in (Case("rows", 4, d_rows=9, N_rows=65, r=R1), Case("image", 4, C=1, p=3, B=1, H=6, W=9, r=R1)):
        gen = torch.Generator().manual_seed(5)
        Wt, m, lam, logw, rr = random_model(Case(c.mode, 2, c.d_rows, c.N_rows, c.C, c.p, c.B, c.H, c.W, c.r), gen)
        d = c.d
        model = (Wt.reshape(2, d * d)[[0, 0, 1, 1]].reshape(4 * d, d), m.reshape(2, d)[[0, 0, 1, 1]].reshape(-1),
                 lam.reshape(2, d)[[0, 0, 1, 1]].reshape(-1), torch.full((4,), math.log(0.25), dtype=torch.float64), rr)
        src = _source(c, gen, False)
        rc, out = r.scores(c, _device_model(r, model), r.buf(src), ARGMAX)
        assert rc == 0, r.err()
        k = _written(c, "ties", out)
        assert set(k.tolist()) <= {0, 2}, f"{c.id}: k* = {sorted(set(k.tolist()))}, expected 0 and 2 only"


def run_refusals(r):
    """every DINV_REQUIRE of the two entry points (csrc/dense.hip, csrc/patch_gmm.hpp), each by a word of its own message, and the
    empty batch launching nothing.  Every refusal returns before a launch, so the operands need not fit the shapes named."""
    c = Case("image", 3, C=1, p=3, B=2, H=5, W=6, r=(0.05, 0.1))
    gen = torch.Generator().manual_seed(9)
    model = random_model(c, gen)
    ops = _device_model(r, model)
    src = r.buf(_source(c, gen, False))
    a = r.buf(torch.ones(c.B))

    def refused(rc, out, word):
        assert rc == 2 and word in r.err(), f"expected a refusal naming '{word}', got {rc}: {r.err()}"
        assert out.untouched(), f"refusal '{word}' wrote to the output"

    def variant(**kw):
        f = {k: getattr(c, k) for k in ("mode", "K", "d_rows", "N_rows", "C", "p", "B", "H", "W", "r")}
        f.update(kw)
        return Case(**f)

    big = Guarded(c.N * c.K, r.device)
    rc, out = r.scores(c, ops, src, 3, out=big); refused(rc, out, "unknown epilogue")
    rc, out = r.scores(variant(p=2, d_rows=9), ops, src, SCORES, out=Guarded(64, r.device)); refused(rc, out, "dimension")
    rc, out = r.scores(variant(H=2, C=1), ops, src, SCORES, out=Guarded(64, r.device)); refused(rc, out, "holds no")
    rc, out = r.scores(variant(K=0), ops, src, SCORES, out=Guarded(64, r.device)); refused(rc, out, "bad model")
    rc, out = r.scores(variant(mode="rows", N_rows=1 << 31, d_rows=9), ops, src, ARGMAX, out=Guarded(64, r.device)); refused(rc, out, "2^31")
    rc, out = r.scores(variant(B=60000, H=300, W=300), ops, src, ARGMAX, out=Guarded(64, r.device)); refused(rc, out, "2^31")
    rc, out = r.scores(variant(K=1 << 20, mode="rows", d_rows=9, N_rows=4), ops, src, ARGMAX, out=Guarded(64, r.device))
    refused(rc, out, "K = 1048576 needs")
    rc, out = r.scores(c, (None, *ops[1:]), src, SCORES, out=big); refused(rc, out, "operands Wt, m and lam must be non-null")
    rc, out = r.scores(c, ops, None, SCORES, out=big); refused(rc, out, "src and out must be non-null")
    before = src.bits().clone()
    rc, out = r.scores(c, ops, src, ARGMAX, out=src)
    assert rc == 2 and "must not alias" in r.err() and torch.equal(src.bits(), before), r.err()
    # the shape checks that come before the model meets the image
    rc, out = r.scores(variant(C=0, d_rows=9), ops, src, SCORES, out=Guarded(64, r.device)); refused(rc, out, "bad shape")
    rc, out = r.scores(variant(p=0, d_rows=9), ops, src, SCORES, out=Guarded(64, r.device)); refused(rc, out, "bad shape")
    rc, out = r.scores(variant(B=-1), ops, src, SCORES, out=Guarded(64, r.device)); refused(rc, out, "bad shape")
    rc, out = r.scores(variant(K=1 << 29, mode="rows", d_rows=9, N_rows=4), ops, src, ARGMAX, out=Guarded(64, r.device))
    refused(rc, out, "rows exceed 2^31")
    # 2^20 + 1 rows of patches are 65537 workgroups of 16 rows (NP = 4) along y
    tall = variant(B=1, H=(1 << 20) + 3, W=3)
    assert patch_tiles(tall) == 4
    rc, out = r.scores(tall, ops, src, ARGMAX, out=Guarded(64, r.device)); refused(rc, out, "too tall")
    rc, out = r.scores(variant(K=1000, mode="rows", d_rows=9, N_rows=(1 << 31) - 1), ops, src, SCORES, out=Guarded(64, r.device))
    refused(rc, out, "score matrix")
    rc, out = r.scores(variant(K=50000), ops, src, ARGMAX, out=Guarded(64, r.device)); refused(rc, out, "C = 1, p = 3 need")
    # the step: r and a are needed, the workspace one byte short
    rc, out, ws = r.step(c, (*ops[:4], None), src, a, None, None); refused(rc, out, "non-null")
    rc, out, ws = r.step(c, ops, src, None, None, None); refused(rc, out, "non-null")
    rc, out, ws = r.step(c, ops, src, a, None, None, ws_bytes=workspace_bytes(c) - 1); refused(rc, out, "are needed")
    assert ws.untouched(), "the refused step wrote to its workspace"
    rc, out, ws = r.step(c, ops, src, a, None, None, ws_off=4); refused(rc, out, "16-byte aligned")
    assert ws.untouched(), "the refused step wrote to its workspace"
    # d = 3 x 46 x 46: the image and the LDS of the score kernel pass, the 2 d floats of the estimate kernel do not
    wide = variant(C=3, p=46, B=1, H=46, W=46)
    assert lds_bytes(wide) <= MAX_LDS and 8 * wide.d > 48 * 1024
    rc, out, ws = r.step(wide, ops, src, a, None, None); refused(rc, out, "estimate kernel")
    assert ws.untouched(), "the refused step wrote to its workspace"
    # an empty batch launches nothing and is no error
    empty = variant(B=0)
    rc, out = r.scores(empty, ops, src, SCORES, out=Guarded(64, r.device))
    assert rc == 0 and out.untouched()
    if r.launches is not None:
        assert r.launches() == []
    rc, out = r.scores(variant(mode="rows", N_rows=0, d_rows=9), ops, src, NLL, out=Guarded(64, r.device))
    assert rc == 0 and out.untouched()
    if r.launches is not None:
        assert r.launches() == []
