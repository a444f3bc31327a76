"""Shared by tests/test_variational_kernels_gpu.py (the gfx950 library) and tests/test_emu_variational_cases.py (the same kernel
sources on the host emulation): the case table of csrc/tv.hip and csrc/tgv.hip - one Chambolle-Pock step from a general state,
the four difference operators alone, TVPrior.grad and TVPrior.fn, the device stop and every refusal - the fp64 restatements of
deepinv's tv.py / tgv.py / prior.py (the one copy: tests/test_tv_gpu.py, test_tgv_gpu.py, test_emu_tv.py and test_emu_tgv.py
import them from here) and the runner that calls the C entry points on guarded buffers (tests/fft_cases.py Guarded).

Error measure, per element: |out - ref| <= c U M with U = 2^-24.  M is the reference expression evaluated on absolute values
with every subtraction turned into an addition (`ab=True` of the restatements), so every intermediate of the fp32 evaluation
is bounded by its own M and a rounding of it moves the output by at most U M.  c is the number of fp32 roundings on the longest
path to the output: BOUNDS counts them.  The two projections onto a ball, v / max(|v| / lam, 1) and s - s / max(|s| / lam, 1),
are 1-Lipschitz in the 2-norm over the component axis, which is why their outputs are measured by the 2-norm of the component
measures, the same for every component of the pixel.  A dropped or misplaced term is about 1e5 U M.  The fp64 references take
the fp32 values of tau, sigma, rho and lam, so the constants are no source of error.

Every operand is guarded, every call is made twice on fresh buffers with identical bits, the set that a call reads must be
unchanged bit for bit and every word of the set that it writes must be written."""
import math
from dataclasses import dataclass

import torch

from fft_cases import GUARD, POISON, Guarded

U = 2.0 ** -24
THREADS, MAX_BLOCKS = 256, 2048            # csrc/tv_common.hpp kThreads, kMaxBlocks
F64 = torch.float64


def cdiv(a, b):
    return -(-a // b)


def f32(v):
    """the fp32 value of a Python float, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


TAU, RHO = f32(0.01), f32(1.99)


def tv_sigma(nd):
    return f32(1 / 0.01 / 2 ** (nd + 1))             # tv.py:66 (12.5 and 6.25: exact)


def tgv_sigma(nd):
    return f32(1 / 0.01 / (72 * (3 if nd == 3 else 1)))   # tgv.py:61


# ------------------------------------------------------------------ the launchers' grid rules, restated
def grid_for(n):
    """csrc/tv_common.hpp grid_for: workgroups of the TV / TGV kernels (dinv_tv_cp_partials, dinv_tgv_cp_partials)"""
    return min(max(cdiv(n, THREADS), 1), MAX_BLOCKS)


def tv_fn_blocks(per_sample):
    """csrc/tv.hip dinv_tv_fn_blocks"""
    return min(max(cdiv(per_sample, 4 * THREADS), 1), 256)


# ------------------------------------------------------------------ fp64 restatements (tv.py:154-218, tgv.py:230-310)
# (ab=True: the abs-measure of the same expression, on non-negative inputs: every subtraction an addition)
def _sl(ndim, axis, s):
    a = [slice(None)] * ndim
    a[axis] = s
    return a


def r_nabla(x, ab=False):
    nd = x.ndim - 2
    u = torch.zeros((*x.shape, nd), dtype=x.dtype, device=x.device)
    for i in range(nd):
        a, b = _sl(x.ndim, i + 2, slice(None, -1)), _sl(x.ndim, i + 2, slice(1, None))
        u[(*a, i)] = x[tuple(b)] + x[tuple(a)] if ab else x[tuple(b)] - x[tuple(a)]
    return u


def r_nabla_adjoint(v, ab=False):
    nd = v.ndim - 3
    u = torch.zeros(v.shape[:-1], dtype=v.dtype, device=v.device)
    for i in range(nd):
        a, b = _sl(u.ndim, i + 2, slice(None, -1)), _sl(u.ndim, i + 2, slice(1, None))
        gs = _sl(v.ndim, i + 2, slice(None, -1))
        gs[-1] = i
        if ab:
            u[tuple(a)] += v[tuple(gs)]
        else:
            u[tuple(a)] -= v[tuple(gs)]
        u[tuple(b)] += v[tuple(gs)]
    return u


def r_epsilon(v, ab=False):
    nd = v.ndim - 3
    out = torch.zeros((*v.shape[:-1], nd * nd), dtype=v.dtype, device=v.device)
    for i in range(nd):
        for j in range(nd):
            a, b = _sl(v.ndim - 1, j + 2, slice(None, -1)), _sl(v.ndim - 1, j + 2, slice(1, None))
            out[(*b, i * nd + j)] = v[(*b, i)] + v[(*a, i)] if ab else v[(*b, i)] - v[(*a, i)]
    return out


def r_epsilon_adjoint(u, ab=False):
    nd = u.ndim - 3
    out = torch.zeros((*u.shape[:-1], nd), dtype=u.dtype, device=u.device)
    for i in range(nd):
        for j in range(nd):
            a, b = _sl(u.ndim - 1, j + 2, slice(None, -1)), _sl(u.ndim - 1, j + 2, slice(1, None))
            if ab:
                out[(*a, i)] += u[(*b, i * nd + j)]
            else:
                out[(*a, i)] -= u[(*b, i * nd + j)]
            out[(*b, i)] += u[(*b, i * nd + j)]
    return out


def tv_iteration(y, x2, u2, lam, aniso, tau, sigma, rho):
    """one over-relaxed Chambolle-Pock iteration of TVDenoiser / TVL1Denoiser (tv.py:131-139, 221-240); lam is [B].
    Returns (x2', u2', which records the projection moved: components if aniso, pixels otherwise)"""
    lam = lam.view(-1, *([1] * y.ndim))
    x = (x2 - tau * r_nabla_adjoint(u2) + tau * y) / (1 + tau)
    v = u2 + sigma * r_nabla(2 * x - x2)
    if aniso:
        u, moved = torch.clamp(v, -lam, lam), v.abs() > lam
    else:
        d = v.norm(dim=-1, keepdim=True) / lam
        u, moved = v / torch.clamp(d, min=1.0), d > 1
    return x2 + rho * (x - x2), u2 + rho * (u - u2), moved


def tv_measure(y, x2, u2, aniso, tau, sigma, rho):
    """the abs-measures of (x2', u2') of tv_iteration"""
    y, x2, u2 = y.abs(), x2.abs(), u2.abs()
    mx = (x2 + tau * r_nabla_adjoint(u2, True) + tau * y) / (1 + tau)
    mv = u2 + sigma * r_nabla(2 * mx + x2, True)
    if not aniso:
        mv = mv.norm(dim=-1, keepdim=True).expand_as(mv)
    return x2 + rho * (mx + x2), u2 + rho * (mv + u2)


def r_tv_prox(y, lam, x2, u2, n_it, crit, aniso, tau=0.01, rho=1.99, rels=None):
    """TVDenoiser.forward (tv.py:86-152) from the state (x2, u2): (x2, u2, iterations run); `rels` collects the stopping ratios"""
    sigma = 1 / tau / 2 ** (y.ndim - 1)
    it_run = 0
    for it in range(n_it):
        x_prev = x2
        x2, u2, _ = tv_iteration(y, x2, u2, lam, aniso, tau, sigma, rho)
        it_run = it + 1
        if rels is not None or crit > 0:
            rel = float((x_prev - x2).norm() / (x2 + 1e-12).norm())
            if rels is not None:
                rels.append(rel)
            if it > 1 and rel < crit:
                break
    return x2, u2, it_run


def tgv_iteration(y, x2, r2, u2, l1, l2, tau, sigma, rho):
    """one over-relaxed Chambolle-Pock iteration of TGVDenoiser (tgv.py:148-160); l1, l2 are [B].
    Returns (x2', r2', u2', z, w, pixels whose r was shrunk, pixels whose u was projected)"""
    l1, l2 = (t.view(-1, *([1] * (y.ndim - 1))) for t in (l1, l2))
    t = tau * r_epsilon_adjoint(u2)
    x = (x2 - r_nabla_adjoint(t) + tau * y) / (1 + tau)
    s = r2 + t
    d1 = s.norm(dim=-1) / (tau * l1)
    r = s - s / torch.clamp(d1, min=1.0).unsqueeze(-1)
    z, w = 2 * x - x2, 2 * r - r2
    v = u2 + sigma * r_epsilon(r_nabla(z) - w)
    d2 = v.norm(dim=-1) / l2
    u = v / torch.clamp(d2, min=1.0).unsqueeze(-1)
    return x2 + rho * (x - x2), r2 + rho * (r - r2), u2 + rho * (u - u2), z, w, d1 > 1, d2 > 1


def tgv_measure(y, x2, r2, u2, tau, sigma, rho):
    """the abs-measures of (x2', r2', u2', z, w) of tgv_iteration"""
    y, x2, r2, u2 = y.abs(), x2.abs(), r2.abs(), u2.abs()
    t = tau * r_epsilon_adjoint(u2, True)
    mx = (x2 + r_nabla_adjoint(t, True) + tau * y) / (1 + tau)
    ms = (r2 + t).norm(dim=-1, keepdim=True).expand_as(r2)
    mr = 2 * ms
    mz, mw = 2 * mx + x2, 2 * mr + r2
    mv = u2 + sigma * r_epsilon(r_nabla(mz, True) + mw, True)
    mv = mv.norm(dim=-1, keepdim=True).expand_as(mv)
    return x2 + rho * (mx + x2), r2 + rho * (mr + r2), u2 + rho * (mv + u2), mz, mw


def r_tgv_prox(y, lam, x2, r2, u2, n_it, crit, tau=0.01, rho=1.99, rels=None):
    """TGVDenoiser.forward (tgv.py:93-214) from the state (x2, r2, u2): (x2, r2, u2, iterations run)"""
    nd = y.ndim - 2
    sigma = 1 / tau / (72 * (3 if nd == 3 else 1))
    l1, l2 = 0.1 * lam, 0.15 * lam
    it_run = 0
    for it in range(n_it):
        x_prev = x2
        x2, r2, u2 = tgv_iteration(y, x2, r2, u2, l1, l2, tau, sigma, rho)[:3]
        it_run = it + 1
        if rels is not None or crit > 0:
            rel = float((x_prev - x2).norm() / (x2.norm() + 1e-12))
            if rels is not None:
                rels.append(rel)
            if it > 1 and rel < crit:
                break
    return x2, r2, u2, it_run


def r_tv_grad_terms(x):
    """TVPrior.grad (prior.py:554-582): (nabla^T (Dx / |Dx|), its abs-measure, |Dx|)"""
    dx = r_nabla(x)
    n = dx.norm(dim=-1, keepdim=True)
    g = torch.where(n > 0, dx / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(dx))
    return r_nabla_adjoint(g), r_nabla_adjoint(g.abs(), True), n.squeeze(-1)


def r_tv_fn(x, mode):
    """TVPrior.fn / TVL1Prior.fn (prior.py:485-552, 584-612): per sample, the sum over the pixels of |Dx|_2 (mode 0) or |Dx|_1"""
    dx = r_nabla(x)
    per = dx.abs().sum(dim=-1) if mode else dx.norm(dim=-1)
    return per.reshape(x.shape[0], -1).sum(dim=1)


# ------------------------------------------------------------------ the bounds: c of |out - ref| <= c U M, counted
def _tv_x(nd):
    # nabla^T u2: 2 nd terms, 2 nd - 1 additions; tau *; x2 -; + tau y (the product is off the longest path); the rounded
    # 1 + tau and the division; x - x2; rho *; x2 +
    return (2 * nd - 1) + 1 + 1 + 1 + 2 + 3


def _tv_v(nd):
    # x as above without the relaxation (2 nd + 4); z = 2 x - x2: 1; z(p + e_k) - z(p): 1 (both sides carry the same count and
    # the measure adds them); sigma *; u2 +
    return (2 * nd + 4) + 1 + 1 + 2


def _ball(ncomp):
    # v / max(|v| / lam, 1) itself: the sum of ncomp squares is relatively off by ncomp U (a product and ncomp - 1 additions
    # of non-negative terms), the root halves it and adds 1, / lam 1, the division of v 1
    return math.ceil(ncomp / 2) + 3


def _tgv_x(nd):
    # t = tau eps^T(u2): 2 nd - 1 additions and the product (2 nd); nabla^T t: 2 nd such terms, 2 nd - 1 additions; x2 -;
    # + tau y; the rounded 1 + tau and the division
    return 2 * nd + (2 * nd - 1) + 1 + 1 + 2


def _tgv_r(nd):
    # s = r2 + t: 2 nd + 1, carried through the 1-Lipschitz s - P(s); the ball (with tau * lam1 one rounding more) and the
    # subtraction
    return (2 * nd + 1) + (_ball(nd) + 1) + 1


def _tgv_v(nd):
    # G = nabla z - w: z carries _tgv_x + 1, the difference 1, - w 1 (w carries fewer: _tgv_r + 1); G(p) - G(p - e_j): 1;
    # sigma *; u2 +
    return max(_tgv_x(nd) + 2, _tgv_r(nd) + 1) + 1 + 1 + 2


# key -> nd -> c, and for the record the worst kernel error / bound on the MI355X over the table (2-D, 3-D) with its case, as the
# *_worst_ratio test of tests/test_variational_kernels_gpu.py and the lines of the cases print them
BOUNDS = {
    # x and the relaxation: 11, 13.  0.272 (1x3x419x419), 0.216 (1x1x9x241x243-aniso)
    "tv.x2": {2: _tv_x(2), 3: _tv_x(3)},
    # v, an exact clamp, u - u2, rho *, u2 +: 15, 17.  0.135, 0.114 (the strided shapes)
    "tv.u2.aniso": {2: _tv_v(2) + 3, 3: _tv_v(3) + 3},
    # v, the ball, the relaxation: 19, 22.  0.085, 0.066 (the strided shapes)
    "tv.u2.iso": {2: _tv_v(2) + _ball(2) + 3, 3: _tv_v(3) + _ball(3) + 3},
    "tgv.x2": {2: _tgv_x(2) + 3, 3: _tgv_x(3) + 3},                 # 14, 18.  0.156, 0.098 (the strided shapes)
    "tgv.z": {2: _tgv_x(2) + 1, 3: _tgv_x(3) + 1},                  # 12, 16: 2 x - x2.  0.204, 0.129 (the strided shapes)
    "tgv.r2": {2: _tgv_r(2) + 3, 3: _tgv_r(3) + 3},                 # 14, 17.  0.122, 0.085 (the strided shapes)
    "tgv.w": {2: _tgv_r(2) + 1, 3: _tgv_r(3) + 1},                  # 12, 15: 2 r - r2.  0.137, 0.082 (the strided shapes)
    # v, the ball of nd^2 components, the relaxation: 25, 32.  0.038 (2x2x37x1), 0.022 (1x1x9x241x243)
    "tgv.u2": {2: _tgv_v(2) + _ball(4) + 3, 3: _tgv_v(3) + _ball(9) + 3},
    "nabla": {2: 2, 3: 2},                                          # the number of terms (one subtraction).  0.5, 0.5
    "nabla_adjoint": {2: 4, 3: 6},                                  # 2 nd terms.  0.645 (1x3x419x419), 0.493
    "epsilon": {2: 2, 3: 2},                                        # 0.5, 0.5
    "epsilon_adjoint": {2: 4, 3: 6},                                # 0.66 (1x3x419x419: the worst of the table), 0.534
    # exact differences and |Dx|^2 (eighths): each of the 2 nd terms is a root and a division (2), summed by 2 nd - 1 additions
    "tv_grad": {2: 2 + 3, 3: 2 + 5},                                # 0.229 (3x2x17x19), 0.328 (1x1x9x241x243)
}
# (dinv_tv_fn, tv_fn_bound below: 0.0996 (1x1x1x7, mode 1); on the host emulation the worst of the table is 0.5, tgv-ops-3x2x17x19)
assert max(max(v.values()) for v in BOUNDS.values()) <= 64


def tv_fn_bound(nd, mode, per_sample):
    """c of dinv_tv_fn against the sum itself (every term is non-negative): the roundings of one term - mode 0: a difference, nd
    squares and nd - 1 additions under a root, (1 + 2 + nd - 1) / 2 + 1; mode 1: a difference and nd - 1 additions - and the
    summation depth restated from the code: terms per lane, 6 shuffle levels, 2 LDS levels, then the per-lane terms of the final
    kernel and its 6 shuffle levels"""
    nblk = tv_fn_blocks(per_sample)
    term = math.ceil((nd + 2) / 2) + 1 if mode == 0 else nd
    return term + cdiv(per_sample, nblk * THREADS) + 6 + 2 + cdiv(nblk, 64) + 6


# ------------------------------------------------------------------ the case table
EDGE = [(1, 1, 1, 1), (2, 3, 1, 1), (1, 1, 1, 7), (1, 1, 7, 1), (1, 1, 1, 300), (2, 2, 37, 1), (1, 1, 2, 2),
        (1, 1, 1, 5, 6), (1, 2, 4, 1, 5), (1, 1, 3, 4, 1), (1, 1, 2, 2, 2)]
ORDINARY = [(3, 2, 17, 19), (2, 1, 5, 9, 7), (1, 1, 16, 16), (1, 1, 16, 17)]
STRIDED = [(1, 3, 419, 419), (1, 1, 9, 241, 243)]        # above grid_for's 2048 x 256 pixels and no multiple of 256
FN_STRIDED = (2, 3, 419, 419)                            # above dinv_tv_fn's 256 x 1024 pixels per sample, two samples
STOP = [(3, 2, 17, 19), (2, 1, 5, 9, 7)]
# one sample takes the first lam of the range, which projects more than 90 % of the records of these shapes: the middle instead
TGV_LAM = {(1, 1, 16, 16): (10.0, 10.0), (1, 1, 16, 17): (10.0, 10.0), (1, 3, 419, 419): (10.0, 10.0), (1, 1, 9, 241, 243): (12.0, 12.0)}
STOP_LAM = (1.0, 3.0)
MIN_RECORDS = 64                                         # the branch-share conditions hold from this many records


@dataclass(frozen=True)
class Case:
    kind: str                   # tv-step | tgv-step | tv-ops | tgv-ops | tv-grad | tv-fn | tv-stop | tgv-stop
    shape: tuple
    aniso: int = 0              # tv-step, tv-stop
    emu: bool = True
    lam: tuple = ()             # the range of the per-sample lam where not the kind's default
    dual: float = 0.0           # the scale of the random dual state where not the default

    @property
    def id(self):
        return f"{self.kind}-{'x'.join(map(str, self.shape))}" + ("-aniso" if self.aniso else "")

    @property
    def nd(self):
        return len(self.shape) - 2

    @property
    def geo(self):
        s = self.shape
        return (2, s[0], s[1], 1, s[2], s[3]) if len(s) == 4 else (3, *s)

    @property
    def n(self):
        return math.prod(self.shape)


def _table():
    t = []
    for shape in EDGE + ORDINARY + STRIDED:
        emu = shape not in STRIDED
        # (a strided step takes the emulation half a minute; the operators and the gradient two seconds: those run there too)
        t += [Case("tv-step", shape, 0, emu), Case("tv-step", shape, 1, emu), Case("tgv-step", shape, 0, emu, TGV_LAM.get(shape, ())),
              Case("tv-ops", shape), Case("tgv-ops", shape), Case("tv-grad", shape)]
        if emu:
            t.append(Case("tv-fn", shape))
    t.append(Case("tv-fn", FN_STRIDED, emu=False))
    for shape in STOP:
        t += [Case("tv-stop", shape, 0, lam=STOP_LAM), Case("tv-stop", shape, 1, lam=STOP_LAM), Case("tgv-stop", shape, lam=STOP_LAM)]
    return t


TABLE = _table()
assert len({c.id for c in TABLE}) == len(TABLE), "duplicate case ids"


def _seed(cid):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(cid)) % (2 ** 31)


def _gen(c):
    return torch.Generator().manual_seed(_seed(c.id))


def _round32(*ts):
    return tuple(t.float().double() for t in ts)


# ---- the general states (fp64 tensors holding fp32 values)
def tv_state(c):
    """y ~ U(0,1), x2 = y + 0.1 N, u2 = 0.2 N and lam = linspace(3, 7, B): both sides of the projection are taken"""
    g, B = _gen(c), c.shape[0]
    y = torch.rand(c.shape, generator=g, dtype=F64)
    x2 = y + 0.1 * torch.randn(c.shape, generator=g, dtype=F64)
    u2 = (c.dual or 0.2) * torch.randn(*c.shape, c.nd, generator=g, dtype=F64)
    lam = torch.linspace(*(c.lam or (3.0, 7.0)), B, dtype=F64)
    return _round32(y, x2, u2, lam)


def tgv_state(c):
    """y ~ U(0,1), x2 = y + 0.1 N, r2 = 0.004 N, u2 = 0.5 N and lam = linspace(6, 14, B) (lam1 = 0.1 lam, lam2 = 0.15 lam)"""
    g, B = _gen(c), c.shape[0]
    y = torch.rand(c.shape, generator=g, dtype=F64)
    x2 = y + 0.1 * torch.randn(c.shape, generator=g, dtype=F64)
    r2 = 0.004 * torch.randn(*c.shape, c.nd, generator=g, dtype=F64)
    u2 = (c.dual or 0.5) * torch.randn(*c.shape, c.nd * c.nd, generator=g, dtype=F64)
    lam = torch.linspace(*(c.lam or (6.0, 14.0)), B, dtype=F64)
    return _round32(y, x2, r2, u2, 0.1 * lam, 0.15 * lam)


def grad_image(c):
    """values in {0, 1/8, ..., 1} constant on patches of 3 pixels per axis: the differences and |Dx|^2 are exact in fp32 and
    |Dx| = 0 exactly inside a patch"""
    g = _gen(c)
    coarse = torch.randint(0, 9, tuple(c.shape[:2]) + tuple(cdiv(s, 3) for s in c.shape[2:]), generator=g).double() / 8
    x = coarse
    for ax in range(2, len(c.shape)):
        x = x.repeat_interleave(3, dim=ax).narrow(ax, 0, c.shape[ax])
    return x.contiguous()


def tv_step_ref(c):
    y, x2, u2, lam = tv_state(c)
    args = (TAU, tv_sigma(c.nd), RHO)
    xn, un, moved = tv_iteration(y, x2, u2, lam, c.aniso, *args)
    return (y, x2, u2, lam), (xn, un), tv_measure(y, x2, u2, c.aniso, *args), moved


def tgv_step_ref(c):
    y, x2, r2, u2, l1, l2 = tgv_state(c)
    args = (TAU, tgv_sigma(c.nd), RHO)
    out = tgv_iteration(y, x2, r2, u2, l1, l2, *args)
    return (y, x2, r2, u2, l1, l2), out[:5], tgv_measure(y, x2, r2, u2, *args), out[5:]


def step_bounds(c):
    nd = c.nd
    if c.kind == "tv-step":
        return [BOUNDS["tv.x2"][nd], BOUNDS["tv.u2.aniso" if c.aniso else "tv.u2.iso"][nd]]
    return [BOUNDS[k][nd] for k in ("tgv.x2", "tgv.r2", "tgv.u2", "tgv.z", "tgv.w")]


def fp32_step_ratio(c):
    """the worst error / bound of the fp32 evaluation of the restatement itself: a bound a correct fp32 implementation meets"""
    if c.kind == "tv-step":
        (y, x2, u2, lam), ref, meas, _ = tv_step_ref(c)
        got = tv_iteration(y.float(), x2.float(), u2.float(), lam.float(), c.aniso, TAU, tv_sigma(c.nd), RHO)[:2]
    else:
        st, ref, meas, _ = tgv_step_ref(c)
        got = tgv_iteration(*(t.float() for t in st), TAU, tgv_sigma(c.nd), RHO)[:5]
    return max(_ratio(f"{c.id} fp32 restatement", g.double(), r, m, b, quiet=True) for g, r, m, b in zip(got, ref, meas, step_bounds(c)))


def branch_shares(c):
    """the share of records on the moved side of each projection of case c, {name: share}; None where the case is too small
    for the condition (fewer than MIN_RECORDS records) or has no branch"""
    if c.kind == "tv-step":
        moved = tv_step_ref(c)[3]
        shares = {"projected": moved}
    elif c.kind == "tgv-step":
        shrunk, projected = tgv_step_ref(c)[3]
        shares = {"r shrunk": shrunk, "u projected": projected}
    elif c.kind == "tv-grad":
        shares = {"|Dx| > 0": r_tv_grad_terms(grad_image(c))[2] > 0}
    else:
        return None
    if c.n < MIN_RECORDS:
        return None
    return {k: float(v.double().mean()) for k, v in shares.items()}


# ---- the stop
def stop_lam(c):
    return torch.linspace(*c.lam, c.shape[0], dtype=F64).float().double()


def stop_image(c):
    """a ramp along W with noise of 0.05: from a cold start on plain noise under a small lam the stopping ratio alternates
    between a large and a small value and its minimum is at iteration 2, the first that the rule tests; this image under a lam
    of order 1 gives a sequence that falls past iteration 4"""
    ramp = torch.linspace(0, 1, c.shape[-1], dtype=F64).expand(c.shape)
    return (ramp + 0.05 * torch.randn(c.shape, generator=_gen(c), dtype=F64)).float().double()


def stop_plan(c):
    """(y, lam, k, crit, rels): the first k in 4..12 of the fp64 cold-start sequence rel_0, rel_1, ... with rel_k < 0.99 crit and
    rel_j > 1.01 crit for every earlier j that the rule tests (j = 2 .. k - 1), crit = sqrt(rel_k rel_{k-1}): fp32 cannot move
    the stop.  k = 0 if there is none"""
    y, lam, rels = stop_image(c), stop_lam(c), []
    if c.kind == "tv-stop":
        r_tv_prox(y, lam, y, torch.zeros(*c.shape, c.nd, dtype=F64), 13, 0.0, c.aniso, rels=rels)
    else:
        r_tgv_prox(y, lam, y, torch.zeros(*c.shape, c.nd, dtype=F64), torch.zeros(*c.shape, c.nd ** 2, dtype=F64), 13, 0.0, rels=rels)
    for k in range(4, 13):
        crit = math.sqrt(rels[k] * rels[k - 1])
        if rels[k] < 0.99 * crit and min(rels[2:k]) > 1.01 * crit:
            return y, lam, k, crit, rels
    return y, lam, 0, 0.0, rels


# ------------------------------------------------------------------ the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.tv and .tgv), `device` of its
    buffers, `stream()` -> the stream argument"""

    def __init__(self, lib, device, stream):
        self.lib, self.device, self._stream = lib, torch.device(device), stream

    def err(self):
        return self.lib.dinv_last_error().decode()

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def tv_iter(self, geo, xa, xb, ua, ub, y, lam, aniso, tau, sigma, rho, crit, partial, state):
        return self.lib.dinv_tv_cp_iter(*geo, xa, xb, ua, ub, y, lam, aniso, tau, sigma, rho, crit, partial, state, self._stream())

    def tgv_iter(self, geo, xa, xb, ra, rb, ua, ub, y, l1, l2, tau, sigma, rho, crit, z, w, partial, state):
        return self.lib.dinv_tgv_cp_iter(*geo, xa, xb, ra, rb, ua, ub, y, l1, l2, tau, sigma, rho, crit, z, w, partial, state,
                                         self._stream())

    def operator(self, name, geo, src, out):
        nd, B, C, D, H, W = geo
        return getattr(self.lib, name)(nd, B * C, D, H, W, src, out, self._stream())

    def tv_fn(self, geo, mode, x, out, partial):
        nd, B, C, D, H, W = geo
        return self.lib.dinv_tv_fn(nd, mode, B, C, D, H, W, x, out, partial, self._stream())


def _p(g, off_bytes=0):
    return None if g is None else g.t.data_ptr() + off_bytes


def _copy(r, t):
    """a guarded device copy of the fp32 values of t, and its bits"""
    g = Guarded(t.numel(), r.device)
    g.t.copy_(t.reshape(-1).float())
    return g, g.bits().clone()


def _state(r, done, it):
    g = Guarded(2, r.device)
    g.full[GUARD:GUARD + 2] = torch.tensor([done, it], dtype=torch.int32)
    return g


def _state_of(g):
    return tuple(g.full[GUARD:GUARD + 2].tolist())


def twice(tag, once):
    """`once()` -> {name: bits of an output} on fresh buffers, two times: identical bits"""
    a, b = once(), once()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{tag}: two identical calls differ in {k}"
    return a


def _written(tag, r, rc, outs, operands):
    """after one call: status 0, every guard intact, every output word written, every operand unchanged"""
    assert rc == 0, f"{tag}: error {rc}: {r.err()}"
    r.sync()
    for name, g in outs.items():
        assert g.guards_intact(), f"{tag}: write outside {name}"
        bad = g.bits() == POISON
        assert not bool(bad.any()), f"{tag}: {int(bad.sum())} words of {name} hold the guard pattern: never written, or read from outside"
    for name, (g, before) in operands.items():
        assert g.guards_intact() and torch.equal(g.bits(), before), f"{tag}: the call modified {name}"


def _ratio(tag, got, ref, measure, c, quiet=False):
    """the worst |got - ref| / (c U measure) over the elements; where the measure is zero the element must be exactly zero"""
    got, ref, measure = got.reshape(-1), ref.reshape(-1), measure.reshape(-1)
    assert not bool(torch.isnan(got).any()), f"{tag}: NaN in the result"
    err, bound = (got - ref).abs(), c * U * measure
    zero = bound == 0
    assert bool((got[zero] == 0).all()), f"{tag}: an element that no term reaches is not exactly zero"
    ratio = torch.where(zero, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max())
    at = int(ratio.argmax())
    if not quiet:
        print(f"{tag}: worst element {at} error / bound {worst:.3g} ({worst * c:.3g} U against c = {c})")
    assert worst <= 1.0, f"{tag}: element {at} is {worst:.3g} times its bound of {c} U M"
    return worst


def _f(bits, shape):
    return bits.view(torch.float32).view(shape).double()


# ---- one step from a general state
def run_tv_step(r, c):
    (y, x2, u2, lam), ref, meas, _ = tv_step_ref(c)
    n, nd = c.n, c.nd
    nblk = int(r.lib.dinv_tv_cp_partials(n))
    assert nblk == grid_for(n), (nblk, grid_for(n))
    worst = 0.0
    for parity in (0, 1):
        tag = f"{c.id}-it{parity}"

        def once():
            X, Uu = [Guarded(n, r.device) for _ in range(2)], [Guarded(n * nd, r.device) for _ in range(2)]
            X[parity].t.copy_(x2.reshape(-1).float())
            Uu[parity].t.copy_(u2.reshape(-1).float())
            ops = {"x2": (X[parity], X[parity].bits().clone()), "u2": (Uu[parity], Uu[parity].bits().clone()),
                   "y": _copy(r, y), "lam": _copy(r, lam)}
            part, st = Guarded(2 * nblk, r.device), _state(r, 0, parity)
            rc = r.tv_iter(c.geo, _p(X[0]), _p(X[1]), _p(Uu[0]), _p(Uu[1]), _p(ops["y"][0]), _p(ops["lam"][0]), c.aniso, TAU,
                           tv_sigma(nd), RHO, 0.0, _p(part), _p(st))
            outs = {"x2'": X[1 - parity], "u2'": Uu[1 - parity], "partial": part}
            _written(tag, r, rc, outs, ops)
            assert st.guards_intact() and _state_of(st) == (0, parity + 1), f"{tag}: state {_state_of(st)}"
            return {k: g.bits().clone() for k, g in outs.items()}

        out = twice(tag, once)
        got = (_f(out["x2'"], x2.shape), _f(out["u2'"], u2.shape))
        for name, g, rf, m, b in zip(("x2'", "u2'"), got, ref, meas, step_bounds(c)):
            worst = max(worst, _ratio(f"{tag} {name}", g, rf, m, b))
    return worst


def run_tgv_step(r, c):
    (y, x2, r2, u2, l1, l2), ref, meas, _ = tgv_step_ref(c)
    n, nd = c.n, c.nd
    nblk = int(r.lib.dinv_tgv_cp_partials(n))
    assert nblk == grid_for(n), (nblk, grid_for(n))
    worst = 0.0
    for parity in (0, 1):
        tag = f"{c.id}-it{parity}"

        def once():
            sets = {}
            for name, t in (("x2", x2), ("r2", r2), ("u2", u2)):
                pair = [Guarded(t.numel(), r.device) for _ in range(2)]
                pair[parity].t.copy_(t.reshape(-1).float())
                sets[name] = pair
            ops = {k: (v[parity], v[parity].bits().clone()) for k, v in sets.items()}
            ops.update({"y": _copy(r, y), "lam1": _copy(r, l1), "lam2": _copy(r, l2)})
            z, w = Guarded(n, r.device), Guarded(n * nd, r.device)
            part, st = Guarded(2 * nblk, r.device), _state(r, 0, parity)
            rc = r.tgv_iter(c.geo, _p(sets["x2"][0]), _p(sets["x2"][1]), _p(sets["r2"][0]), _p(sets["r2"][1]), _p(sets["u2"][0]),
                            _p(sets["u2"][1]), _p(ops["y"][0]), _p(ops["lam1"][0]), _p(ops["lam2"][0]), TAU, tgv_sigma(nd), RHO,
                            0.0, _p(z), _p(w), _p(part), _p(st))
            outs = {"x2'": sets["x2"][1 - parity], "r2'": sets["r2"][1 - parity], "u2'": sets["u2"][1 - parity], "z": z, "w": w,
                    "partial": part}
            _written(tag, r, rc, outs, ops)
            assert st.guards_intact() and _state_of(st) == (0, parity + 1), f"{tag}: state {_state_of(st)}"
            return {k: g.bits().clone() for k, g in outs.items()}

        out = twice(tag, once)
        for name, rf, m, b in zip(("x2'", "r2'", "u2'", "z", "w"), ref, meas, step_bounds(c)):
            worst = max(worst, _ratio(f"{tag} {name}", _f(out[name], rf.shape), rf, m, b))
    return worst


# ---- the operators alone
def _operator(r, c, name, src, words, ref, measure, key):
    tag = f"{c.id} {name}"
    sb = _copy(r, src)

    def once():
        out = Guarded(words, r.device)
        rc = r.operator(name, c.geo, _p(sb[0]), _p(out))
        _written(tag, r, rc, {"out": out}, {"in": sb})
        return {"out": out.bits().clone()}

    return _ratio(tag, _f(twice(tag, once)["out"], ref.shape), ref, measure, BOUNDS[key][c.nd])


def run_tv_ops(r, c):
    g, nd = _gen(c), c.nd
    x = torch.randn(c.shape, generator=g, dtype=F64).float().double()
    v = torch.randn(*c.shape, nd, generator=g, dtype=F64).float().double()
    return max(_operator(r, c, "dinv_tv_nabla", x, c.n * nd, r_nabla(x), r_nabla(x.abs(), True), "nabla"),
               _operator(r, c, "dinv_tv_nabla_adjoint", v, c.n, r_nabla_adjoint(v), r_nabla_adjoint(v.abs(), True), "nabla_adjoint"))


def run_tgv_ops(r, c):
    g, nd = _gen(c), c.nd
    v = torch.randn(*c.shape, nd, generator=g, dtype=F64).float().double()
    u = torch.randn(*c.shape, nd * nd, generator=g, dtype=F64).float().double()
    return max(_operator(r, c, "dinv_tgv_epsilon", v, c.n * nd * nd, r_epsilon(v), r_epsilon(v.abs(), True), "epsilon"),
               _operator(r, c, "dinv_tgv_epsilon_adjoint", u, c.n * nd, r_epsilon_adjoint(u), r_epsilon_adjoint(u.abs(), True),
                         "epsilon_adjoint"))


def run_tv_grad(r, c):
    x = grad_image(c)
    ref, measure, _ = r_tv_grad_terms(x)
    return _operator(r, c, "dinv_tv_grad", x, c.n, ref, measure, "tv_grad")


def run_tv_fn(r, c):
    g, (nd, B) = _gen(c), c.geo[:2]
    x = torch.randn(c.shape, generator=g, dtype=F64).float().double()
    per = c.n // B
    nblk = int(r.lib.dinv_tv_fn_blocks(per))
    assert nblk == tv_fn_blocks(per), (nblk, tv_fn_blocks(per))
    xb = _copy(r, x)
    worst = 0.0
    for mode in (0, 1):
        tag = f"{c.id}-mode{mode}"

        def once():
            out, part = Guarded(B, r.device), Guarded(B * nblk, r.device)
            rc = r.tv_fn(c.geo, mode, _p(xb[0]), _p(out), _p(part))
            _written(tag, r, rc, {"out": out, "partial": part}, {"x": xb})
            return {"out": out.bits().clone(), "partial": part.bits().clone()}

        ref = r_tv_fn(x, mode)
        worst = max(worst, _ratio(tag, _f(twice(tag, once)["out"], ref.shape), ref, ref, tv_fn_bound(nd, mode, per)))
    # layout, exact: on integers in 0..4 every |Dx|_1 is an integer and a sample sums to less than 2^24 in any order, and a pixel
    # that is dropped or counted twice changes the sum, which the bound above cannot see among half a million terms
    xi = torch.randint(0, 5, c.shape, generator=g).double()
    xb, mode, tag = _copy(r, xi), 1, f"{c.id}-mode1-exact"
    want = r_tv_fn(xi, 1)
    assert float(want.max()) < 2 ** 24
    got = _f(twice(tag, once)["out"], want.shape)
    assert torch.equal(got, want), f"{tag}: {got.tolist()} for the exact {want.tolist()}"
    return worst


# ---- the stop
def _rel(got, ref):
    if float(ref.norm()) == 0:
        return float(got.abs().max())
    return float((got - ref).norm() / ref.norm())


def run_stop(r, c):
    """k + 1 + 4 launches enqueued with no host read but one synchronisation after k + 1, where the set that is not current is
    poisoned: state (1, k + 1), the current set the fp64 iterate, and not a word written by the four launches after the stop;
    and crit = 1: stops at (1, 3), the first iteration the rule tests"""
    y, lam, k, crit, rels = stop_plan(c)
    assert k, f"{c.id}: no k in 4..12 with a 1 % margin in {rels}"
    tgv = c.kind == "tgv-stop"
    n, nd = c.n, c.nd
    shapes = {"x2": c.shape, "r2": (*c.shape, nd), "u2": (*c.shape, nd * nd)} if tgv else {"x2": c.shape, "u2": (*c.shape, nd)}
    nblk = grid_for(n)
    l1, l2 = (0.1 * lam).float(), (0.15 * lam).float()
    for crit_run, want_it in ((crit, k + 1), (1.0, 3)):
        tag = f"{c.id}-crit{crit_run:.3g}"
        sets = {name: [Guarded(math.prod(s), r.device) for _ in range(2)] for name, s in shapes.items()}
        sets["x2"][0].t.copy_(y.reshape(-1).float())
        for name in shapes:
            if name != "x2":
                sets[name][0].t.zero_()
        yb, part, st = _copy(r, y), Guarded(2 * nblk, r.device), _state(r, 0, 0)
        if tgv:
            lb1, lb2, z, w = _copy(r, l1), _copy(r, l2), Guarded(n, r.device), Guarded(n * nd, r.device)
            scratch = {"z": z, "w": w, "partial": part}

            def launch():
                return r.tgv_iter(c.geo, _p(sets["x2"][0]), _p(sets["x2"][1]), _p(sets["r2"][0]), _p(sets["r2"][1]),
                                  _p(sets["u2"][0]), _p(sets["u2"][1]), _p(yb[0]), _p(lb1[0]), _p(lb2[0]), f32(0.01),
                                  tgv_sigma(nd), f32(1.99), crit_run, _p(z), _p(w), _p(part), _p(st))
        else:
            lb = _copy(r, lam)
            scratch = {"partial": part}

            def launch():
                return r.tv_iter(c.geo, _p(sets["x2"][0]), _p(sets["x2"][1]), _p(sets["u2"][0]), _p(sets["u2"][1]), _p(yb[0]),
                                 _p(lb[0]), c.aniso, f32(0.01), tv_sigma(nd), f32(1.99), crit_run, _p(part), _p(st))
        for _ in range(k + 1):
            rc = launch()
            assert rc == 0, f"{tag}: error {rc}: {r.err()}"
        r.sync()
        cur = want_it & 1
        for pair in sets.values():
            pair[cur ^ 1].full.fill_(POISON)
        before = {name: g.bits().clone() for name, g in scratch.items()}
        before.update({name: pair[cur].bits().clone() for name, pair in sets.items()})
        for _ in range(4):
            rc = launch()
            assert rc == 0, f"{tag}: error {rc}: {r.err()}"
        r.sync()
        assert _state_of(st) == (1, want_it), f"{tag}: state {_state_of(st)}, the fp64 sequence stops at (1, {want_it}): {rels}"
        for name, pair in sets.items():
            assert pair[cur ^ 1].untouched(), f"{tag}: a launch after the stop wrote into the {name} that is not current"
            assert pair[cur].guards_intact() and torch.equal(pair[cur].bits(), before[name]), f"{tag}: a launch after the stop changed {name}"
        for name, g in scratch.items():
            assert g.guards_intact() and torch.equal(g.bits(), before[name]), f"{tag}: a launch after the stop wrote {name}"
        assert st.guards_intact() and yb[0].guards_intact() and torch.equal(yb[0].bits(), yb[1])
        z0 = [torch.zeros(s, dtype=F64) for name, s in shapes.items() if name != "x2"]
        if tgv:
            ref = r_tgv_prox(y, lam.float().double(), y, *z0, want_it, 0.0)[:3]
            tols = (1e-5, 1e-5, 1e-4)
        else:
            ref = r_tv_prox(y, lam, y, *z0, want_it, 0.0, c.aniso)[:2]
            tols = (1e-5, 1e-4)
        for (name, pair), rf, tol in zip(sets.items(), ref, tols):
            e = _rel(_f(pair[cur].bits(), rf.shape), rf)
            print(f"{tag}: {name} after {want_it} iterations: relative error {e:.3g} (below {tol:g})")
            assert e < tol, f"{tag}: {name} is {e:.3g} from the fp64 iterate {want_it}"
    return 0.0


def run_case(r, c):
    """runs case c on runner r, asserts everything the module docstring lists and returns the worst |error| / bound"""
    return {"tv-step": run_tv_step, "tgv-step": run_tgv_step, "tv-ops": run_tv_ops, "tgv-ops": run_tgv_ops, "tv-grad": run_tv_grad,
            "tv-fn": run_tv_fn, "tv-stop": run_stop, "tgv-stop": run_stop}[c.kind](r, c)


# ------------------------------------------------------------------ refusals: non-zero status and not a word written
def run_rejections(r):
    dev = r.device
    nd2, nd3 = (2, 1, 1, 1, 4, 4), (3, 1, 1, 2, 4, 4)
    B = {k: Guarded(16 * 9 + 8, dev) for k in ("xa", "xb", "ra", "rb", "ua", "ub", "y", "lam", "lam2", "z", "w", "partial", "state", "out")}

    def refused(what, rc):
        r.sync()
        assert rc != 0, f"{what}: accepted"
        assert r.err(), f"{what}: no message"
        for name, g in B.items():
            assert g.untouched(), f"{what}: refused, but {name} was written"

    def tv(geo=nd2, aniso=0, **kw):
        a = {k: _p(B[k]) for k in ("xa", "xb", "ua", "ub", "y", "lam", "partial", "state")}
        a.update(kw)
        return r.tv_iter(geo, a["xa"], a["xb"], a["ua"], a["ub"], a["y"], a["lam"], aniso, TAU, 12.5, RHO, 0.0, a["partial"], a["state"])

    def tgv(geo=nd2, **kw):
        a = {k: _p(B[k]) for k in ("xa", "xb", "ra", "rb", "ua", "ub", "y", "lam", "lam2", "z", "w", "partial", "state")}
        a.update(kw)
        return r.tgv_iter(geo, a["xa"], a["xb"], a["ra"], a["rb"], a["ua"], a["ub"], a["y"], a["lam"], a["lam2"], TAU, 1.0, RHO,
                          0.0, a["z"], a["w"], a["partial"], a["state"])

    big_tv, big_tgv = (2, 1, 1, 1, 32768, 32768), (2, 1, 1, 1, 16384, 32768)      # n nd = 2^31; n nd^2 = 2^31
    big3_tv, big3_tgv = (3, 1, 1, 1024, 1024, 683), (3, 1, 1, 512, 683, 683)      # 3 n >= 2^31; 9 n >= 2^31
    assert 3 * 1024 * 1024 * 683 >= 2 ** 31 and 9 * 512 * 683 * 683 >= 2 ** 31
    bad_geo = {"nd = 1": (1, 1, 1, 1, 4, 4), "nd = 4": (4, 1, 1, 1, 4, 4), "D = 2 with nd = 2": (2, 1, 1, 2, 4, 4),
               "H = 0": (2, 1, 1, 1, 0, 4), "W = 0": (3, 1, 1, 2, 4, 0), "D = 0": (3, 1, 1, 0, 4, 4), "batch = 0": (2, 0, 1, 1, 4, 4),
               "channels = 0": (2, 1, 0, 1, 4, 4)}
    for what, geo in bad_geo.items():
        refused(f"tv_cp_iter {what}", tv(geo))
        refused(f"tgv_cp_iter {what}", tgv(geo))
        refused(f"tv_fn {what}", r.tv_fn(geo, 0, _p(B["xa"]), _p(B["out"]), _p(B["partial"])))
        for name in ("dinv_tv_nabla", "dinv_tv_nabla_adjoint", "dinv_tv_grad", "dinv_tgv_epsilon", "dinv_tgv_epsilon_adjoint"):
            refused(f"{name} {what}", r.operator(name, geo, _p(B["xa"]), _p(B["out"])))
    for geo in (big_tv, big3_tv):
        refused("tv_cp_iter n nd >= 2^31", tv(geo))
        refused("tv_fn n nd >= 2^31", r.tv_fn(geo, 0, _p(B["xa"]), _p(B["out"]), _p(B["partial"])))
        for name in ("dinv_tv_nabla", "dinv_tv_nabla_adjoint", "dinv_tv_grad"):
            refused(f"{name} n nd >= 2^31", r.operator(name, geo, _p(B["xa"]), _p(B["out"])))
    for geo in (big_tgv, big3_tgv):
        refused("tgv_cp_iter n nd^2 >= 2^31", tgv(geo))
        for name in ("dinv_tgv_epsilon", "dinv_tgv_epsilon_adjoint"):
            refused(f"{name} n nd^2 >= 2^31", r.operator(name, geo, _p(B["xa"]), _p(B["out"])))
    for geo in (nd2, nd3):
        for k in ("xa", "xb", "ua", "ub", "y", "lam", "partial", "state"):
            refused(f"tv_cp_iter null {k}", tv(geo, **{k: None}))
        for k in ("xa", "xb", "ra", "rb", "ua", "ub", "y", "lam", "lam2", "z", "w", "partial", "state"):
            refused(f"tgv_cp_iter null {k}", tgv(geo, **{k: None}))
        refused("tv_cp_iter xa == xb", tv(geo, xb=_p(B["xa"])))
        refused("tv_cp_iter ua == ub", tv(geo, ub=_p(B["ua"])))
        refused("tv_cp_iter xa == y", tv(geo, y=_p(B["xa"])))
        refused("tv_cp_iter xb == y", tv(geo, y=_p(B["xb"])))
        refused("tgv_cp_iter xa == xb", tgv(geo, xb=_p(B["xa"])))
        refused("tgv_cp_iter ra == rb", tgv(geo, rb=_p(B["ra"])))
        refused("tgv_cp_iter ua == ub", tgv(geo, ub=_p(B["ua"])))
        refused("tgv_cp_iter xa == y", tgv(geo, y=_p(B["xa"])))
        for name in ("dinv_tv_nabla", "dinv_tv_nabla_adjoint", "dinv_tv_grad", "dinv_tgv_epsilon", "dinv_tgv_epsilon_adjoint"):
            refused(f"{name} out == in", r.operator(name, geo, _p(B["xa"]), _p(B["xa"])))
            refused(f"{name} null in", r.operator(name, geo, None, _p(B["out"])))
            refused(f"{name} null out", r.operator(name, geo, _p(B["xa"]), None))
        refused("tv_fn null x", r.tv_fn(geo, 0, None, _p(B["out"]), _p(B["partial"])))
        refused("tv_fn null out", r.tv_fn(geo, 0, _p(B["xa"]), None, _p(B["partial"])))
        refused("tv_fn null partial", r.tv_fn(geo, 0, _p(B["xa"]), _p(B["out"]), None))
        for mode in (-1, 2):
            refused(f"tv_fn mode {mode}", r.tv_fn(geo, mode, _p(B["xa"]), _p(B["out"]), _p(B["partial"])))
    refused("tv_fn batch 65536", r.tv_fn((2, 65536, 1, 1, 1, 1), 0, _p(B["xa"]), _p(B["out"]), _p(B["partial"])))
    # the 16-byte records of the 2-D TGV fields: 8-byte aligned is not enough
    for k in ("ua", "ub", "ra", "rb", "w"):
        refused(f"tgv_cp_iter 2-D {k} + 8 bytes", tgv(nd2, **{k: _p(B[k], 8)}))
