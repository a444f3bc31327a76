"""Shared by tests/test_variational_kernels_gpu.py (the gfx950 library) and tests/test_emu_variational_cases.py (the same kernel
sources on the host emulation): the case table of csrc/elementwise.hip - the loop algebra of the iteration drivers (lincomb,
affine, the per-sample dot product, the CG updates and their device stop, the pointwise divisions of the closed-form proxes
and the pointwise likelihood operators) - per element against fp64 or, where the kernel restates a tensor expression of the
reference operation by operation, bit for bit against its fp32 evaluation on the CPU.  The runner calls the C entry points on
guarded buffers (tests/fft_cases.py Guarded), every call twice on fresh outputs with identical bits, operands unchanged.

Error measure, per element: |out - ref| <= c U M with U = 2^-24, M the expression on absolute values with every subtraction
an addition and c the number of fp32 roundings on the longest path, counted in BOUNDS.  The sizes are those at which a kernel
takes another path: below one float4 (the tail alone), a tail after whole float4s, one workgroup and one more, and a second
pass of the grid-stride loop with a ragged end above each launcher's cap on workgroups."""
from dataclasses import dataclass

import torch

from fft_cases import GUARD, POISON, Guarded

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
INF = float("inf")
POISSON_GRAD, POISSON_PROX, L1_GRAD, L1_PROX, LOGPOISSON_GRAD = range(5)      # include/deepinv_amd.h DINV_FID_*
DENORMALIZE = 1


def cdiv(a, b):
    return -(-a // b)


def f32(v):
    return float(torch.tensor(v, dtype=F32))


# ------------------------------------------------------------------ the launchers' grid rules, restated (csrc/elementwise.hip)
def stream_blocks(n):
    """workgroups of 256 lanes, a float4 each, of lincomb / affine / cg_update"""
    return min(max(cdiv(n // 4 + 1, 256), 1), 2048)


def dot_blocks(n):
    """dinv_batched_dot_blocks: four float4 per lane"""
    return min(max(cdiv(n // 4 + 1, 1024), 1), 256)


def pointwise_blocks(n):
    """cdiv_real / mask_solve / fidelity_pointwise: one element per lane"""
    return min(cdiv(n, 256), 2048)


# ------------------------------------------------------------------ the bounds: c of |out - ref| <= c U M, counted
# (and for the record the worst kernel error / bound on the MI355X over the table, as tests/test_variational_kernels_gpu.py prints it)
BOUNDS = {
    "lincomb": 3,               # fma(c, z, fma(b, y, fma(a, x, d))): one rounding per fma.  0.778 (lincomb-n2098355, y and z)
    "cg_update": 2,             # one fma on the fp32 scalar s_b restated on the host (two operations, counted as 2).  0.5
    "cdiv_real": 2,             # d + add, the division: relative, per component.  0.79 (cdiv-n525289-period525289: the worst of the table)
    # y / p0, x / p0, + p1, the quotient (4 on q); 1 - q; p0 *: against p0 (1 + q).  0.513 (fidelity-n525289, DENORMALIZE)
    "poisson_grad": 6,
    # c = 1 / (p0 gamma): 2; d = x - c: 3 on |x| + c; d d: 7; + 4 yd / gamma (2 on its own term): 8 on the radicand; the root
    # halves it and adds 1: 5; c *: 8; x -: 9 on |x| + c sqrt(.), and the exact halving
    "poisson_prox": 9,          # 0.276 (fidelity-n525289)
    # the rounded argument -p1 x moves exp by |p1 x| U <= 2 U (inputs below 4, p1 = 1/2); expf itself 1 ulp = 2 U (HIP math API
    # reference, "Single precision mathematical functions": expf, maximum error 1 ULP; the table is not shipped with the ROCm
    # installation, the host emulation calls the C library's, which is within 1 ulp as well); the difference, p0 p1, the product
    "logpoisson_grad": 2 + 2 + 3,       # 0.312 (fidelity-n525289)
}


def dot_bound(n):
    """the fma chain of one lane (4 per float4, ceil(n4 / lanes) float4s), 6 shuffle levels, 2 LDS levels, then the per-lane
    terms of the final kernel and its 6 shuffle levels: against sum |x| |y|.  (MI355X: 0.0488, dot-n4-b3)"""
    nblk = dot_blocks(n)
    return 4 * cdiv(n // 4, nblk * 256) + 6 + 2 + cdiv(nblk, 64) + 6


# ------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    kind: str                   # lincomb | dot | cg-update | cg-check | cdiv | mask-solve | fidelity
    n: int
    batch: int = 1
    period: int = 0
    emu: bool = True

    @property
    def id(self):
        return (f"{self.kind}-n{self.n}" + (f"-b{self.batch}" if self.batch > 1 else "")
                + (f"-period{self.period}" if self.period else ""))


STREAM_SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1027, 2048 * 1024 + 4 * 300 + 3]
CG_BIG = 2048 * 1024 + 4 * 300
POINTWISE_BIG = 524288 + 1001
# 262144 + 4 * 77 floats are 65 workgroups of dinv_batched_dot_blocks, every lane in its fourth or fifth float4: the cap of 256
# workgroups is reached from 4 * 255 * 1024 floats, so 4 * 262144 + 4 * 77 is in the table as well
DOT_SIZES = [4, 1024, 4100, 262144 + 4 * 77, 4 * 262144 + 4 * 77]
CHECK_BATCHES = [1, 63, 64, 65, 200]
FIDELITY_SIZES = [1, 255, 257, POINTWISE_BIG]

TABLE = ([Case("lincomb", n, emu=n < 10 ** 6) for n in STREAM_SIZES]
         + [Case("dot", n, 3, emu=n < 10 ** 6) for n in DOT_SIZES]
         + [Case("cg-update", n, 3) for n in STREAM_SIZES if n % 4 == 0] + [Case("cg-update", CG_BIG, 2, emu=False)]
         + [Case("cg-check", 0, b) for b in CHECK_BATCHES]
         + [Case(k, POINTWISE_BIG, period=p) for k in ("cdiv", "mask-solve") for p in (3 * 37 * 11, POINTWISE_BIG)]
         + [Case(k, 700, period=p) for k in ("cdiv", "mask-solve") for p in (3 * 37, 700)]
         + [Case("fidelity", n, emu=n < 10 ** 5) for n in FIDELITY_SIZES])
assert len({c.id for c in TABLE}) == len(TABLE), "duplicate case ids"


def strided(c):
    """(work items of the case's widest launch, lanes of its capped grid): the case reaches a second pass of the grid-stride
    loop with a ragged end when the first exceeds the second and is no multiple of 256"""
    if c.kind in ("lincomb", "cg-update"):
        return c.n // 4, stream_blocks(c.n) * 256
    if c.kind == "dot":
        return c.n // 4, dot_blocks(c.n) * 1024
    return c.n, pointwise_blocks(c.n) * 256


# ------------------------------------------------------------------ the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.elementwise), `device` of its
    buffers, `stream()` -> the stream argument"""

    def __init__(self, lib, device, stream):
        self.lib, self.device, self._stream = lib, torch.device(device), stream

    def err(self):
        return self.lib.dinv_last_error().decode()

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def lincomb(self, n, a, x, b, y, c, z, out):
        return self.lib.dinv_lincomb(n, a, x, b, y, c, z, out, self._stream())

    def affine(self, n, a, x, b, y, c, z, d, lo, hi, out):
        return self.lib.dinv_affine(n, a, x, b, y, c, z, d, lo, hi, out, self._stream())

    def dot(self, batch, n, x, y, out, partial):
        return self.lib.dinv_batched_dot(batch, n, x, y, out, partial, self._stream())

    def cg_update(self, mode, batch, n, num, den, eps, v0, v1, w0, w1, done=False):
        if done is False:
            return self.lib.dinv_cg_update(mode, batch, n, num, den, eps, v0, v1, w0, w1, self._stream())
        return self.lib.dinv_cg_update_masked(mode, batch, n, num, den, eps, v0, v1, w0, w1, done, self._stream())

    def cg_check(self, batch, res, tol2, done):
        return self.lib.dinv_cg_check(batch, res, tol2, done, self._stream())

    def cdiv_real(self, n, period, s, d, add, out):
        return self.lib.dinv_cdiv_real(n, period, s, d, add, out, self._stream())

    def mask_solve(self, mode, n, period, x, m, add, out):
        return self.lib.dinv_mask_solve(mode, n, period, x, m, add, out, self._stream())

    def fidelity(self, op, n, x, y, p0, p1, gamma, flags, out):
        return self.lib.dinv_fidelity_pointwise(op, n, x, y, p0, p1, gamma, flags, out, self._stream())


def _seed(cid):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(cid)) % (2 ** 31)


def _gen(c):
    return torch.Generator().manual_seed(_seed(c.id))


def _p(g, off_bytes=0):
    return None if g is None else g.t.data_ptr() + off_bytes


def _copy(r, t):
    """a guarded device copy of the fp32 (or int32) tensor t, and its bits"""
    g = Guarded(t.numel(), r.device)
    if t.dtype == torch.int32:
        g.full[GUARD:GUARD + t.numel()] = t.reshape(-1).to(r.device)
    else:
        g.t.copy_(t.reshape(-1).float())
    return g, g.bits().clone()


def _ints(g):
    return g.full[GUARD:GUARD + g.n].cpu()


def _floats(bits):
    return bits.view(F32)


def _intact(tag, operands):
    for name, (g, before) in operands.items():
        assert g.guards_intact() and torch.equal(g.bits(), before), f"{tag}: the call modified {name}"


def _ok(tag, r, rc, outs, operands, poison_check=True):
    assert rc == 0, f"{tag}: error {rc}: {r.err()}"
    r.sync()
    for name, g in outs.items():
        assert g.guards_intact(), f"{tag}: write outside {name}"
        if poison_check:
            bad = g.bits() == POISON
            assert not bool(bad.any()), f"{tag}: {int(bad.sum())} words of {name} hold the guard pattern: never written, or read from outside"
    _intact(tag, operands)


def twice(tag, once):
    a, b = once(), once()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{tag}: two identical calls differ in {k}"
    return a


def _ratio(tag, got, ref, measure, c):
    got, ref, measure = got.reshape(-1).double(), ref.reshape(-1), measure.reshape(-1)
    assert not bool(torch.isnan(got).any()), f"{tag}: NaN in the result"
    err, bound = (got - ref).abs(), c * U * measure
    zero = bound == 0
    assert bool((err[zero] == 0).all()), f"{tag}: an element with a zero measure is not exact"
    ratio = torch.where(zero, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst, at = float(ratio.max()), int(ratio.argmax())
    print(f"{tag}: worst element {at} error / bound {worst:.3g} ({worst * c:.3g} U against c = {c})")
    assert worst <= 1.0, f"{tag}: element {at} is {worst:.3g} times its bound of {c} U M"
    return worst


def _same(tag, got, want):
    """bit for bit, a NaN for a NaN"""
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{tag}: NaN at other places: first at {int((gn != wn).nonzero()[0])}"
    diff = (got.view(torch.int32) != want.view(torch.int32)) & ~gn
    assert not bool(diff.any()), (f"{tag}: {int(diff.sum())} of {diff.numel()} elements differ from the fp32 CPU expression, the first at "
                                  f"{int(diff.nonzero()[0])}: {float(got[diff][0])!r} for {float(want[diff][0])!r}")


# ---- lincomb / affine
def run_lincomb(r, c):
    g, n = _gen(c), c.n
    x, y, z = (torch.randn(n, generator=g) for _ in range(3))
    a, b, cc, d, lo, hi = f32(0.75), f32(-1.3), f32(2.1), f32(0.4), f32(-0.5), f32(0.8)
    bufs = {"x": _copy(r, x), "y": _copy(r, y), "z": _copy(r, z)}
    xd, yd, zd = x.double(), y.double(), z.double()
    worst = 0.0

    def call(tag, fn, operands=bufs, poison_check=True):
        def once():
            out = Guarded(n, r.device)
            rc = fn(_p(out))
            _ok(tag, r, rc, {"out": out}, operands, poison_check)
            return {"out": out.bits().clone()}
        return _floats(twice(tag, once)["out"])

    for has_y in (0, 1):
        for has_z in (0, 1):
            tag = f"{c.id}" + ("-y" if has_y else "") + ("-z" if has_z else "")
            py, pz = _p(bufs["y"][0]) if has_y else None, _p(bufs["z"][0]) if has_z else None
            ref = a * xd + (b * yd if has_y else 0) + (cc * zd if has_z else 0)
            M = abs(a) * xd.abs() + (abs(b) * yd.abs() if has_y else 0) + (abs(cc) * zd.abs() if has_z else 0)
            got = call(f"{tag} lincomb", lambda o: r.lincomb(n, a, _p(bufs["x"][0]), b, py, cc, pz, o))
            worst = max(worst, _ratio(f"{tag} lincomb", got, ref, M, BOUNDS["lincomb"]))
            free = call(f"{tag} affine", lambda o: r.affine(n, a, _p(bufs["x"][0]), b, py, cc, pz, d, -INF, INF, o))
            worst = max(worst, _ratio(f"{tag} affine", free, ref + d, M + abs(d), BOUNDS["lincomb"]))
            clamped = call(f"{tag} affine clamped", lambda o: r.affine(n, a, _p(bufs["x"][0]), b, py, cc, pz, d, lo, hi, o))
            assert torch.equal(clamped, torch.clamp(free, lo, hi)), f"{tag}: the clamped result is not the clamp of the free one"
            if n >= 1023:
                assert bool((clamped == lo).any()) and bool((clamped == hi).any()) and bool(((clamped > lo) & (clamped < hi)).any())
    # NaN in, NaN out at the same places, and the other places as without them (y and z present: the last pass of the loop)
    clean = {"lincomb": got, "affine clamped": clamped}
    xn, yn = x.clone(), y.clone()
    xn[3 % n::7] = float("nan")
    yn[5 % n::11] = float("nan")
    nb = {"x": _copy(r, xn), "y": _copy(r, yn), "z": bufs["z"]}
    want = torch.isnan(xn) | torch.isnan(yn)
    for name, fn in (("lincomb", lambda o: r.lincomb(n, a, _p(nb["x"][0]), b, _p(nb["y"][0]), cc, _p(nb["z"][0]), o)),
                     ("affine clamped", lambda o: r.affine(n, a, _p(nb["x"][0]), b, _p(nb["y"][0]), cc, _p(nb["z"][0]), d, lo, hi, o))):
        out = call(f"{c.id} NaN {name}", fn, nb, poison_check=False)
        assert torch.equal(torch.isnan(out), want), f"{c.id} {name}: NaN in at {want.nonzero().flatten().tolist()[:8]}, NaN out elsewhere"
        assert torch.equal(out[~want].view(torch.int32), clean[name][~want].view(torch.int32)), f"{c.id} {name}: a NaN moved its neighbours"
    return worst


# ---- batched dot
def run_dot(r, c):
    g, B, n = _gen(c), c.batch, c.n
    x, y = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    nblk = int(r.lib.dinv_batched_dot_blocks(n))
    assert nblk == dot_blocks(n), (nblk, dot_blocks(n))
    ops = {"x": _copy(r, x), "y": _copy(r, y)}

    def once():
        out, part = Guarded(B, r.device), Guarded(B * nblk, r.device)
        rc = r.dot(B, n, _p(ops["x"][0]), _p(ops["y"][0]), _p(out), _p(part))
        _ok(c.id, r, rc, {"out": out, "partial": part}, ops)
        return {"out": out.bits().clone(), "partial": part.bits().clone()}

    got = _floats(twice(c.id, once)["out"])
    xd, yd = x.double(), y.double()
    worst = _ratio(c.id, got, (xd * yd).sum(1), (xd.abs() * yd.abs()).sum(1), dot_bound(n))
    # layout, exact: operands of +-1 sum without rounding in any order (n < 2^24), and an element that is dropped or counted
    # twice changes the sum, which the bound above cannot see among a million terms
    x, y = (torch.randint(0, 2, (B, n), generator=g).float() * 2 - 1 for _ in range(2))
    ops = {"x": _copy(r, x), "y": _copy(r, y)}
    got = _floats(twice(f"{c.id} exact", once)["out"])
    want = (x.long() * y.long()).sum(1)
    assert n < 2 ** 24 and torch.equal(got.long(), want) and torch.equal(got, want.float()), f"{c.id}: {got.tolist()} for the exact {want.tolist()}"
    return worst


# ---- CG updates
def run_cg_update(r, c):
    g, B, n = _gen(c), c.batch, c.n
    num = torch.tensor([1.5, -0.02, 300.0][:B])
    den = torch.tensor([0.5, 4.0, -0.007][:B])
    eps = f32(1e-8)
    s = (num / (den + torch.tensor(eps))).double().view(B, 1)       # the kernel's num[b] / (den[b] + eps), in fp32
    worst = 0.0
    for mode in (0, 1):
        v0, v1, w0, w1 = (torch.randn(B, n, generator=g) for _ in range(4))
        ro = {"num": _copy(r, num), "den": _copy(r, den), "w0": _copy(r, w0)}
        if mode == 0:
            ro["w1"] = _copy(r, w1)
        for done_flag in (False, 0, 1):
            tag = f"{c.id}-mode{mode}" + ("" if done_flag is False else f"-masked-done{done_flag}")
            ops = dict(ro)
            if done_flag is not False:
                ops["done"] = _copy(r, torch.tensor([done_flag], dtype=torch.int32))

            def once():
                b0, b1 = _copy(r, v0)[0], (_copy(r, v1)[0] if mode == 0 else None)
                rc = r.cg_update(mode, B, n, _p(ro["num"][0]), _p(ro["den"][0]), eps, _p(b0), _p(b1), _p(ro["w0"][0]),
                                 _p(ro["w1"][0]) if mode == 0 else None, False if done_flag is False else _p(ops["done"][0]))
                outs = {"v0": b0, "v1": b1} if mode == 0 else {"v0": b0}
                _ok(tag, r, rc, outs, ops)
                return {k: o.bits().clone() for k, o in outs.items()}

            got = {k: _floats(v).view(B, n) for k, v in twice(tag, once).items()}
            if done_flag is False:
                plain = got
                a, b = (v0.double(), w0.double()) if mode == 0 else (w0.double(), v0.double())
                worst = max(worst, _ratio(f"{tag} v0", got["v0"], a + s * b, a.abs() + s.abs() * b.abs(), BOUNDS["cg_update"]))
                if mode == 0:
                    a, b = v1.double(), w1.double()
                    worst = max(worst, _ratio(f"{tag} v1", got["v1"], a - s * b, a.abs() + s.abs() * b.abs(), BOUNDS["cg_update"]))
            elif done_flag == 0:
                for k in got:
                    assert torch.equal(got[k].view(torch.int32), plain[k].view(torch.int32)), f"{tag}: {k} differs from dinv_cg_update"
            else:
                for k, before in (("v0", v0), ("v1", v1)):
                    if k in got:
                        assert torch.equal(got[k].view(torch.int32), before.view(torch.int32)), f"{tag}: {k} was written after the stop"
    return worst


def run_cg_check(r, c):
    batch = c.batch
    tol2 = torch.rand(batch, generator=_gen(c)) + 0.5
    below = tol2 * 0.5

    def check(tag, res, done_in, want):
        ops = {"res": _copy(r, res), "tol2": _copy(r, tol2)}

        def once():
            done = _copy(r, torch.tensor([done_in], dtype=torch.int32))[0]
            rc = r.cg_check(batch, _p(ops["res"][0]), _p(ops["tol2"][0]), _p(done))
            _ok(tag, r, rc, {"done": done}, ops)
            assert int(_ints(done)[0]) == want, f"{tag}: done = {int(_ints(done)[0])}, expected {want}"
            return {"done": done.bits().clone()}
        twice(tag, once)

    check(f"{c.id} all below", below, 0, 1)
    for at in sorted({0, 63, 64, batch - 1}):
        if at < batch:
            for what, v in (("above", tol2[at] * 2), ("equal", tol2[at]), ("NaN", torch.tensor(float("nan")))):
                res = below.clone()
                res[at] = v
                check(f"{c.id} sample {at} {what}", res, 0, 0)
                check(f"{c.id} sample {at} {what}, done already", res, 1, 1)
    return 0.0


# ---- the pointwise divisions
def _period_index(n, period):
    return torch.arange(n) % period


def run_cdiv(r, c):
    g, n, period = _gen(c), c.n, c.period
    s = torch.randn(n, 2, generator=g)
    d = torch.rand(period, generator=g) + 0.05
    add = f32(1.0 / 7e5)
    ops = {"s": _copy(r, s), "d": _copy(r, d)}

    def once():
        out = Guarded(2 * n, r.device)
        rc = r.cdiv_real(n, period, _p(ops["s"][0]), _p(ops["d"][0]), add, _p(out))
        _ok(c.id, r, rc, {"out": out}, ops)
        return {"out": out.bits().clone()}

    bits = twice(c.id, once)["out"]
    inplace = _copy(r, s)[0]
    rc = r.cdiv_real(n, period, _p(inplace), _p(ops["d"][0]), add, _p(inplace))
    _ok(f"{c.id} in place", r, rc, {"s": inplace}, {"d": ops["d"]})
    assert torch.equal(inplace.bits(), bits), f"{c.id}: in place differs"
    ref = s.double() / (d.double()[_period_index(n, period)] + add).view(n, 1)
    return _ratio(c.id, _floats(bits), ref, ref.abs(), BOUNDS["cdiv_real"])


def run_mask_solve(r, c):
    g, n, period = _gen(c), c.n, c.period
    x = torch.randn(n, generator=g)
    m = (torch.rand(period, generator=g) > 0.4).float() * (0.5 + torch.rand(period, generator=g))
    m[7], m[9], m[11] = 5e-6, 1e-5, 1.0000001e-5 * 1.001        # below, at (not above: 0) and above the threshold of A_dagger
    add = f32(1 / 0.37)
    ops = {"x": _copy(r, x), "m": _copy(r, m)}
    mm = m[_period_index(n, period)]
    # the reference's tensor expressions in fp32 on the CPU (forward.py:1223-1252), as tests/test_elementwise_gpu.py has them
    want = {0: x / (mm * mm + torch.tensor(add)), 1: x * torch.where(mm > torch.tensor(1e-5), mm.reciprocal(), torch.zeros(()))}
    assert float(want[1][9]) == 0.0 and float(want[1][7]) == 0.0 and float(want[1][11]) != 0.0
    for mode in (0, 1):
        tag = f"{c.id}-mode{mode}"

        def once():
            out = Guarded(n, r.device)
            rc = r.mask_solve(mode, n, period, _p(ops["x"][0]), _p(ops["m"][0]), add, _p(out))
            _ok(tag, r, rc, {"out": out}, ops)
            return {"out": out.bits().clone()}

        _same(tag, _floats(twice(tag, once)["out"]), want[mode])
    return 0.0


# ---- the pointwise likelihood operators
def run_fidelity(r, c):
    g, n = _gen(c), c.n
    worst = 0.0

    def call(tag, op, x, y, p0, p1, gamma, flags):
        ops = {"x": _copy(r, x), "y": _copy(r, y)}

        def once():
            out = Guarded(n, r.device)
            rc = r.fidelity(op, n, _p(ops["x"][0]), _p(ops["y"][0]), p0, p1, gamma, flags, _p(out))
            _ok(tag, r, rc, {"out": out}, ops, poison_check=False)
            return {"out": out.bits().clone()}
        return _floats(twice(tag, once)["out"])

    # L1: exact eighths so that d = 0, d = +-gamma, +-0 and NaN are met exactly; compared with torch on the CPU bit for bit
    gamma = 0.25
    y = torch.randint(-8, 9, (n,), generator=g).float() / 8
    x = y + torch.randint(-4, 5, (n,), generator=g).float() / 8         # d in {-1/2, ..., 1/2}: 0 and +-gamma among them
    special = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (float("nan"), 0.5), (0.5, float("nan")), (0.75, 0.5), (0.25, 0.5),
               (0.5, 0.5)]
    for i, (xv, yv) in enumerate(special[:n] if n < len(special) else special):
        x[(i * 29) % n], y[(i * 29) % n] = xv, yv
    got = call(f"{c.id} l1-grad", L1_GRAD, x, y, 1.0, 0.0, gamma, 0)
    # (torch.sign of a NaN is 0; the kernel passes the NaN on, as tests/test_emu_poisson.py requires: a diverged iterate stays visible)
    d = x - y
    _same(f"{c.id} l1-grad", got, torch.where(torch.isnan(d), d, torch.sign(d)))
    got = call(f"{c.id} l1-prox", L1_PROX, x, y, 1.0, 0.0, gamma, 0)
    _same(f"{c.id} l1-prox", got, torch.nn.functional.softshrink(x - y, gamma) + y)
    # Poisson and log-Poisson: x / p0 + p1 > 0
    x = torch.rand(n, generator=g) * 3.9 + 0.05
    y = torch.rand(n, generator=g) * 3.9
    p0, p1, gm = f32(0.7), f32(0.05), f32(0.6)
    xd, yd = x.double(), y.double()
    for flags in (0, DENORMALIZE):
        yy = yd / p0 if flags else yd
        q = yy / (xd / p0 + p1)
        got = call(f"{c.id} poisson-grad-flags{flags}", POISSON_GRAD, x, y, p0, p1, 1.0, flags)
        worst = max(worst, _ratio(f"{c.id} poisson-grad-flags{flags}", got, p0 * (1 - q), p0 * (1 + q), BOUNDS["poisson_grad"]))
        cc = 1 / (p0 * gm)
        ref = (xd - cc * torch.sqrt((xd - cc) ** 2 + 4 * yy / gm)) / 2
        M = (xd + cc * torch.sqrt((xd + cc) ** 2 + 4 * yy / gm)) / 2
        got = call(f"{c.id} poisson-prox-flags{flags}", POISSON_PROX, x, y, p0, 0.0, gm, flags)
        worst = max(worst, _ratio(f"{c.id} poisson-prox-flags{flags}", got, ref, M, BOUNDS["poisson_prox"]))
    n0, mu = f32(1.3), 0.5
    got = call(f"{c.id} logpoisson-grad", LOGPOISSON_GRAD, x, y, n0, mu, 1.0, 0)
    ey, ex = torch.exp(-mu * yd), torch.exp(-mu * xd)
    worst = max(worst, _ratio(f"{c.id} logpoisson-grad", got, n0 * mu * (ey - ex), n0 * mu * (ey + ex), BOUNDS["logpoisson_grad"]))
    return worst


def run_case(r, c):
    """runs case c on runner r and returns the worst |error| / bound (0 for the cases that are exact)"""
    return {"lincomb": run_lincomb, "dot": run_dot, "cg-update": run_cg_update, "cg-check": run_cg_check, "cdiv": run_cdiv,
            "mask-solve": run_mask_solve, "fidelity": run_fidelity}[c.kind](r, c)


# ------------------------------------------------------------------ refusals: non-zero status and not a word written
def run_rejections(r):
    n = 64
    B = {k: Guarded(3 * n + 8, r.device) for k in ("x", "y", "z", "out", "v1", "w1", "num", "den", "partial", "done")}
    P = {k: _p(g) for k, g in B.items()}

    def refused(what, rc):
        r.sync()
        assert rc != 0, f"{what}: accepted"
        assert r.err(), f"{what}: no message"
        for name, g in B.items():
            assert g.untouched(), f"{what}: refused, but {name} was written"

    refused("affine lo > hi", r.affine(n, 1.0, P["x"], 0.0, None, 0.0, None, 0.0, 1.0, 0.5, P["out"]))
    refused("lincomb n < 0", r.lincomb(-1, 1.0, P["x"], 0.0, None, 0.0, None, P["out"]))
    refused("lincomb null x", r.lincomb(n, 1.0, None, 0.0, None, 0.0, None, P["out"]))
    refused("lincomb null out", r.lincomb(n, 1.0, P["x"], 0.0, None, 0.0, None, None))
    for off in (4, 8, 12):
        refused(f"lincomb x + {off}", r.lincomb(n, 1.0, P["x"] + off, 1.0, P["y"], 1.0, P["z"], P["out"]))
        refused(f"lincomb y + {off}", r.lincomb(n, 1.0, P["x"], 1.0, P["y"] + off, 1.0, P["z"], P["out"]))
        refused(f"lincomb z + {off}", r.lincomb(n, 1.0, P["x"], 1.0, P["y"], 1.0, P["z"] + off, P["out"]))
        refused(f"lincomb out + {off}", r.lincomb(n, 1.0, P["x"], 1.0, P["y"], 1.0, P["z"], P["out"] + off))
        refused(f"affine out + {off}", r.affine(n, 1.0, P["x"], 0.0, None, 0.0, None, 0.0, -INF, INF, P["out"] + off))
        refused(f"batched_dot x + {off}", r.dot(3, n, P["x"] + off, P["y"], P["out"], P["partial"]))
        refused(f"batched_dot y + {off}", r.dot(3, n, P["x"], P["y"] + off, P["out"], P["partial"]))
        for done in (False, P["done"]):
            for mode in (0, 1):
                refused(f"cg_update mode {mode} v0 + {off}", r.cg_update(mode, 3, n, P["num"], P["den"], 0.0, P["x"] + off, P["v1"], P["y"], P["w1"], done))
                refused(f"cg_update mode {mode} w0 + {off}", r.cg_update(mode, 3, n, P["num"], P["den"], 0.0, P["x"], P["v1"], P["y"] + off, P["w1"], done))
            refused(f"cg_update mode 0 v1 + {off}", r.cg_update(0, 3, n, P["num"], P["den"], 0.0, P["x"], P["v1"] + off, P["y"], P["w1"], done))
            refused(f"cg_update mode 0 w1 + {off}", r.cg_update(0, 3, n, P["num"], P["den"], 0.0, P["x"], P["v1"], P["y"], P["w1"] + off, done))
    for bad in (1, 2, 3, 62):
        refused(f"batched_dot n = {bad}", r.dot(3, bad, P["x"], P["y"], P["out"], P["partial"]))
        for done in (False, P["done"]):
            for mode in (0, 1):
                refused(f"cg_update n = {bad}", r.cg_update(mode, 3, bad, P["num"], P["den"], 0.0, P["x"], P["v1"], P["y"], P["w1"], done))
    refused("batched_dot batch 65536", r.dot(65536, 4, P["x"], P["y"], P["out"], P["partial"]))
    refused("batched_dot null partial", r.dot(3, n, P["x"], P["y"], P["out"], None))
    for done in (False, P["done"]):
        refused("cg_update batch 65536", r.cg_update(1, 65536, 4, P["num"], P["den"], 0.0, P["x"], None, P["y"], None, done))
        refused("cg_update mode 2", r.cg_update(2, 3, n, P["num"], P["den"], 0.0, P["x"], P["v1"], P["y"], P["w1"], done))
        refused("cg_update mode 0 without v1", r.cg_update(0, 3, n, P["num"], P["den"], 0.0, P["x"], None, P["y"], P["w1"], done))
        refused("cg_update mode 0 without w1", r.cg_update(0, 3, n, P["num"], P["den"], 0.0, P["x"], P["v1"], P["y"], None, done))
        refused("cg_update null num", r.cg_update(1, 3, n, None, P["den"], 0.0, P["x"], None, P["y"], None, done))
    refused("cg_update_masked null done", r.cg_update(1, 3, n, P["num"], P["den"], 0.0, P["x"], None, P["y"], None, None))
    refused("cg_check null done", r.cg_check(3, P["x"], P["y"], None))
    for period in (0, -3):
        refused(f"cdiv_real period {period}", r.cdiv_real(n, period, P["x"], P["y"], 0.0, P["out"]))
        for mode in (0, 1):
            refused(f"mask_solve period {period}", r.mask_solve(mode, n, period, P["x"], P["y"], 0.0, P["out"]))
    refused("cdiv_real s + 4", r.cdiv_real(n, 8, P["x"] + 4, P["y"], 0.0, P["out"]))
    refused("cdiv_real out + 4", r.cdiv_real(n, 8, P["x"], P["y"], 0.0, P["out"] + 4))
    refused("mask_solve mode 2", r.mask_solve(2, n, 8, P["x"], P["y"], 0.0, P["out"]))
    for op in (-1, 5):
        refused(f"fidelity op {op}", r.fidelity(op, n, P["x"], P["y"], 1.0, 0.0, 1.0, 0, P["out"]))
    for flags in (2, 3, -1):
        refused(f"fidelity flags {flags}", r.fidelity(L1_GRAD, n, P["x"], P["y"], 1.0, 0.0, 1.0, flags, P["out"]))
    refused("fidelity null out", r.fidelity(L1_GRAD, n, P["x"], P["y"], 1.0, 0.0, 1.0, 0, None))
