"""Shared by tests/test_emu_hadamard.py and tests/test_emu_operator_cases.py (the kernel sources of csrc/hadamard.hip on the host
emulation) and by tests/test_operator_kernels_gpu.py (the gfx950 library): the case table of the Walsh-Hadamard kernels, the
operator table of SinglePixelCamera (deepinv/physics/singlepixel.py:408-439 with deepinv/physics/forward.py:1080-1117,
1212-1252), their float64 restatement (an fp64 butterfly, H_H x H_W / sqrt(H W) in natural order), the Python restatement of
run()'s choice of kernel form as a function of the compute-unit count, and the runner that calls dinv_hadamard and
dinv_hadamard_apply on guarded buffers (tests/fft_cases.py Guarded).

The bound against fp64 is the worst-case rounding of the arithmetic, not a measured figure: a transform over L index bits is L
rounded additions per output, each relative 2^-24, and the scale, the symbol's products and its division add at most four
more, so the l2 error of one transform is at most (L + 4) 2^-24 of the l2 norm of what it transforms, and of an operator with
two transforms twice that.

run_case applies it per plane.  The rounding of a transform is relative to the norm of the plane it transforms, and a symbol s
applied after it scales that error by at most max |s| over the plane, so the error of a plane of  s H2(x)  or  H2(s H2(x))  is
measured against  max_plane |s| ||x_plane||  - which is the norm of the result when s = 1, and stays the right measure when a
mask leaves a few small coefficients of a plane (a 2 x 2 plane with one open pixel), where the norm of the result is no measure
of the rounding that went into it.  For H2(s y) it is ||s y||, for prox_l2 the larger of ||z|| and the norm of the symbol's
value.  A plane whose measure is zero must be zero exactly."""
import ctypes
from dataclasses import dataclass, field

import torch

from fft_cases import POISON, Guarded

PRE = lambda m: m
SYM = lambda m: m << 4
SECOND, NO_TRANSFORM, LAST_AXIS, NO_NORMALIZE = 0x100, 0x200, 0x400, 0x800
RESIDENT_LOG2 = lambda c: c << 16
U = 2.0 ** -24
TILE_LOG2, MAX_THREADS = 14, 512
EMU_CUS = 16                      # what the emulation's hipDeviceGetAttribute reports


# ---------------------------------------------------------------- float64 restatement
def fwht(v):
    """the un-normalised natural-order (Sylvester) Walsh-Hadamard transform of the last axis, a butterfly in float64"""
    shape, n = v.shape, v.shape[-1]
    v = v.double().reshape(-1, n).clone()
    h = 1
    while h < n:
        w = v.view(-1, n // (2 * h), 2, h)
        a, b = w[:, :, 0], w[:, :, 1]
        d = a - b
        a += b
        b.copy_(d)
        h *= 2
    return v.view(shape)


def r_h2(x):
    H, W = x.shape[-2:]
    return fwht(x.reshape(*x.shape[:-2], H * W)).view(x.shape) / (H * W) ** 0.5


def r_last(x):
    """the last axis only, un-normalised"""
    return fwht(x)


def r_inv(m):
    return torch.where(m > 1e-5, 1 / m, torch.zeros_like(m))


def rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-300))


def bits(H, W):
    return (H * W).bit_length() - 1


def make(shape, seed, mask_batch=False, binary=True):
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    x = torch.randn(shape, generator=g)
    y = torch.randn(shape, generator=g)
    mshape = (B if mask_batch else 1, C, H, W)
    if binary:
        mask = (torch.rand(mshape, generator=g) < 0.4).float()
    else:
        mask = torch.rand(mshape, generator=g) * (torch.rand(mshape, generator=g) < 0.7).float()
    return x, y, mask


# (shape [B,C,H,W], resident-limit override or 0).  Resident: the smallest plane, thin planes both ways, groups of 32x32
# planes with a partial last group (35 planes over groups of 2), groups of 2x2 planes with a partial last group, the largest
# resident plane.  Two-pass (planes above 2^c floats): the smallest (8 floats over chunks of 4), rectangular both ways, a strip
# narrower than a chunk (c = 8 with 64 rows: strips of 256 -> 2^14 / 64), P > 1.
RESIDENT = [((1, 3, 2, 2), 0), ((2, 1, 2, 64), 0), ((2, 1, 64, 2), 0), ((5, 7, 32, 32), 0), ((67, 3, 2, 2), 0),
            ((1, 1, 128, 128), 0), ((1, 2, 16, 64), 0)]
TWO_PASS = [((1, 1, 2, 4), 2), ((1, 3, 8, 8), 4), ((2, 1, 4, 32), 3), ((1, 2, 32, 4), 5), ((1, 1, 128, 128), 8),
            ((2, 1, 64, 64), 11)]
CASES = RESIDENT + TWO_PASS
IDS = [f"{'x'.join(map(str, s))}-c{c}" for s, c in CASES]


# ---------------------------------------------------------------- run()'s choice of form, restated
def cdiv(a, b):
    return -(-a // b)


def form(planes, l, tbits, c, cus, second=False):
    """what run() of csrc/hadamard.hip launches for `planes` planes of 2^l floats with the butterflies of the bits below tbits,
    resident chunks of up to 2^c floats (0: the default) and `cus` compute units: passes (1 resident, 2 two-pass), g (log2 of the
    planes per workgroup), nt (floats per tile of the first launch), rl (log2 of the rows of the strip pass) and, per launch,
    the tiles and the threads"""
    c = c or TILE_LOG2
    total = planes << l
    threads = lambda nt: min(MAX_THREADS, max(64, nt // 16))
    if tbits <= c:
        g = 12 - l if l < 12 else 0
        while g > 0 and cdiv(planes, 1 << g) < cus:
            g -= 1
        if l + g < 2:
            g = 2 - l
        nt = 1 << (min(l, c) + g)
        return dict(passes=1, g=g, nt=nt, rl=0, tiles=[cdiv(total, nt)], threads=[threads(nt)])
    rl = l - c
    wd = min(TILE_LOG2 - rl, c)
    lo, hi = (total >> c, threads(1 << c)), (planes << (c - wd), threads(1 << (wd + rl)))
    seq = [lo, hi, lo] if second else [lo, hi]
    return dict(passes=2, g=0, nt=1 << c, rl=rl, tiles=[t for t, _ in seq], threads=[t for _, t in seq])


# ---------------------------------------------------------------- the case table
@dataclass(frozen=True)
class Case:
    id: str
    P: int
    H: int
    W: int
    c: int = 0                  # DINV_HAD_RESIDENT_LOG2 override
    masks: tuple = ()           # (binary, mask planes) variants of the operator table; empty: no operator table
    plain: bool = True          # the 2-D transform
    last: bool = True           # the last-axis transform
    emu: bool = True
    expect: dict = field(default_factory=dict, hash=False, compare=False)   # cus -> the part of form() the case is named for


def _moved(shape, c, cid):
    B, C, H, W = shape
    # what the table was written to reach on the emulation's 16 compute units
    expect = {((5, 7, 32, 32), 0): {EMU_CUS: dict(passes=1, g=1, tiles=[18])},
              ((67, 3, 2, 2), 0): {EMU_CUS: dict(passes=1, g=3, tiles=[26])}}.get((shape, c), {})
    if c:
        expect = {EMU_CUS: dict(passes=2), 256: dict(passes=2)}
    return Case(cid, B * C, H, W, c, masks=((True, C), (False, B * C)), expect=expect)


def build_table():
    t = [_moved(s, c, i) for (s, c), i in zip(CASES, IDS)]
    any_cus = lambda **kw: {EMU_CUS: kw, 256: kw}
    # grouped resident with a partial last group at 256 compute units: 257 tiles of 4 planes of 32 x 32 with one plane in the last,
    # 256 tiles of 1024 planes of 2 x 2 with 3 planes in the last (the scalar tail is not reached: a plane is 16 bytes)
    t.append(Case("grouped-g2-1025x32x32-last-tile-1-of-4", 1025, 32, 32, masks=((True, 205), (False, 205)), last=False, emu=False,
                  expect=any_cus(passes=1, g=2, tiles=[257])))
    P = 255 * 1024 + 3
    t.append(Case(f"grouped-g10-{P}x2x2-last-tile-3-of-1024", P, 2, 2, masks=((True, 1), (False, 1)), last=False, emu=False,
                  expect=any_cus(passes=1, g=10, tiles=[256])))
    # the last axis with an odd count of rows of 2 floats: the tensor ends inside a 16-byte access.  3 rows reach the l + g >= 2
    # floor (tiles of 4 floats), 256 * 1024 + 1 rows a grouped tile of 1024 rows at 256 compute units
    t.append(Case("last-axis-3-rows-of-2-floor", 3, 1, 2, plain=False, expect=any_cus(passes=1, g=1, nt=4, tiles=[2])))
    # planes of one float (H = W = 1: no butterfly, the scale only): the only shape whose tensor can end 1 or 3 floats into a
    # 16-byte access, where a store that took 3 remaining floats for 4 would write past the end
    t.append(Case("single-float-planes-7-ends-3-into-a-quad", 7, 1, 1, expect=any_cus(passes=1, g=2, nt=4, tiles=[2])))
    R = 256 * 1024 + 1
    t.append(Case(f"last-axis-{R}-rows-of-2-grouped", R, 1, 2, plain=False,
                  expect={256: dict(passes=1, g=10, tiles=[257]), EMU_CUS: dict(passes=1, g=11, tiles=[129])}))
    # two-pass on any device: planes above 2^14 floats
    for H, W, rl in ((256, 256, 2), (128, 1024, 3), (1024, 1024, 6)):
        for P in (1, 3):
            t.append(Case(f"two-pass-rl{rl}-{P}x{H}x{W}", P, H, W, masks=((True, 1),) if H * W > 2 ** 17 else ((True, 1), (False, P)),
                          last=False, emu=P * H * W <= 2 ** 18, expect=any_cus(passes=2, rl=rl)))
    assert len({c.id for c in t}) == len(t), "duplicate case ids"
    return t


TABLE = build_table()


# ---------------------------------------------------------------- the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.hadamard), `device` of its
    buffers, `stream()` -> the stream argument, `cus` the compute units run() sees there and - on the emulation - `reset()` /
    `launches()`, the launches since the last reset as "kernel xTHREADS" """

    def __init__(self, lib, device, stream, cus, reset=None, launches=None):
        self.lib, self.device, self._stream, self.cus = lib, torch.device(device), stream, int(cus)
        self.reset, self.launches = reset, launches

    def err(self):
        return self.lib.dinv_last_error().decode()

    def _logged(self, rc, f):
        if self.launches is not None and f is not None:
            want = [f"hadamard_tile_kernel x{t}" for t in f["threads"]] if rc == 0 else []
            assert self.launches() == want, f"launched {self.launches()}, the restated dispatch expects {want}"
        return rc

    def hadamard(self, x_ptr, out_ptr, P, H, W, flags, scale=1.0, f=None):
        if self.reset:
            self.reset()
        return self._logged(self.lib.dinv_hadamard(ctypes.c_void_p(x_ptr), ctypes.c_void_p(out_ptr), P, H, W, flags, scale, None, 0,
                                                   self._stream()), f)

    def apply(self, x_ptr, y_ptr, mask_ptr, out_ptr, P, H, W, mask_planes, flags, add=0.0, scale=1.0, f=None):
        if self.reset:
            self.reset()
        return self._logged(self.lib.dinv_hadamard_apply(ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr), ctypes.c_void_p(mask_ptr),
                                                         ctypes.c_void_p(out_ptr), P, H, W, mask_planes, flags, add, scale, None, 0,
                                                         self._stream()), f)


def _guarded(r, t):
    b = Guarded(t.numel(), r.device)
    b.t.copy_(t.reshape(-1))
    return b


def worst_plane(got, ref, den):
    """(max over planes of ||got_p - ref_p|| / den_p, its plane): [P, n] tensors and den [P]; a plane with den = 0 must be exact,
    NaN (an unwritten output) counts as infinite"""
    num = (got.double() - ref).pow(2).sum(-1).sqrt()
    e = torch.where(num == 0, torch.zeros_like(num), num / den)
    if bool(torch.isnan(e).any()):
        return float("inf"), int(torch.isnan(e).nonzero()[0])
    return float(e.max()), int(e.argmax())


def _norm(t):
    return t.pow(2).sum(-1).sqrt()


def _checked(r, c, what, out, ref, den, bound, worst):
    """the three checks after a call: guards, no word left unwritten, every plane within its bound"""
    assert out.guards_intact(), f"{c.id} {what}: write outside the output"
    left = int((out.bits() == POISON).sum())
    assert left == 0, f"{c.id} {what}: {left} outputs were never written"
    got = out.t.cpu().view(ref.shape)
    err, plane = worst_plane(got, ref, den)
    worst[what] = (err / bound, plane)
    assert err <= bound, f"{c.id} {what}: plane {plane} has error {err:.3g} > {bound:.3g}"
    return got


def _expect(r, c, f):
    for key, want in c.expect.get(r.cus, {}).items():
        assert f[key] == want, f"{c.id}: run() would take {key} = {f[key]} at {r.cus} compute units, the case is named for {want}"


def run_case(r, c):
    """runs case c on runner r, asserts everything the module docstring lists and returns {check: (worst error / bound, plane)}"""
    P, H, W = c.P, c.H, c.W
    n, L = H * W, bits(H, W)
    flag_c = RESIDENT_LOG2(c.c)
    gen = torch.Generator().manual_seed(P * 131 + H * 17 + W * 3 + c.c)
    x, y = torch.randn(P, n, generator=gen), torch.randn(P, n, generator=gen)
    xb, yb = _guarded(r, x), _guarded(r, y)
    X, Y = x.double(), y.double()
    worst = {}
    new = lambda: Guarded(P * n, r.device)
    one, two = (L + 4) * U, 2 * (L + 4) * U

    if c.plain:
        f = form(P, L, L, c.c, r.cus)
        _expect(r, c, f)
        TX = fwht(X) / n ** 0.5
        out = new()
        assert r.hadamard(xb.t.data_ptr(), out.t.data_ptr(), P, H, W, flag_c, 1.0, f) == 0, r.err()
        _checked(r, c, "H2", out, TX, _norm(X), one, worst)
        again = new()
        assert r.hadamard(xb.t.data_ptr(), again.t.data_ptr(), P, H, W, flag_c, 1.0, f) == 0, r.err()
        assert torch.equal(again.bits(), out.bits()), f"{c.id}: two identical calls differ"
        inpl = _guarded(r, x)
        assert r.hadamard(inpl.t.data_ptr(), inpl.t.data_ptr(), P, H, W, flag_c, 1.0, f) == 0, r.err()
        assert inpl.guards_intact() and torch.equal(inpl.bits(), out.bits()), f"{c.id}: in place differs from out of place"
        del again, inpl
        out = new()
        assert r.hadamard(xb.t.data_ptr(), out.t.data_ptr(), P, H, W, flag_c | NO_NORMALIZE, 0.5, f) == 0, r.err()
        _checked(r, c, "H2 raw x 0.5", out, 0.5 * n ** 0.5 * TX, 0.5 * n ** 0.5 * _norm(X), one, worst)

    if c.last:
        # rows of W floats: the planes of the last-axis transform
        Lw = W.bit_length() - 1
        f = form(P * H, Lw, Lw, min(c.c, 14), r.cus)
        if not c.plain:
            _expect(r, c, f)
        rows = X.view(P * H, W)
        raw = fwht(rows)
        for what, fl, ref in (("last axis", 0, raw / W ** 0.5), ("last axis raw", NO_NORMALIZE, raw)):
            out = new()
            assert r.hadamard(xb.t.data_ptr(), out.t.data_ptr(), P, H, W, flag_c | LAST_AXIS | fl, 1.0, f) == 0, r.err()
            _checked(r, c, what, out, ref, _norm(ref), (Lw + 4) * U, worst)

    for binary, mp in c.masks:
        assert P % mp == 0
        if binary:
            mask = (torch.rand(mp, n, generator=gen) < 0.4).float()
        else:
            mask = torch.rand(mp, n, generator=gen) * (torch.rand(mp, n, generator=gen) < 0.7).float()
        mb = _guarded(r, mask)
        m = mask.double().repeat(P // mp, 1)
        zero = m == 0
        smax = lambda s: s.abs().amax(-1)
        T = lambda v: fwht(v) / n ** 0.5
        f1, f2, f0 = form(P, L, L, c.c, r.cus), form(P, L, L, c.c, r.cus, True), form(P, L, 0, c.c, r.cus)
        _expect(r, c, f1)
        assert len(f2["tiles"]) == (3 if f1["passes"] == 2 else 1)
        TX = T(X)
        tag = ("binary" if binary else "real") + f"-mask{mp}"

        def call(what, inp, flags, ref, den, bound, f, yy=None, add=0.0, scale=1.0, zeros=False):
            out = new()
            rc = r.apply(inp.t.data_ptr(), yy.t.data_ptr() if yy is not None else 0, mb.t.data_ptr(), out.t.data_ptr(), P, H, W, mp,
                         flag_c | flags, add, scale, f)
            assert rc == 0, f"{c.id} {what}: {r.err()}"
            got = _checked(r, c, f"{what} {tag}", out, ref, den, bound, worst)
            if zeros:     # zero where the mask is: the sign bit aside (0 * negative = -0), every bit
                assert bool(((got[zero].view(torch.int32) & 0x7FFFFFFF) == 0).all()), f"{c.id} {what}: not zero where the mask is"
            return out

        call("A", xb, SYM(1), m * TX, smax(m) * _norm(X), one, f1, zeros=True)
        call("A^T", yb, PRE(1), T(m * Y), _norm(m * Y), one, f1)
        ata = call("A^T A", xb, SYM(2) | SECOND, T(m * m * TX), smax(m * m) * _norm(X), two, f2)
        again = call("A^T A", xb, SYM(2) | SECOND, T(m * m * TX), smax(m * m) * _norm(X), two, f2)
        assert torch.equal(again.bits(), ata.bits()), f"{c.id}: two identical A^T A calls differ"
        inpl = _guarded(r, x)
        assert r.apply(inpl.t.data_ptr(), 0, mb.t.data_ptr(), inpl.t.data_ptr(), P, H, W, mp, flag_c | SYM(2) | SECOND, 0.0, 1.0,
                       f2) == 0, r.err()
        assert inpl.guards_intact() and torch.equal(inpl.bits(), ata.bits()), f"{c.id}: A^T A in place differs from out of place"
        del again, inpl, ata
        aat = call("A A^T", yb, SYM(2) | NO_TRANSFORM, m * m * Y, _norm(m * m * Y), 2 * U, f0, zeros=True)
        if binary:
            assert torch.equal(aat.t.cpu().view(P, n), mask.repeat(P // mp, 1) ** 2 * y), f"{c.id}: A A^T is an exact product"
        del aat
        for gamma in (0.7, 1e-3):
            w = (m * Y + TX / gamma) / (m * m + 1 / gamma)
            call(f"prox gamma={gamma:g}", xb, SYM(3) | SECOND, T(w), torch.maximum(_norm(X), _norm(w)), two + 4 * U, f2, yy=yb,
                 add=1 / gamma)
        call("A^+", yb, PRE(2), T(Y * r_inv(m)), _norm(Y * r_inv(m)), one + U, f1)
        # the transposes the backward passes use
        g = 1 / 0.7
        s = m / (m * m + g)
        call("d prox / d y", xb, SYM(4), s * TX, smax(s) * _norm(X), one + 2 * U, f1, add=g)
        call("(A^+)^T", xb, SYM(5), TX * r_inv(m), smax(r_inv(m)) * _norm(X), one + U, f1, zeros=True)
        s = g / (m * m + g)
        call("d prox / d z", xb, SYM(3) | SECOND, T(TX * s), smax(s) * _norm(X), two + 4 * U, f2, add=g)
        # the caller's scale
        call("-2 A", xb, SYM(1), -2 * m * TX, 2 * smax(m) * _norm(X), one, f1, scale=-2.0)
        assert mb.guards_intact() and torch.equal(mb.t.cpu(), mask.reshape(-1)), f"{c.id}: the mask was modified"
    assert xb.guards_intact() and yb.guards_intact() and torch.equal(xb.t.cpu(), x.reshape(-1)) and \
        torch.equal(yb.t.cpu(), y.reshape(-1)), f"{c.id}: an input was modified"
    return worst


def report(c, worst):
    what, (ratio, plane) = max(worst.items(), key=lambda kv: kv[1][0])
    return f"{c.id}: worst plane {plane} of {what}: error / bound {ratio:.3g}"


def run_misaligned(r):
    """x or out 4 bytes off 16-byte alignment is refused, and the guarded output is untouched afterwards"""
    P, H, W = 3, 8, 8
    x = _guarded(r, torch.randn(P * H * W + 1, generator=torch.Generator().manual_seed(1)))
    mask = _guarded(r, torch.ones(H * W))
    out = Guarded(P * H * W + 1, r.device)
    for xo, oo in ((4, 0), (0, 4), (4, 4)):
        assert r.hadamard(x.t.data_ptr() + xo, out.t.data_ptr() + oo, P, H, W, 0) != 0 and "aligned" in r.err()
        assert r.hadamard(x.t.data_ptr() + xo, out.t.data_ptr() + oo, P, H, W, LAST_AXIS) != 0 and "aligned" in r.err()
        assert r.apply(x.t.data_ptr() + xo, 0, mask.t.data_ptr(), out.t.data_ptr() + oo, P, H, W, 1, SYM(1)) != 0 and \
            "aligned" in r.err()
    if r.device.type == "cuda":
        torch.cuda.synchronize(r.device)
    assert out.untouched(), "a refused call wrote to its output"
    if r.launches is not None:
        assert r.launches() == []
