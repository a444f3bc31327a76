"""Shared by tests/test_svblur_gpu.py (the gfx950 library) and tests/test_emu_svblur.py (the same kernel sources on the host
emulation): one table of product-convolution cases for dinv_pconv2d / dinv_pconv2d_transpose (csrc/blur.hip), the fp64 definition,
the Python restatement of the launcher's rules, the runner that calls the C entry points on guarded buffers (fft_cases.Guarded)
and the checks of every case; and the class-level, autograd and golden checks both files run on their device.

The definition (deepinv/physics/functional/product_convolution.py:10-68; `_ref_conv` is the fp64 conv2d of conv_cases.py):
    A x   = sum_k _ref_conv(w_k x, h_k, mode, 1)           A^T v = autograd of <A x, v> with respect to x.

The launcher, restated.  One launch per call.  The tiled kernel (pconv2d_tiled_kernel / pconv2d_tiled_transpose_kernel) where
launch_tiled takes the plain convolution: always for A, for A^T in valid / circular / constant, when the filter table and the
patch fit, ((fh + 6) w4 + (64 + fh - 1) (64 + w4)) 4 <= 65536 bytes with w4 = fw rounded up to 4 (conv_cases.tiled_lds).  Else
the general kernel (pconv2d_pad_kernel / pconv2d_pad_transpose_kernel) with fh fw 4 bytes of LDS.

Layout, exact.  Integer operands in [-4, 4] drawn at random for x, w, h and v.  A term |h| |w| |x| is at most 64, an output of A
has at most K fh fw of them, so every partial sum stays below K fh fw 64 < 2^24 (asserted for every case; for A^T, whose border
pixels collect the folded taps, the sum of the absolute terms is asserted below 2^24 as well): fp32 accumulates them without
rounding in any order and the result must equal the exact integer evaluation bit for bit.  This catches a swapped k, a
multiplier indexed after the padding instead of before, and a wrong fold-back.

Rounding, per element.  randn operands, |got - exact| <= gamma_n sum |h| |w| |x| over the terms of that element, gamma_n =
n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  n is counted from the
kernels' operation order, not measured:
  A (both kernels): the product w_k x is rounded once (before it is staged / used), and ALL K fh fw products of an output are
    accumulated by ONE chain of fused multiply-adds, the accumulator staying in a register across k (the zero taps of the tiled
    table add exact zeros).  A term passes through at most K fh fw roundings of the chain and the one of its product:
        n_A = K fh fw + 1.
  A^T (both kernels): per k the T products of an element - T = the number of (tap, measurement) pairs that fold onto it, fh fw
    in the interior, up to 9 fh fw (reflect) or (fh/2 + 1)(fw/2 + 1) fh fw (replicate) at a border - are accumulated by one chain
    of T fused multiply-adds; the partial result joins the total with one more fused multiply-add by w_k[r, c], K of them:
        n_AT = T + K,   T counted per element as the transpose applied to all-ones operands (conv of ones, fp64).

Dot test.  |<A x, v> - <x, A^T v>| <= 1e-5 max(|<A x, v>|, 1, 0.01 |A x| |v|), the bound of tests/test_emu_blur.py.

Every buffer is guarded (POISON is a NaN): a read outside x, w, h, v shows in the result, a write outside the result in the
guard bands."""
import ctypes
import os
from dataclasses import dataclass

import numpy as np
import torch

import conv_cases as CC
from conv_cases import _ref_conv
from fft_cases import POISON, Guarded

from deepinv_amd.hip.conv import ConvDesc

U = 2.0 ** -24
ALL = ("valid", "circular", "reflect", "replicate", "constant")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svblur.npz")


def gamma(n):
    return n * U / (1 - n * U)


# ------------------------------------------------------------------ the fp64 definition
def ref_A(x, w, h, mode):
    """sum_k conv(w_k x, h_k) in the dtype of the operands (fp64 in the tests): x [B,C,H,W], w [b,c,K,H,W], h [b',c',K,fh,fw]"""
    out = 0
    for k in range(w.shape[2]):
        out = out + _ref_conv(w[:, :, k] * x, h[:, :, k], mode, 1)
    return out


def ref_AT(v, w, h, mode, size):
    """the transpose by autograd through the definition"""
    B, C = v.shape[:2]
    z = torch.zeros(B, C, *size, dtype=v.dtype, requires_grad=True)
    (ref_A(z, w, h, mode) * v).sum().backward()
    return z.grad


# ------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    B: int
    C: int
    H: int
    W: int
    mb: int
    mc: int
    fb: int
    fc: int
    K: int
    fh: int
    fw: int
    emu: bool = True
    modes: tuple = ALL

    @property
    def id(self):
        return (f"{self.B}x{self.C}x{self.H}x{self.W}-w{self.mb}x{self.mc}-h{self.fb}x{self.fc}-K{self.K}-k{self.fh}x{self.fw}")

    def conv(self, mode):
        return CC.Conv2(self.B, self.C, self.H, self.W, self.fb, self.fc, self.fh, self.fw, mode, 1)


_T = [
    Case(1, 1, 8, 9, 1, 1, 1, 1, 1, 3, 3),                  # K = 1: equals dinv_conv2d(w x)
    Case(2, 3, 17, 19, 1, 1, 1, 1, 3, 5, 4),                # both shared, even and odd filter sides
    Case(2, 2, 20, 13, 2, 2, 2, 2, 4, 3, 7),                # per plane
    Case(2, 3, 12, 10, 1, 3, 2, 1, 3, 3, 4),                # mixed broadcasting
    Case(2, 3, 12, 10, 2, 1, 1, 3, 3, 4, 3),
    Case(1, 1, 9, 9, 1, 1, 1, 1, 2, 9, 9),                  # valid: a 1 x 1 output
    Case(1, 1, 4, 5, 1, 1, 1, 1, 2, 7, 9),                  # filter larger than the image: valid refused, reflect legal (3 < 4, 4 < 5)
    Case(1, 2, 8, 9, 1, 1, 1, 1, 1, 1, 1),                  # 1 x 1 filter: no padding in any mode, pinned to the fp64 definition
    Case(2, 1, 70, 66, 2, 1, 2, 1, 3, 8, 6),                # several 64-tiles, ragged edges, Wo % 4 != 0: the scalar store
    Case(1, 2, 65, 130, 1, 1, 1, 1, 2, 3, 3),               # a one-row overhang, three tiles across
    Case(1, 1, 24, 24, 1, 1, 1, 1, 10, 7, 7),               # K = 10
    # the tiled budget of 16384 floats: 51 x 51 and 52 x 52 (65424 B) fit, 53 x 53 does not and takes the general kernels
    Case(1, 1, 56, 60, 1, 1, 1, 1, 2, 51, 51),
    Case(1, 1, 56, 60, 1, 1, 1, 1, 2, 52, 52),
    Case(1, 1, 56, 60, 1, 1, 1, 1, 2, 53, 53),
    # past the budget with several workgroups per plane and per-plane operands: seconds on the emulation, device only
    Case(2, 2, 65, 70, 2, 2, 2, 2, 2, 53, 53, emu=False, modes=("valid", "circular")),
]
CASES = [(c, m) for c in _T for m in c.modes]
assert len({(c.id, m) for c, m in CASES}) == len(CASES) and len({c.id for c in _T}) == len(_T), "duplicate case ids"
for _c in _T:
    assert _c.K * _c.fh * _c.fw * 64 < 2 ** 24, f"{_c.id}: the exact check needs every partial sum below 2^24"


def item_id(item):
    return f"{item[0].id}-{item[1]}"


# ------------------------------------------------------------------ the launcher's rules, restated
def rejection(c, mode, stride=1):
    """the check of make_pgeom / make_geom the call fails (None when it is accepted)"""
    if stride != 1:
        return "stride must be 1"
    if c.K < 1:
        return "bad number of filters"
    r = CC.rejection(c.conv(mode))
    if r:
        return r
    if c.mb not in (1, c.B) or c.mc not in (1, c.C):
        return "multiplier shape not broadcastable"
    return None


def expected_kernel(c, mode, transpose):
    gather = not transpose or mode in ("valid", "circular", "constant")
    if gather and CC.tiled_lds(c.fh, c.fw) <= CC.LDS_MAX:
        return "pconv2d_tiled_transpose_kernel" if transpose else "pconv2d_tiled_kernel"
    return "pconv2d_pad_transpose_kernel" if transpose else "pconv2d_pad_kernel"


def lds_bytes(c, mode, transpose):
    return CC.tiled_lds(c.fh, c.fw) if "tiled" in expected_kernel(c, mode, transpose) else c.fh * c.fw * 4


assert CC.tiled_lds(51, 51) < CC.tiled_lds(52, 52) == 65424 <= CC.LDS_MAX < CC.tiled_lds(53, 53)


# ------------------------------------------------------------------ the runner
class Runner:
    """the two C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.conv), `device` of its
    buffers, `stream()` -> the stream argument and - on the emulation - `reset()` / `launches()`"""

    def __init__(self, lib, device, stream, reset=None, launches=None):
        self.lib, self.device, self._stream = lib, torch.device(device), stream
        self.reset, self.launches = reset, launches

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def err(self):
        return self.lib.dinv_last_error().decode()

    def call(self, transpose, desc, K, mb, mc, a, w, h, out, expect=None):
        """a, w, h, out: addresses; desc: a ConvDesc or None (a null descriptor)"""
        if self.reset:
            self.reset()
        fn = self.lib.dinv_pconv2d_transpose if transpose else self.lib.dinv_pconv2d
        rc = fn(ctypes.byref(desc) if desc is not None else None, K, mb, mc, ctypes.c_void_p(a), ctypes.c_void_p(w), ctypes.c_void_p(h),
                ctypes.c_void_p(out), self._stream())
        self.sync()
        if self.launches is not None and expect is not None:
            got = self.launches()
            assert got == expect, f"launched {got}, the restated dispatch expects {expect}"
        return rc

    def conv2d(self, desc, x, k, out):
        rc = self.lib.dinv_conv2d(ctypes.byref(desc), ctypes.c_void_p(x), ctypes.c_void_p(k), ctypes.c_void_p(out), self._stream())
        self.sync()
        assert rc == 0, self.err()


def _guarded(r, t):
    g = Guarded(t.numel(), r.device)
    g.t.copy_(t.reshape(-1).float())
    return g


def _apply(r, c, mode, transpose, a, w, h, nout):
    """one guarded call and a second one into a fresh buffer; returns the result on the CPU (flat, fp32)"""
    bufs = [_guarded(r, t) for t in (a, w, h)]
    before = [b.bits().clone() for b in bufs]
    expect = [expected_kernel(c, mode, transpose)]
    results = []
    for _ in range(2):
        out = Guarded(nout, r.device)
        rc = r.call(transpose, c.conv(mode).desc(), c.K, c.mb, c.mc, bufs[0].t.data_ptr(), bufs[1].t.data_ptr(), bufs[2].t.data_ptr(),
                    out.t.data_ptr(), expect)
        assert rc == 0, f"error {rc}: {r.err()}"
        bits = out.bits()
        assert out.guards_intact(), "write outside the result"
        assert not bool((bits == POISON).any()), (f"{int((bits == POISON).sum())} outputs hold the guard pattern: never written, or "
                                                  "computed from a read outside the operands")
        results.append(bits.clone())
    assert torch.equal(results[0], results[1]), "two identical calls differ"
    for b, was in zip(bufs, before):
        assert b.guards_intact() and torch.equal(b.bits(), was), "the call modified an operand"
    return results[0].view(torch.float32)


def _worst(got, exact, bound):
    """max over elements of |got - exact| / bound (bound == 0: got must equal exact); NaN counts as infinite"""
    return CC.worst_ratio(got, exact, bound)


def run_case(r, c, mode):
    """runs case c in padding `mode` on runner r, asserts everything the module docstring lists, returns the worst error / bound
    of A and A^T"""
    if rejection(c, mode):
        return _run_reject(r, c, mode, c.conv(mode).desc(), c.K, c.mb, c.mc, rejection(c, mode))
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(item_id((c, mode)))) % (2 ** 31)
    gen = torch.Generator().manual_seed(seed)
    B, C, H, W, K = c.B, c.C, c.H, c.W, c.K
    Ho, Wo = CC.out_size(H, c.fh, mode), CC.out_size(W, c.fw, mode)
    shapes = ((B, C, H, W), (c.mb, c.mc, K, H, W), (c.fb, c.fc, K, c.fh, c.fw), (B, C, Ho, Wo))
    # ---- layout, exact
    x, w, h, v = (torch.randint(-4, 5, s, generator=gen).double() for s in shapes)
    want = ref_A(x, w, h, mode)
    assert tuple(want.shape) == (B, C, Ho, Wo)
    want_t = ref_AT(v, w, h, mode, (H, W))
    assert float(ref_A(x.abs(), w.abs(), h.abs(), mode).max()) < 2 ** 24
    assert float(ref_AT(v.abs(), w.abs(), h.abs(), mode, (H, W)).max()) < 2 ** 24
    for transpose, a, exact in ((False, x, want), (True, v, want_t)):
        got = _apply(r, c, mode, transpose, a, w, h, exact.numel()).double().view(exact.shape)
        wrong = got != exact
        assert not bool(wrong.any()), (f"{'A^T' if transpose else 'A'}: {int(wrong.sum())} of {wrong.numel()} integer outputs are wrong, "
                                       f"the first at {tuple(int(i) for i in wrong.nonzero()[0])}")
    # ---- rounding, per element
    x, w, h, v = (torch.randn(s, generator=gen) for s in shapes)
    xd, wd, hd, vd = x.double(), w.double(), h.double(), v.double()
    y = _apply(r, c, mode, False, x, w, h, B * C * Ho * Wo).view(B, C, Ho, Wo)
    n_a = K * c.fh * c.fw + 1
    err_a = _worst(y, ref_A(xd, wd, hd, mode), gamma(n_a) * ref_A(xd.abs(), wd.abs(), hd.abs(), mode))
    assert err_a <= 1.0, f"A: an element is {err_a:.3g} times its bound gamma_{n_a} sum |h| |w| |x|"
    xt = _apply(r, c, mode, True, v, w, h, B * C * H * W).view(B, C, H, W)
    ones = [torch.ones(s, dtype=torch.float64) for s in shapes]
    terms = ref_AT(ones[3], ones[1][:, :, :1], ones[2][:, :, :1], mode, (H, W))        # T: the products of one k per element
    err_t = _worst(xt, ref_AT(vd, wd, hd, mode, (H, W)), gamma(terms + K) * ref_AT(vd.abs(), wd.abs(), hd.abs(), mode, (H, W)))
    assert err_t <= 1.0, f"A^T: an element is {err_t:.3g} times its bound gamma_(T + {K}) sum |w| |h| |v|"
    # ---- dot test
    lhs, rhs = float((y.double() * vd).sum()), float((xd * xt.double()).sum())
    tol = 1e-5 * max(abs(lhs), 1.0, 0.01 * float(y.double().norm() * vd.norm()))
    assert abs(lhs - rhs) <= tol, f"dot test: <A x, v> = {lhs}, <x, A^T v> = {rhs}"
    # ---- K = 1 on the tiled kernel: the bits of dinv_conv2d(w x), the same chain of multiply-adds
    if K == 1 and (c.mb, c.mc) == (1, 1) and (c.fb, c.fc) == (1, 1):
        wx = _guarded(r, (w[:, :, 0] * x).contiguous())
        hb, out = _guarded(r, h), Guarded(B * C * Ho * Wo, r.device)
        r.conv2d(c.conv(mode).desc(), wx.t.data_ptr(), hb.t.data_ptr(), out.t.data_ptr())
        assert torch.equal(out.bits(), y.reshape(-1).view(torch.int32)), "K = 1 differs from dinv_conv2d(w x)"
    print(f"{item_id((c, mode))}: A {err_a:.3g} of gamma_{n_a}, A^T {err_t:.3g} of gamma_(T + {K}), T <= {int(terms.max())}")
    return err_a, err_t


def _run_reject(r, c, mode, desc, K, mb, mc, reason):
    """both entry points return an error with `reason` in dinv_last_error, launch nothing and leave the (poisoned) result alone"""
    n = max(c.B, 1) * max(c.C, 1) * c.H * c.W
    a, w, h = (r_dev(r, torch.randn(m)) for m in (n, max(mb, 1) * max(mc, 1) * max(K, 1) * c.H * c.W,
                                                   max(c.fb, 1) * max(c.fc, 1) * max(K, 1) * c.fh * c.fw))
    for transpose in (False, True):
        out = Guarded(n, r.device)
        rc = r.call(transpose, desc, K, mb, mc, a.data_ptr(), w.data_ptr(), h.data_ptr(), out.t.data_ptr(), expect=[])
        assert rc != 0, f"dinv_pconv2d{'_transpose' if transpose else ''} accepted a call it must refuse ({reason})"
        assert reason in r.err(), f"refused for '{r.err()}', the restated checks expect '{reason}'"
        assert out.untouched(), "a refused call wrote to its result"
    return None


def r_dev(r, t):
    return t.contiguous().to(r.device)


def refusals():
    """(id, case, mode, stride, null descriptor, reason) of every bad argument the entry points must refuse"""
    ok = Case(2, 3, 12, 10, 1, 1, 1, 1, 2, 3, 3)
    R = [
        ("null-descriptor", ok, "reflect", 1, True, "null descriptor"),
        ("stride-2", ok, "reflect", 2, False, "stride must be 1"),
        ("K-0", Case(2, 3, 12, 10, 1, 1, 1, 1, 0, 3, 3), "reflect", 1, False, "bad number of filters"),
        ("multiplier-batch-3-of-2", Case(2, 3, 12, 10, 3, 1, 1, 1, 2, 3, 3), "constant", 1, False, "multiplier shape not broadcastable"),
        ("multiplier-channels-2-of-3", Case(2, 3, 12, 10, 1, 2, 1, 1, 2, 3, 3), "valid", 1, False, "multiplier shape not broadcastable"),
        ("filter-batch-3-of-2", Case(2, 3, 12, 10, 1, 1, 3, 1, 2, 3, 3), "circular", 1, False, "filter shape not broadcastable"),
        ("filter-channels-2-of-3", Case(2, 3, 12, 10, 1, 1, 1, 2, 2, 3, 3), "replicate", 1, False, "filter shape not broadcastable"),
        ("valid-filter-larger", Case(1, 1, 4, 5, 1, 1, 1, 1, 2, 7, 9), "valid", 1, False, "filter larger than"),
        ("circular-pad-wider", Case(1, 1, 5, 20, 1, 1, 1, 1, 2, 12, 3), "circular", 1, False, "circular padding wider than"),
        ("reflect-pad-eq-image", Case(1, 1, 8, 20, 1, 1, 1, 1, 2, 17, 3), "reflect", 1, False, "reflect padding must be smaller"),
        ("planes-65536", Case(1, 65536, 1, 1, 1, 1, 1, 1, 1, 1, 1), "constant", 1, False, "too many (batch*channel) planes"),
        ("filter-66048B", Case(1, 1, 8, 8, 1, 1, 1, 1, 1, 129, 128), "constant", 1, False, "filter too large for LDS"),
        ("mode-5", ok, 5, 1, False, "unknown padding mode"),
    ]
    return R


def run_refusal(r, item):
    _, c, mode, stride, null, reason = item
    if not null and stride == 1 and mode in ALL:
        assert reason in (rejection(c, mode) or ""), (rejection(c, mode), reason)
    desc = None
    if not null:
        desc = ConvDesc(c.B, c.C, c.H, c.W, c.fb, c.fc, c.fh, c.fw, CC.MODES.get(mode, mode), stride)
    _run_reject(r, c, mode, desc, c.K, c.mb, c.mc, reason)


def run_empty_batch(r):
    """B = 0: returns 0 without a launch (NULL operands are fine)"""
    d = ConvDesc(0, 3, 12, 10, 1, 1, 3, 3, 2, 1)
    for transpose in (False, True):
        assert r.call(transpose, d, 2, 1, 1, 0, 0, 0, 0, expect=[]) == 0, r.err()


# ------------------------------------------------------------------ class level (run under emu_backend() or on the device)
def _params(gen, B, C, K, H, W, fh, fw, mb=1, mc=1, fb=1, fc=1):
    return torch.randn(fb, fc, K, fh, fw, generator=gen) / (fh * fw) ** 0.5, torch.randn(mb, mc, K, H, W, generator=gen)


def _close(got, exact, bound, what):
    ratio = CC.worst_ratio(got, exact, bound)
    assert ratio <= 1.0, f"{what}: an element is {ratio:.3g} times its counted bound"


def check_class(dev):
    """SpaceVaryingBlur.A / A_adjoint / A_adjoint_A against the fp64 definition within the counted bounds, a parameter update
    through A(x, filters=..., padding=...), use_fft=True against use_fft=False, and the LinearPhysics machinery on top"""
    import deepinv_amd as dinv

    gen = torch.Generator().manual_seed(868)
    B, C, K, H, W, fh, fw = 2, 3, 3, 14, 12, 5, 4
    h, w = _params(gen, B, C, K, H, W, fh, fw, mb=1, mc=C, fb=B, fc=1)
    x = torch.randn(B, C, H, W, generator=gen)
    p = dinv.physics.SpaceVaryingBlur(filters=h, multipliers=w, padding="reflect", device=dev)
    assert p.filters.device.type == torch.device(dev).type and set(p.state_dict()) >= {"filters", "multipliers"}
    n_a, n_t = K * fh * fw + 1, 9 * fh * fw + K
    hd, wd, xd = h.double(), w.double(), x.double()
    y = p.A(x.to(dev))
    ref = ref_A(xd, wd, hd, "reflect")
    _close(y, ref, gamma(n_a) * ref_A(xd.abs(), wd.abs(), hd.abs(), "reflect"), "A")
    v = torch.randn(ref.shape, generator=gen)
    xt = p.A_adjoint(v.to(dev))
    _close(xt, ref_AT(v.double(), wd, hd, "reflect", (H, W)), gamma(n_t) * ref_AT(v.double().abs(), wd.abs(), hd.abs(), "reflect", (H, W)),
           "A_adjoint")
    ata = p.A_adjoint_A(x.to(dev))
    assert torch.equal(ata, p.A_adjoint(y)), "A_adjoint_A is A_adjoint(A(.)) through the base class"
    # a parameter update through A: stored, and used by the next A_adjoint
    h2, _ = _params(gen, B, C, K, H, W, 3, 3)
    y2 = p.A(x.to(dev), filters=h2.to(dev), padding="valid")
    assert p.padding == "valid" and tuple(p.filters.shape) == (1, 1, K, 3, 3) and tuple(y2.shape) == (B, C, H - 2, W - 2)
    ref2 = ref_A(xd, wd, h2.double(), "valid")
    _close(y2, ref2, gamma(K * 9 + 1) * ref_A(xd.abs(), wd.abs(), h2.double().abs(), "valid"), "A after the update")
    assert tuple(p.A_adjoint(y2).shape) == (B, C, H, W)
    # use_fft = True: the loop over k on conv2d_fft / conv_transpose2d_fft, every mode, against the spatial kernels
    for mode in ALL:
        ps = dinv.physics.SpaceVaryingBlur(filters=h, multipliers=w, padding=mode, device=dev)
        pf = dinv.physics.SpaceVaryingBlur(filters=h, multipliers=w, padding=mode, use_fft=True, device=dev)
        ys, yf = ps.A(x.to(dev)), pf.A(x.to(dev))
        assert float((ys - yf).norm() / ys.norm()) < 1e-5, mode
        vv = torch.randn(ys.shape, generator=gen).to(dev)
        a_s, a_f = ps.A_adjoint(vv), pf.A_adjoint(vv)
        assert float((a_s - a_f).norm() / a_s.norm()) < 1e-5, mode
    # LinearPhysics on top: the norm, the least-squares prox through CG
    p = dinv.physics.SpaceVaryingBlur(filters=h, multipliers=w, padding="circular", device=dev)
    x0 = torch.randn(B, C, H, W, generator=gen).to(dev)
    nrm = p.compute_norm(x0, max_iter=20, tol=1e-3, verbose=False)
    assert float(torch.as_tensor(nrm).max()) > 0
    z, gam = torch.randn(B, C, H, W, generator=gen).to(dev), 0.7
    yy = p.A(x.to(dev))
    u = p.prox_l2(z, yy, gam)
    res = p.A_adjoint(p.A(u) - yy) + (u - z) / gam          # the optimality condition of argmin 1/2 |A u - y|^2 + 1/(2 gam) |u - z|^2
    assert float(res.norm() / (z.norm() / gam)) < 1e-2


def check_autograd(dev):
    """d<A x, v>/dx is A^T v bit for bit (the same kernel); the gradients with respect to the filters and the multipliers (the
    composition of the differentiable pieces) against fp64 autograd of the definition to relative 2e-6"""
    from deepinv_amd.physics import functional as dF

    gen = torch.Generator().manual_seed(41)
    B, C, K, H, W, fh, fw = 2, 2, 3, 13, 11, 4, 3
    for mode in ("reflect", "valid", "circular"):
        h, w = _params(gen, B, C, K, H, W, fh, fw, mb=B, mc=1, fb=1, fc=C)
        x = torch.randn(B, C, H, W, generator=gen)
        Ho, Wo = CC.out_size(H, fh, mode), CC.out_size(W, fw, mode)
        v = torch.randn(B, C, Ho, Wo, generator=gen)
        xg = x.to(dev).clone().requires_grad_(True)
        y = dF.product_convolution2d(xg, w.to(dev), h.to(dev), mode)
        (gx,) = torch.autograd.grad((y * v.to(dev)).sum(), xg)
        assert torch.equal(gx, dF.product_convolution2d_adjoint(v.to(dev), w.to(dev), h.to(dev), mode)), mode
        vg = v.to(dev).clone().requires_grad_(True)
        xt = dF.product_convolution2d_adjoint(vg, w.to(dev), h.to(dev), mode)
        (gv,) = torch.autograd.grad((xt * x.to(dev)).sum(), vg)
        assert torch.equal(gv, y.detach()), mode
        # parameter gradients
        hd, wd = h.double().requires_grad_(True), w.double().requires_grad_(True)
        (ref_A(x.double(), wd, hd, mode) * v.double()).sum().backward()
        hg, wg = h.to(dev).clone().requires_grad_(True), w.to(dev).clone().requires_grad_(True)
        yp = dF.product_convolution2d(x.to(dev), wg, hg, mode)
        assert float((yp.detach() - y.detach()).norm() / y.detach().norm()) < 2e-6
        (yp * v.to(dev)).sum().backward()
        for name, got, want in (("filters", hg.grad, hd.grad), ("multipliers", wg.grad, wd.grad)):
            rel = float((got.cpu().double() - want).norm() / want.norm())
            assert rel < 2e-6, f"{mode}: gradient w.r.t. the {name} off by {rel:.3g}"
        hg2, wg2 = h.to(dev).clone().requires_grad_(True), w.to(dev).clone().requires_grad_(True)
        (dF.product_convolution2d_adjoint(v.to(dev), wg2, hg2, mode) * x.to(dev)).sum().backward()    # <x, A^T v> = <A x, v>
        for name, got, want in (("filters", hg2.grad, hd.grad), ("multipliers", wg2.grad, wd.grad)):
            rel = float((got.cpu().double() - want).norm() / want.norm())
            assert rel < 2e-6, f"{mode}: gradient of the adjoint w.r.t. the {name} off by {rel:.3g}"


def t_max(fh, fw):
    """the most products of one k that fold onto one element of A^T: 3 pre-images per axis (circular, reflect), fh / 2 + 1 (replicate)"""
    return max(3, fh // 2 + 1) * max(3, fw // 2 + 1) * fh * fw


def golden():
    return np.load(GOLDEN)


def check_golden_definition(gold):
    """the fp64 definition reproduces the stored outputs of the reference (fp32) within the counted bounds of the REFERENCE's
    evaluation: per k a convolution of fh fw products, the rounded product w_k x (w_k times the rounded transposed convolution),
    and K - 1 additions of the partial results: n = fh fw + K (A), T + K (A^T, T <= t_max)"""
    for tag in ("diffraction", "motion", "mixed"):
        x, h, w = (torch.from_numpy(gold[f"{tag}_{n}"]).double() for n in ("x", "filters", "multipliers"))
        K, fh, fw = h.shape[2:]
        for mode in ALL:
            y, v, adj = (torch.from_numpy(gold[f"{tag}_{mode}_{n}"]).double() for n in ("y", "v", "adj"))
            _close(y, ref_A(x, w, h, mode), gamma(fh * fw + K) * ref_A(x.abs(), w.abs(), h.abs(), mode), f"{tag} {mode}: reference A")
            size = tuple(x.shape[-2:])
            t = t_max(fh, fw)
            _close(adj, ref_AT(v, w, h, mode, size), gamma(t + K) * ref_AT(v.abs(), w.abs(), h.abs(), mode, size),
                   f"{tag} {mode}: reference A_adjoint")


def check_golden_product(gold, dev):
    """the product's outputs on the stored operands lie within the counted bounds of the fp64 definition"""
    import deepinv_amd as dinv

    for tag in ("diffraction", "motion", "mixed"):
        x, h, w = (torch.from_numpy(gold[f"{tag}_{n}"]) for n in ("x", "filters", "multipliers"))
        K, fh, fw = h.shape[2:]
        xd, hd, wd = x.double(), h.double(), w.double()
        for mode in ALL:
            v = torch.from_numpy(gold[f"{tag}_{mode}_v"])
            p = dinv.physics.SpaceVaryingBlur(filters=h, multipliers=w, padding=mode, device=dev)
            _close(p.A(x.to(dev)), ref_A(xd, wd, hd, mode), gamma(K * fh * fw + 1) * ref_A(xd.abs(), wd.abs(), hd.abs(), mode),
                   f"{tag} {mode}: A")
            size = tuple(x.shape[-2:])
            t = t_max(fh, fw)
            _close(p.A_adjoint(v.to(dev)), ref_AT(v.double(), wd, hd, mode, size),
                   gamma(t + K) * ref_AT(v.double().abs(), wd.abs(), hd.abs(), mode, size), f"{tag} {mode}: A_adjoint")
