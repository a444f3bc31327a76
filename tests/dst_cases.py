"""Shared by tests/test_operator_kernels_gpu.py (the gfx950 library) and tests/test_emu_operator_cases.py (the same kernel
sources on the host emulation): the case tables of csrc/dst.hip - the bare DST-I (dinv_dst1) and the fused StructuredRandom
operator (dinv_structured_apply) - the fp64 restatement (the dense sine matrix with the reference's sign, with pad, diagonals
and trim composed around it per axis), the Python restatement of the launcher's `lines` rule and the runner that calls the C
entry points on guarded buffers (tests/fft_cases.py Guarded).

Bound, per row.  The derived bound of tests/test_emu_dst.py: a radix-r butterfly stage of the FFT of length P = 2 (n + 1) adds
at most (r + 3) u to the relative l2 error (radix 4 and 8 are two and three radix-2 levels), the final scale and a diagonal one u
each, so an operator of T transforms is within (T (sum_stages (r + 3) + 2) + diagonals) u, u = 2^-24.  Two rows ride one
complex transform, so the error of a row is relative to the l2 norm of the fp64 result over the row and its partner in the
pair - over the whole working row of each, which a column trim shortens only after the last transform.  Rows are drawn alike
(randn) and the diagonals are signs, so the norm of a row is the same before and after every layer, as the bound assumes.

Exactness.  The padded output rows that meet no input row are zero in every bit but the sign.  The input rows a trim discards
are never read: the case runs with NaN in them and must return the bits of the run with zeros there."""
import ctypes
import math
from dataclasses import dataclass

import torch

from fft_cases import POISON, Guarded

U = 2.0 ** -24
THREADS, MAX_LINES, TILE_BUDGET = 256, 32, 32 * 1024


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the launcher's rules, restated
def fft_line_stride(n):
    """csrc/fft_core.hpp fft_line_stride"""
    return n + 1 if n % 2 == 0 else n


def lines_per_workgroup(rows, n):
    """`lines` of csrc/dst.hip launch(): pairs of rows per workgroup"""
    P = 2 * (n + 1)
    lines = max(1, min(MAX_LINES, TILE_BUDGET // (2 * fft_line_stride(P) * 8)))
    want = cdiv(cdiv(rows, 2), 256)
    return max(1, want) if want < lines else lines


def workgroups(rows, n):
    return max(1, cdiv(cdiv(rows, 2), lines_per_workgroup(rows, n)))


def sine(n):
    j = torch.arange(1, n + 1, dtype=torch.float64)
    return -math.sqrt(2.0 / (n + 1)) * torch.sin(math.pi * j[:, None] * j[None, :] / (n + 1))


# ------------------------------------------------------------------ the case tables
@dataclass(frozen=True)
class Bare:
    n: int
    rows: int
    lines: int                  # what the case is meant to reach; asserted against lines_per_workgroup
    what: str
    inplace: bool = False
    emu: bool = True

    @property
    def id(self):
        return f"dst1-n{self.n}-rows{self.rows}-lines{self.lines}-{self.what}"


BARE = [
    # the length: one thread group covers the row (n <= tpl = 256) or strides it (257, 1024); 100 and 1024 take the generic
    # radix stage (P = 202 = 2 101, P = 2050 = 2 5^2 41)
    Bare(1, 3, 1, "shortest"), Bare(2, 3, 1, "n2"), Bare(3, 5, 1, "n3"), Bare(12, 3, 1, "dead-partner"),
    Bare(31, 2, 1, "one-pair"), Bare(100, 3, 1, "generic-stage"), Bare(255, 5, 1, "below-tpl"), Bare(256, 5, 1, "tpl"),
    Bare(257, 5, 1, "tpl-strides"), Bare(1024, 2, 1, "generic-stage-strides"), Bare(1024, 3, 1, "generic-stage-dead-partner"),
    # the row count: one row, one more than a tile, two tiles and a tail; then several lines per workgroup with an odd last row
    Bare(12, 1, 1, "one-row"), Bare(12, 2, 1, "one-pair"), Bare(12, 5, 1, "two-tiles-and-a-row"), Bare(31, 1, 1, "one-row"),
    Bare(31, 5, 1, "two-tiles-and-a-row"), Bare(12, 513, 2, "odd-last-row"), Bare(31, 513, 2, "odd-last-row"),
    Bare(12, 1025, 3, "odd-last-row"), Bare(31, 1025, 3, "odd-last-row"), Bare(100, 513, 2, "generic-stage-multi-line"),
    Bare(12, 16385, 32, "ragged-last-tile"),
    # n = 255: the 32 KB budget holds 3 lines of P = 512, the row count asks for 4
    Bare(255, 1539, 3, "lds-budget-cap"),
    # in place at a multi-line shape
    Bare(12, 513, 2, "in-place", inplace=True), Bare(255, 1539, 3, "in-place-lds-budget-cap", inplace=True),
]


@dataclass(frozen=True)
class Structured:
    what: str
    planes: int
    hin: int                    # the image side (A reads it, A_adjoint writes it); 0: the 1-D form
    win: int
    hout: int
    wout: int
    layers: float               # layers + half / 2, as StructuredRandom counts them
    diag_planes: int = 0        # planes of one diagonal (diag_rows = diag_planes * H_work); 0: one per plane
    lines: int = 1
    emu: bool = True

    @property
    def id(self):
        g = f"{self.hin}x{self.win}-to-{self.hout}x{self.wout}" if self.hin else f"1d-{self.win}"
        return f"structured-{self.what}-p{self.planes}-{g}-layers{self.layers:g}-lines{self.lines}"


STRUCTURED = [
    Structured("equal", 4, 6, 12, 6, 12, 2),
    Structured("pad-rows", 4, 5, 12, 8, 12, 1),
    Structured("pad-cols", 4, 6, 9, 6, 12, 1.5),
    Structured("pad-both-odd-rows-even-cols", 4, 5, 8, 8, 12, 3),
    Structured("pad-both-even-rows-odd-cols", 4, 4, 9, 8, 12, 0.5),
    Structured("trim-rows", 4, 8, 12, 5, 12, 2),
    Structured("trim-cols", 4, 6, 12, 6, 9, 1),
    Structured("trim-both", 4, 8, 12, 5, 7, 1.5),
    Structured("1d", 5, 0, 31, 0, 31, 3),
    Structured("1d-half-only", 3, 0, 100, 0, 100, 0.5),
    # the header admits a geometry that grows along one axis and shrinks along the other: the working size is the larger side
    # per axis.  StructuredRandom refuses it, the entry point does not: pad per axis, then trim per axis
    Structured("mixed-pad-rows-trim-cols", 4, 5, 12, 8, 9, 2),
    Structured("mixed-trim-rows-pad-cols", 4, 8, 9, 5, 12, 1.5),
    # a diagonal of 2 planes under 6: row r uses diagonal row r % diag_rows and wraps twice
    Structured("diag-wraps", 6, 6, 12, 6, 12, 2, diag_planes=2),
    Structured("diag-wraps-padded", 6, 5, 8, 8, 12, 1, diag_planes=3),
    # an odd total row count: the last pair has a dead partner whose diagonal must not be read past the wrap
    Structured("diag-wraps-odd-rows", 3, 5, 12, 5, 12, 2, diag_planes=1),
    Structured("odd-rows-trimmed", 3, 7, 12, 5, 9, 1.5),
    # padded and large enough for two lines per workgroup: the zero fill of the padded rows (39804 floats over 129 workgroups of
    # 256 threads) runs grid-stride beside the multi-line tiles
    Structured("pad-multi-line-zero-fill-strides", 3, 172, 30, 600, 31, 1, lines=2),
    Structured("trim-multi-line", 3, 600, 31, 172, 30, 2, diag_planes=1, lines=2),
]
assert len({c.id for c in BARE + STRUCTURED}) == len(BARE) + len(STRUCTURED), "duplicate case ids"


def geometry(c, adjoint):
    """((H_in, W_in), (H_out, W_out), (H_work, W_work), top, left, diag_rows) of the call, as StructuredRandom builds them"""
    if not c.hin:
        return (1, c.win), (1, c.win), (1, c.win), 0, 0, c.diag_planes or c.planes
    work = (max(c.hin, c.hout), max(c.win, c.wout))
    top, left = math.ceil(abs(c.hin - c.hout) / 2), math.ceil(abs(c.win - c.wout) / 2)
    a, b = ((c.hout, c.wout), (c.hin, c.win)) if adjoint else ((c.hin, c.win), (c.hout, c.wout))
    return a, b, work, top, left, (c.diag_planes or c.planes) * work[0]


def _fit(t, size, off, dim):
    """pad or trim axis `dim` of t to `size`, the smaller side at offset `off` of the larger"""
    have = t.shape[dim]
    if have < size:
        shape = list(t.shape)
        shape[dim] = size
        out = t.new_zeros(shape)
        out.narrow(dim, off, have).copy_(t)
        return out
    return t.narrow(dim, off if have > size else 0, size)


def restated(x, diag, c, adjoint):
    """float64: pad per axis, ([F]; D_i, F ...) or its mirror, trim per axis.  x [planes, H_in, W_in], diag [L, diag_rows, W_work].
    Returns (the result [planes, H_out, W_out], the same before the trim [planes, H_work, W_work])"""
    (hi, wi), (ho, wo), (hw, ww), top, left, drows = geometry(c, adjoint)
    L, half = math.floor(c.layers), c.layers - math.floor(c.layers) == 0.5
    w = _fit(_fit(x.double(), hw, top, 1), ww, left, 2)
    S = sine(ww)
    idx = torch.arange(c.planes * hw) % drows
    D = [diag[i].double()[idx].view(c.planes, hw, ww) for i in range(L)]
    if not adjoint:
        if half:
            w = w @ S
        for i in range(L):
            w = (D[i] * w) @ S
    else:
        for i in range(L):
            w = D[L - 1 - i] * (w @ S)
        if half:
            w = w @ S
    return _fit(_fit(w, ho, top, 1), wo, left, 2), w


# ------------------------------------------------------------------ the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.dst), `device` of its buffers,
    `stream()` -> the stream argument, `fft_plan(n)` -> (plan struct, table tensor on the device) and - on the emulation -
    `reset()` / `launches()`, the launches since the last reset as "kernel xTHREADS" """

    def __init__(self, lib, device, stream, fft_plan, reset=None, launches=None):
        self.lib, self.device, self._stream, self.fft_plan = lib, torch.device(device), stream, fft_plan
        self.reset, self.launches = reset, launches

    def err(self):
        return self.lib.dinv_last_error().decode()

    def derived(self, n, transforms=1, diagonals=0):
        plan, _ = self.fft_plan(2 * (n + 1))
        cost = {4: 10, 8: 15}
        per = sum(cost.get(r, r + 3) for r in plan.radix[:plan.nstages]) + 2
        return (transforms * per + diagonals) * U

    def _logged(self, rc, what):
        if self.launches is not None:
            want = ["dst_tile_kernel x256"] if rc == 0 else []
            assert self.launches() == want, f"{what}: launched {self.launches()}, expected {want}"
        return rc

    def dst1(self, x_ptr, out_ptr, rows, n):
        plan, table = self.fft_plan(2 * (n + 1))
        if self.reset:
            self.reset()
        rc = self.lib.dinv_dst1(ctypes.c_void_p(x_ptr), ctypes.c_void_p(out_ptr), rows, n, ctypes.byref(plan),
                                ctypes.c_void_p(table.data_ptr()), self._stream())
        return self._logged(rc, "dst1")

    def structured(self, x, out, diag, c, adjoint):
        (hi, wi), (ho, wo), (hw, ww), top, left, drows = geometry(c, adjoint)
        L, half = math.floor(c.layers), int(c.layers - math.floor(c.layers) == 0.5)
        plan, table = self.fft_plan(2 * (ww + 1))
        if self.reset:
            self.reset()
        rc = self.lib.dinv_structured_apply(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                            ctypes.c_void_p(diag.data_ptr() if L else 0), c.planes, hi, wi, ho, wo, hw, ww, top,
                                            left, drows, L, half, int(adjoint), ctypes.byref(plan),
                                            ctypes.c_void_p(table.data_ptr()), self._stream())
        return self._logged(rc, "structured")


def _seed(cid):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(cid)) % (2 ** 31)


def worst_row(got, ref, full):
    """(max over rows g of ||got_g - ref_g|| / sqrt(||full_g||^2 + ||full_partner||^2), its row): rows [rows, *], the partner of
    row g in its complex transform is g ^ 1 where that row exists; NaN (an unwritten output) counts as infinite"""
    rows = ref.shape[0]
    num = (got.double() - ref).pow(2).sum(-1).sqrt()
    own = full.pow(2).sum(-1)
    partner = own[(torch.arange(rows) ^ 1).clamp_max(rows - 1)].clone()
    if rows % 2:
        partner[-1] = 0.0           # the last row of an odd count rides alone
    e = num / (own + partner).sqrt()
    if bool(torch.isnan(e).any()):
        return float("inf"), int(torch.isnan(e).nonzero()[0])
    return float(e.max()), int(e.argmax())


def run_bare(r, c):
    """runs one case of BARE on runner r, asserts everything it checks and returns the worst row error / bound"""
    assert lines_per_workgroup(c.rows, c.n) == c.lines, (c.id, lines_per_workgroup(c.rows, c.n))
    gen = torch.Generator().manual_seed(_seed(c.id))
    x = torch.randn(c.rows, c.n, generator=gen)
    words = c.rows * c.n
    xb = Guarded(words, r.device)
    xb.t.copy_(x.reshape(-1))
    ref = x.double() @ sine(c.n)
    bound = r.derived(c.n)
    if c.inplace:
        out = Guarded(words, r.device)
        assert r.dst1(xb.t.data_ptr(), out.t.data_ptr(), c.rows, c.n) == 0, r.err()
        assert r.dst1(xb.t.data_ptr(), xb.t.data_ptr(), c.rows, c.n) == 0, r.err()
        assert xb.guards_intact(), f"{c.id}: the in-place call wrote outside the tensor"
        assert torch.equal(xb.bits(), out.bits()), f"{c.id}: in place differs from out of place"
    else:
        out = Guarded(words, r.device)
        assert r.dst1(xb.t.data_ptr(), out.t.data_ptr(), c.rows, c.n) == 0, r.err()
        assert torch.equal(xb.t.cpu(), x.reshape(-1)) and xb.guards_intact(), f"{c.id}: the call modified its input"
        again = Guarded(words, r.device)
        assert r.dst1(xb.t.data_ptr(), again.t.data_ptr(), c.rows, c.n) == 0, r.err()
        assert again.guards_intact() and torch.equal(again.bits(), out.bits()), f"{c.id}: two identical calls differ"
    bits = out.bits()
    assert out.guards_intact(), f"{c.id}: write outside the output"
    assert not bool((bits == POISON).any()), f"{c.id}: {int((bits == POISON).sum())} outputs were never written"
    err, row = worst_row(out.t.cpu().view(c.rows, c.n), ref, ref)
    print(f"{c.id}: worst row {row} error {err:.3g} bound {bound:.3g} ratio {err / bound:.3g}")
    assert err <= bound, f"{c.id}: row {row} has error {err:.3g} > {bound:.3g}"
    return err / bound


def run_structured(r, c, adjoint):
    """runs one case of STRUCTURED as A or A_adjoint on runner r; returns the worst row error / bound"""
    (hi, wi), (ho, wo), (hw, ww), top, left, drows = geometry(c, adjoint)
    tag = f"{c.id}-{'At' if adjoint else 'A'}"
    htr = min(hi, ho)
    assert lines_per_workgroup(c.planes * htr, ww) == c.lines, (tag, lines_per_workgroup(c.planes * htr, ww))
    L, half = math.floor(c.layers), int(c.layers - math.floor(c.layers) == 0.5)
    gen = torch.Generator().manual_seed(_seed(tag))
    x = torch.randn(c.planes, hi, wi, generator=gen)
    diag = torch.where(torch.rand(max(L, 1), drows, ww, generator=gen) > 0.5, -1.0, 1.0)
    xb, db = Guarded(x.numel(), r.device), Guarded(L * drows * ww, r.device)
    xb.t.copy_(x.reshape(-1))
    db.t.copy_(diag[:L].reshape(-1))
    ref, full = restated(x, diag, c, adjoint)
    out = Guarded(c.planes * ho * wo, r.device)
    assert r.structured(xb.t, out.t, db.t, c, adjoint) == 0, f"{tag}: {r.err()}"
    bits = out.bits()
    assert out.guards_intact(), f"{tag}: write outside the output"
    assert xb.guards_intact() and db.guards_intact() and torch.equal(xb.t.cpu(), x.reshape(-1)), f"{tag}: an operand was modified"
    assert not bool((bits == POISON).any()), f"{tag}: {int((bits == POISON).sum())} outputs were never written"
    got = out.t.cpu().view(c.planes, ho, wo)
    again = Guarded(c.planes * ho * wo, r.device)
    assert r.structured(xb.t, again.t, db.t, c, adjoint) == 0, r.err()
    assert again.guards_intact() and torch.equal(again.bits(), bits), f"{tag}: two identical calls differ"
    # the rows that are transformed, in the order the kernel pairs them: row t of every plane's smaller side
    ro = top if ho > htr else 0
    rw = top if hw > htr else 0
    rows = c.planes * htr
    err, row = worst_row(got[:, ro:ro + htr].reshape(rows, wo), ref[:, ro:ro + htr].reshape(rows, wo),
                         full[:, rw:rw + htr].reshape(rows, ww))
    bound = r.derived(ww, L + half, L)
    print(f"{tag}: worst row {row} error {err:.3g} bound {bound:.3g} ratio {err / bound:.3g}")
    assert err <= bound, f"{tag}: transformed row {row} has error {err:.3g} > {bound:.3g}"
    if ho > htr:
        # the padded output rows meet no input row: zero in every bit, bar the sign
        padded = torch.ones(ho, dtype=torch.bool)
        padded[ro:ro + htr] = False
        assert bool((ref[:, padded] == 0).all())
        assert bool((got[:, padded].contiguous().view(torch.int32) & 0x7FFFFFFF == 0).all()), f"{tag}: a padded output row is not zero"
    if hi > htr:
        # the input rows the trim discards are never read: NaN there changes no bit
        xn = x.clone()
        dead = torch.ones(hi, dtype=torch.bool)
        dead[top:top + htr] = False
        xn[:, dead] = float("nan")
        xb.t.copy_(xn.reshape(-1))
        nan_out = Guarded(c.planes * ho * wo, r.device)
        assert r.structured(xb.t, nan_out.t, db.t, c, adjoint) == 0, r.err()
        assert bool(torch.isfinite(nan_out.t).all()), f"{tag}: a trimmed input row reached the output"
        xz = x.clone()
        xz[:, dead] = 0.0
        xb.t.copy_(xz.reshape(-1))
        zero_out = Guarded(c.planes * ho * wo, r.device)
        assert r.structured(xb.t, zero_out.t, db.t, c, adjoint) == 0, r.err()
        assert torch.equal(nan_out.bits(), zero_out.bits()) and torch.equal(zero_out.bits(), bits), \
            f"{tag}: the trimmed input rows changed the result"
    return err / bound


def run_rejections(r):
    """calls the entry points must refuse, with a message and without a launch or a write"""
    out = Guarded(2 * 8 * 12, r.device)
    x = Guarded(2 * 8 * 12, r.device)
    x.t.zero_()
    c = Structured("reject", 2, 8, 12, 8, 12, 0.5)
    assert r.structured(x.t, x.t, x.t, c, False) != 0 and "distinct" in r.err()
    for bad, msg in ((Structured("reject", 2, 8, 12, 8, 12, 0), "at least one transform"),):
        assert r.structured(x.t, out.t, x.t, bad, False) != 0 and msg in r.err(), r.err()
    if r.device.type == "cuda":
        torch.cuda.synchronize(r.device)
    assert out.untouched(), "a refused call wrote to its output"
