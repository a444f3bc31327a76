"""Shared by tests/test_complex_operator_kernels_gpu.py (the gfx950 library) and tests/test_emu_complex_operator_cases.py (the
same kernel sources on the host emulation): the case tables of csrc/cstructured.hip - the fused structured operator
(dinv_cstructured_apply) and ptychography (dinv_ptycho_apply) - the complex128 restatements, the Python restatement of the
launcher's rules (the LDS footprint and `fits`, the group / accumulator / workspace rules of ptychography) and the runner that
calls the C entry points on guarded buffers (tests/fft_cases.py Guarded): input, diagonals, probe, real array, output, workspace.

Bound of the structured operator, per element.  The derived bound of tests/phase_retrieval_cases.py derived_fft_bound: a radix-r
stage adds at most (r + 3) u to the relative l2 error of a line (radix 4 and 8 are two and three radix-2 levels), the scale and
a diagonal one u each; `per` is the sum over both axes plus the scale, u = 2^-24.  An element errs by at most the l2 error of
its plane, so |got - exact| <= (T per + D) u ||working plane||_2 with T transforms and D diagonals.  The norm is that of the
exact working plane before the trim; the diagonals are unit-modulus phases, so it is the same at every layer.  A misplaced
element errs by about ||plane|| / sqrt(H W), thousands of times this bound.

Exact cases.  Planes of sides 1, 2 and 4 have no twiddle multiply and a power-of-two scale: with Gaussian-integer inputs and
diagonals in {1, -1, i, -i} every operation is exact in fp32, and the result must equal the complex128 one bit for bit.

Epilogues.  The transform is bit-reproducible, so the value v an epilogue sees is the output of the NONE call on the same
inputs, and the fp32 epilogue is checked against the fp64 one of v: WEIGHT is one multiplication per part (bit-exact), ABS2 two
products and an addition (2 u), AMPLITUDE f = 1 - sqrt(y / (|v|^2 + eps)): s carries half of the 2 u of |v|^2 and of the u of
the division plus the u of the root (2.5 u s), the subtraction u |1 - s| and the product u |v f|: within |v| (4 u s + 2 u |1 - s|).

Ptychography.  Forward, per element: (per + 1) u ||p_l x_b||_2 (one transform, the probe product).  Adjoint, element e: the
inverse transform of y_bl errs by per u ||y_bl||_2, is multiplied by conj p_l(e) and summed over l in fp32:
sum_l |p_l(e)| per u ||y_bl||_2 + (L + 2) u sum_l |p_l(e)||w_l(e)| with w_l the exact inverse transform.  Normal: the adjoint
bound of t_l = f(F p_l x) with the error D_l of the computed t_l carried through the unitary inverse transform (an element of
F^-1 D is at most ||D||_2): sum_l |p_l(e)| (||D_l|| + per u (||t_l|| + ||D_l||)) + (L + 2) u sum_l |p_l(e)| (|w_l(e)| + ||D_l||),
where D_l is elementwise a |w| + u |z w| for WEIGHT (a the forward bound) and for AMPLITUDE
a |1 - s| + s a |z| / (|z| - a) + (|z| + a)(4 u s + 2 u |1 - s|) where |z| >= 8 a, and a + 2.01 sqrt(y) + 4 u (|z| + a)
elsewhere (|z s| <= sqrt(y) whatever z is).  The normal operation must also be bit for bit the adjoint operation applied to the
stored result of the forward operation with the same epilogue at the same group size."""
import ctypes
import math
from dataclasses import dataclass

import torch

from fft_cases import POISON, Guarded

U = 2.0 ** -24
THREADS, MAX_ACC, SMALL_ACC = 512, 20, 8
MAX_LDS, DEFAULT_LDS = 160 * 1024, 48 * 1024
EMU_CUS = 16                       # compute units of the emulated device (tests/emu/include/hip/hip_runtime.h)
NONE, ABS2, WEIGHT, AMPLITUDE = 0, 1, 2, 3
FORWARD, ADJOINT, NORMAL = 0, 1, 2
EPS = 1e-12
C128 = torch.complex128


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the launcher's rules, restated
def fft_line_stride(n):
    """csrc/fft_core.hpp fft_line_stride"""
    return n + 1 if n % 2 == 0 else n


def round_up16(b):
    return cdiv(b, 16) * 16


def fft_table_lds_bytes(n):
    """csrc/fft_core.hpp fft_table_lds_bytes: [tw n * 8][perm n * 4]"""
    return round_up16(n * 8 + round_up16(n * 4))


def buf_elems(H, W):
    return max(H * fft_line_stride(W), W * fft_line_stride(H))


def lds_bytes(H, W):
    return fft_table_lds_bytes(W) + fft_table_lds_bytes(H) + 2 * buf_elems(H, W) * 8


def fits(H, W):
    """dinv_cstructured_fits"""
    return H >= 1 and W >= 1 and H * W < (1 << 24) and lds_bytes(H, W) <= MAX_LDS


def radices(n):
    """the stages of dinv_fft_plan_init: generic primes outermost, then 5, 3, then the powers of two as 8s, a 4 or a 2"""
    m, e, pow2, small, primes = n, 0, [], [], []
    while m % 2 == 0:
        m, e = m // 2, e + 1
    pow2 = [8] * (e // 3) + ([4] if e % 3 == 2 else []) + ([2] if e % 3 == 1 else [])
    for q in (5, 3):
        while m % q == 0:
            small.append(q)
            m //= q
    q = 7
    while q * q <= m:
        while m % q == 0:
            primes.append(q)
            m //= q
        q += 2
    if m > 1:
        primes.append(m)
    return (primes + small + pow2) or [1]


def generic_stages(n):
    """stages of length n that ping-pong between the two buffers of tile_fft (radix 1 is one: a copy)"""
    return sum(r not in (2, 3, 4, 5, 8) for r in radices(n))


def accumulators(H, W):
    """ACC of ptycho_kernel<OP, ACC> for the adjoint and the normal operation"""
    return SMALL_ACC if H * W <= THREADS * SMALL_ACC else MAX_ACC


def ptycho_group(batch, L, H, W, group, cus):
    """positions per workgroup: csrc/cstructured.hip ptycho_group"""
    if group > 0:
        return min(group, L)
    per_cu = 2 if H * W <= THREADS * SMALL_ACC and 2 * lds_bytes(H, W) <= MAX_LDS else 1
    groups = min(cdiv(cus * per_cu, batch), L)
    return cdiv(L, groups)


def ptycho_groups(batch, L, H, W, op, group, cus):
    return 1 if op == FORWARD else cdiv(L, ptycho_group(batch, L, H, W, group, cus))


def ptycho_workspace_bytes(batch, L, H, W, op, group, cus):
    if batch < 1 or L < 1 or H < 1 or W < 1 or op == FORWARD:
        return 0
    g = ptycho_groups(batch, L, H, W, op, group, cus)
    return batch * g * H * W * 8 if g > 1 else 0


def ptycho_launches(batch, L, H, W, op, group, cus):
    acc = MAX_ACC if op == FORWARD else accumulators(H, W)
    reduce = ptycho_groups(batch, L, H, W, op, group, cus) > 1
    return [f"ptycho_kernel<{op}, {acc}> x{THREADS}"] + (["ptycho_reduce_kernel x256"] if reduce else [])


def widest(H):
    """the widest plane of H rows that fits"""
    W = 1
    while fits(H, W + 1) or fits(H, W + 2):
        W += 1 if fits(H, W + 1) else 2
    return W


def largest_fused_square():
    n = 1
    while fits(n + 1, n + 1):
        n += 1
    return n


# ------------------------------------------------------------------ the case tables
@dataclass(frozen=True)
class Structured:
    what: str
    planes: int
    hin: int                    # the side B reads and B^H writes
    win: int
    hout: int
    wout: int
    layers: float               # layers + half / 2, as StructuredRandomPhaseRetrieval counts them
    diag_planes: int = 0        # planes of one diagonal; 0: one per plane
    pos: str = "centre"         # where the smaller side lies in the working one: zero | centre (the class's) | far
    emu: bool = True

    @property
    def id(self):
        work = (max(self.hin, self.hout), max(self.win, self.wout))
        return (f"cstructured-{self.what}-p{self.planes}-{self.hin}x{self.win}-to-{self.hout}x{self.wout}-layers{self.layers:g}"
                f"-lds{lds_bytes(*work)}" + (f"-dp{self.diag_planes}" if self.diag_planes else "")
                + (f"-{self.pos}" if self.pos != "centre" else ""))


def _sq(what, H, W, planes=2, layers=2, **kw):
    return Structured(what, planes, H, W, H, W, layers, **kw)


SQUARE = largest_fused_square()
STRUCTURED = [
    # the geometry: pad or trim of rows only, columns only or both with odd and even differences; B^H of each runs the other way
    Structured("equal", 4, 12, 15, 12, 15, 2),
    Structured("pad-rows-odd", 3, 9, 16, 12, 16, 1),
    Structured("pad-cols-even", 3, 12, 12, 12, 16, 1.5),
    Structured("pad-both-odd-rows-even-cols", 4, 7, 12, 12, 16, 3),
    Structured("pad-both-even-rows-odd-cols", 4, 8, 11, 12, 16, 0.5),
    Structured("trim-rows", 3, 12, 16, 9, 16, 2),
    Structured("trim-cols", 3, 12, 16, 12, 12, 1),
    Structured("trim-both", 4, 12, 16, 7, 11, 1.5),
    # the header admits a geometry that grows along one axis and shrinks along the other: the working size is the larger side
    # per axis.  The class refuses it, the entry point does not: pad per axis, then trim per axis
    Structured("mixed-pad-rows-trim-cols", 4, 7, 16, 12, 11, 2),
    Structured("mixed-trim-rows-pad-cols", 4, 12, 11, 7, 16, 1.5),
    # the smaller side at the origin and flush to the far edge of the working plane
    Structured("pad-both", 2, 7, 11, 12, 16, 1, pos="zero"),
    Structured("pad-both", 2, 7, 11, 12, 16, 1, pos="far"),
    Structured("mixed-pad-rows-trim-cols", 2, 7, 16, 12, 11, 1, pos="zero"),
    Structured("mixed-pad-rows-trim-cols", 2, 7, 16, 12, 11, 1.5, pos="far"),
    # diagonals of 1, 2 and 3 planes under 6: plane p uses diagonal plane p % diag_planes; and one per plane
    Structured("diag-wraps", 6, 12, 16, 12, 16, 2, diag_planes=1),
    Structured("diag-wraps-padded", 6, 7, 12, 12, 16, 1, diag_planes=2),
    Structured("diag-wraps-trimmed", 6, 12, 16, 7, 11, 1.5, diag_planes=3),
    Structured("diag-per-plane", 6, 12, 16, 12, 16, 1, diag_planes=6),
    # 0, 1 and 2 generic-radix stages per axis (each swaps the two buffers of tile_fft) in every combination of H and W; two
    # and a half layers so that the ping-pong of plane_fft2 starts from either buffer
    _sq("generic-0-0", 12, 15), _sq("generic-0-1", 12, 7, layers=1.5), _sq("generic-0-2", 4, 49),
    _sq("generic-1-0", 11, 16, layers=1.5), _sq("generic-1-1", 7, 11), _sq("generic-1-2", 7, 49, layers=1.5),
    _sq("generic-2-0", 77, 12), _sq("generic-2-1", 49, 11, layers=1.5), _sq("generic-2-2", 49, 77),
    _sq("pow2", 2, 64, layers=3), _sq("pow2", 64, 2, layers=0.5), _sq("pow2", 16, 4, layers=1),
    # sides of 1 (a radix-1 stage, which is a generic one)
    _sq("one-row", 1, 16, planes=3), _sq("one-column", 16, 1, planes=3), _sq("one-element", 1, 1, planes=5, layers=1.5),
    _sq("one-row-generic", 1, 7, planes=3, layers=1), Structured("one-row-padded", 3, 1, 5, 1, 12, 1),
    Structured("one-element-padded", 3, 1, 1, 4, 15, 1.5),
    # the dynamic-LDS opt-in: the planes on either side of 48 KiB
    _sq("lds-default", 48, 48, layers=1), _sq("lds-default-last", 54, 54, layers=1.5), _sq("lds-optin-first", 55, 55, layers=1),
    _sq("lds-optin", 64, 64, layers=1.5),
    # the largest fused square, and thin planes at the limit of the LDS in both orientations
    _sq("largest-square", SQUARE, SQUARE, layers=1.5), Structured("largest-square-padded", 2, 50, 64, SQUARE, SQUARE, 1),
    _sq("thin", 3, 2500, layers=1), _sq("thin-widest", 3, widest(3), layers=1, emu=False),
    _sq("thin-tallest", widest(2), 2, layers=1.5), _sq("thin-widest-one-row", 1, widest(1), layers=1, emu=False),
]
assert len({c.id for c in STRUCTURED}) == len(STRUCTURED), "duplicate case ids"

EXACT = [Structured("exact", 3, H, W, H, W, 1.5, diag_planes=dp) for H, W, dp in ((1, 1, 0), (1, 4, 2), (4, 1, 0), (2, 2, 1), (4, 4, 0))]
EXACT += [Structured("exact-padded", 3, 2, 1, 4, 4, 2), Structured("exact-trimmed", 3, 4, 4, 1, 2, 1, pos="far")]


@dataclass(frozen=True)
class Ptycho:
    H: int
    W: int
    L: int
    batch: int
    cplx: bool                  # a complex probe with imaginary parts as large as the real ones, or a real one
    zero_plane: bool = False    # one probe plane is all zero
    only: tuple = ()            # the group arguments of the case where not all of `forced`
    emu: bool = True

    @property
    def id(self):
        return (f"ptycho-{self.H}x{self.W}-acc{accumulators(self.H, self.W)}-lds{lds_bytes(self.H, self.W)}-l{self.L}-b{self.batch}"
                + ("-complex" if self.cplx else "-real") + ("-zero-plane" if self.zero_plane else ""))

    @property
    def forced(self):
        """the group arguments of the case: automatic, 1, 2, (L + 1) / 2 (a last group of G - 1 positions), L - 1 (a last group
        of one position), L, L + 3"""
        return sorted(self.only or {0, 1, 2, (self.L + 1) // 2, max(self.L - 1, 1), self.L, self.L + 3})


PTYCHO = [
    Ptycho(16, 16, 5, 3, True), Ptycho(16, 16, 1, 1, False), Ptycho(16, 16, 9, 1, True, zero_plane=True),
    Ptycho(12, 20, 9, 1, False), Ptycho(12, 20, 2, 3, True),
    Ptycho(33, 22, 5, 1, True, zero_plane=True), Ptycho(33, 22, 2, 3, False),
    # around the accumulator switch at 4096 elements and the LDS opt-in
    Ptycho(63, 65, 2, 1, True), Ptycho(64, 64, 5, 3, False, emu=False), Ptycho(64, 64, 2, 1, True), Ptycho(50, 82, 5, 1, True, emu=False),
    Ptycho(50, 82, 2, 3, False),
    Ptycho(1, 64, 5, 3, True), Ptycho(64, 1, 9, 1, False),
    # a batch that leaves the 16 compute units of the emulation fewer workgroups than positions: automatic groups of two
    Ptycho(64, 1, 9, 7, True, only=(0,)),
    # the largest fused square: 9801 elements, the 20th accumulator of a thread is used by 73 threads of 512
    Ptycho(SQUARE, SQUARE, 2, 1, True), Ptycho(SQUARE, SQUARE, 5, 1, False, emu=False),
]
assert len({c.id for c in PTYCHO}) == len(PTYCHO), "duplicate case ids"


def check_structured_table():
    """the structured table itself reaches what it is meant to"""
    C = STRUCTURED
    work = lambda c: (max(c.hin, c.hout), max(c.win, c.wout))
    assert {c.layers for c in C} == {0.5, 1, 1.5, 2, 3} and all(2 <= c.planes <= 6 for c in C)
    swaps = {(min(generic_stages(work(c)[0]), 2), min(generic_stages(work(c)[1]), 2)) for c in C}
    assert swaps == {(a, b) for a in range(3) for b in range(3)}
    assert {generic_stages(n) for n in (2, 4, 12, 15, 16, 64)} == {0} and {generic_stages(n) for n in (1, 7, 11)} == {1}
    assert {generic_stages(n) for n in (49, 77)} == {2}
    sides = {s for c in C for s in work(c)}
    assert sides >= {1, 2, 4, 12, 15, 16, 7, 11, 49, 77, 64}
    assert {c.pos for c in C} == {"zero", "centre", "far"}
    assert {c.diag_planes for c in C if c.planes == 6} == {1, 2, 3, 6}
    kinds = set()
    for c in C:
        dh, dw = c.hout - c.hin, c.wout - c.win
        kinds.add(((dh > 0) - (dh < 0), (dw > 0) - (dw < 0), abs(dh) % 2, abs(dw) % 2))
    for sh, sw in ((1, 0), (0, 1), (1, 1), (-1, 0), (0, -1), (-1, -1), (1, -1), (-1, 1)):
        assert any(k[:2] == (sh, sw) for k in kinds), (sh, sw)
    assert (1, 1, 1, 0) in kinds and (1, 1, 0, 1) in kinds
    assert any(work(c) == (1, 1) for c in C) and any(work(c)[0] == 1 < work(c)[1] for c in C)
    assert any(work(c)[1] == 1 < work(c)[0] for c in C)
    # the last plane under the 48 KiB default and the first over it, the largest square, thin planes within 1 % of the limit
    assert any(lds_bytes(*work(c)) <= DEFAULT_LDS < lds_bytes(work(c)[0] + 1, work(c)[1] + 1) for c in C)
    assert any(lds_bytes(work(c)[0] - 1, work(c)[1] - 1) <= DEFAULT_LDS < lds_bytes(*work(c)) for c in C)
    assert SQUARE == 99 and any(work(c) == (SQUARE, SQUARE) for c in C) and not fits(SQUARE + 1, SQUARE + 1)
    assert sum(min(work(c)) <= 3 and lds_bytes(*work(c)) > 0.99 * MAX_LDS for c in C) >= 3
    assert all(fits(*work(c)) for c in C + EXACT)
    assert {work(c) for c in EXACT} >= {(1, 1), (1, 4), (4, 1), (2, 2), (4, 4)}


def check_ptycho_table():
    """the ptychography table itself reaches what it is meant to"""
    C = PTYCHO
    assert {c.L for c in C} == {1, 2, 5, 9} and {c.batch for c in C} >= {1, 3} and {c.cplx for c in C} == {False, True}
    assert {(c.H, c.W) for c in C} == {(16, 16), (12, 20), (33, 22), (63, 65), (64, 64), (50, 82), (1, 64), (64, 1), (SQUARE, SQUARE)}
    assert {c.H * c.W for c in C} >= {4095, 4096, 4100}
    for acc in (SMALL_ACC, MAX_ACC):
        mine = [c for c in C if accumulators(c.H, c.W) == acc]
        assert {c.cplx for c in mine} == {False, True} and {c.L for c in mine} >= {2, 5} and {c.batch for c in mine} >= {1, 3}
    assert accumulators(64, 64) == 8 and accumulators(63, 65) == 8 and accumulators(50, 82) == 20
    assert (MAX_ACC - 1) * THREADS < SQUARE * SQUARE < MAX_ACC * THREADS        # the 20th accumulator is partly used
    assert any(lds_bytes(c.H, c.W) <= DEFAULT_LDS for c in C) and any(lds_bytes(c.H, c.W) > DEFAULT_LDS for c in C)
    assert any(generic_stages(c.H) or generic_stages(c.W) for c in C) and any(c.zero_plane for c in C)
    ragged = {(c.L % g) for c in C for g in c.forced if 0 < g < c.L and c.L % g}
    assert 1 in ragged and any(c.L % g == g - 1 and g > 2 for c in C for g in c.forced if 0 < g < c.L)
    assert all(c.L + 3 in c.forced and 0 in c.forced and 1 in c.forced and c.L in c.forced for c in C if not c.only)
    # the emulation's 16 compute units: automatic groups of one position almost everywhere, and of several for the batch of 7
    assert any(ptycho_group(c.batch, c.L, c.H, c.W, 0, EMU_CUS) > 1 for c in C)
    assert any(ptycho_groups(c.batch, c.L, c.H, c.W, ADJOINT, 0, EMU_CUS) > 1 for c in C)


def check_groups_at_256():
    cus = 256
    # two workgroups a compute unit where two planes of at most 4096 elements fit its LDS, one otherwise
    assert ptycho_group(300, 9, 64, 64, 0, cus) == 5 and ptycho_group(300, 9, 50, 82, 0, cus) == 9
    assert ptycho_group(100, 9, 64, 64, 0, cus) == 2 and ptycho_group(100, 9, 50, 82, 0, cus) == 3
    assert ptycho_group(600, 9, 16, 16, 0, cus) == 9 and ptycho_group(512, 9, 16, 16, 0, cus) == 9
    assert ptycho_group(511, 9, 16, 16, 0, cus) == 5
    assert 2 * lds_bytes(64, 64) <= MAX_LDS and 2 * lds_bytes(63, 65) <= MAX_LDS
    for c in PTYCHO:
        # the table's batches leave every position its own workgroup on the device
        assert ptycho_group(c.batch, c.L, c.H, c.W, 0, cus) == 1
        for g in c.forced:
            for op in (ADJOINT, NORMAL):
                groups = ptycho_groups(c.batch, c.L, c.H, c.W, op, g, cus)
                assert groups == cdiv(c.L, min(g, c.L) if g else 1)
                assert ptycho_workspace_bytes(c.batch, c.L, c.H, c.W, op, g, cus) == (c.batch * groups * c.H * c.W * 8 if groups > 1 else 0)
            assert ptycho_workspace_bytes(c.batch, c.L, c.H, c.W, FORWARD, g, cus) == 0


# ------------------------------------------------------------------ the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.cstructured and .ptycho),
    `device` of its buffers, `stream()` -> the stream argument, `fft_plan(n)` -> (plan struct, table tensor on the device), `cus`
    the compute units of the device and - on the emulation - `reset()` / `launches()`, the launches since the last reset as
    "instance xTHREADS" """

    def __init__(self, lib, device, stream, fft_plan, cus, reset=None, launches=None):
        self.lib, self.device, self._stream, self.fft_plan, self.cus = lib, torch.device(device), stream, fft_plan, int(cus)
        self.reset, self.launches = reset, launches

    def err(self):
        return self.lib.dinv_last_error().decode()

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def per(self, H, W):
        """the `per` of phase_retrieval_cases.derived_fft_bound from the plans of this library, which must be the restated ones"""
        cost = {4: 10, 8: 15}
        per = 1
        for n in (H, W):
            plan, _ = self.fft_plan(n)
            stages = list(plan.radix[:plan.nstages])
            assert stages == radices(n), (n, stages, radices(n))
            per += sum(cost.get(r, r + 3) for r in stages)
        return per

    def _check_log(self, what, rc, want):
        if self.launches is not None:
            want = want if rc == 0 else []
            assert self.launches() == want, f"{what}: launched {self.launches()}, the restated dispatch expects {want}"
        return rc

    def cstructured_raw(self, x, out, diag, aux, planes, hi, wi, ho, wo, hw, ww, top, left, dplanes, L, half, adjoint, epilogue,
                        plan_w=None, plan_h=None, launches=1):
        pw, tw = self.fft_plan(plan_w or ww)
        ph, th = self.fft_plan(plan_h or hw)
        if self.reset:
            self.reset()
        vp = ctypes.c_void_p
        rc = self.lib.dinv_cstructured_apply(vp(x), vp(out), vp(diag), vp(aux), planes, hi, wi, ho, wo, hw, ww, top, left, dplanes, L,
                                             half, int(adjoint), epilogue, EPS, ctypes.byref(pw), vp(tw.data_ptr()), ctypes.byref(ph),
                                             vp(th.data_ptr()), self._stream())
        return self._check_log("cstructured", rc, ["cstructured_plane_kernel x512"] * launches)

    def ptycho_workspace_bytes(self, batch, L, H, W, op, group):
        return int(self.lib.dinv_ptycho_workspace_bytes(batch, L, H, W, op, group))

    def ptycho_raw(self, x, out, probe, cplx, aux, batch, L, H, W, op, epilogue, group, ws, ws_bytes, plan_w=None, plan_h=None):
        pw, tw = self.fft_plan(plan_w or W)
        ph, th = self.fft_plan(plan_h or H)
        if self.reset:
            self.reset()
        vp = ctypes.c_void_p
        rc = self.lib.dinv_ptycho_apply(vp(x), vp(out), vp(probe), int(cplx), vp(aux), batch, L, H, W, op, epilogue, EPS, group,
                                        ctypes.byref(pw), vp(tw.data_ptr()), ctypes.byref(ph), vp(th.data_ptr()), vp(ws), ws_bytes,
                                        self._stream())
        want = ptycho_launches(batch, L, H, W, op, group, self.cus) if batch > 0 and rc == 0 else []
        return self._check_log("ptycho", rc, want)


def _seed(cid):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(cid)) % (2 ** 31)


def _randc(gen, *shape):
    return torch.complex(torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen))


def _guarded(r, t):
    """a guarded device copy of tensor t (complex as interleaved pairs) and its bits"""
    t = torch.view_as_real(t.to(torch.complex64).contiguous()) if t.is_complex() else t.float()
    g = Guarded(t.numel(), r.device)
    g.t.copy_(t.reshape(-1))
    return g, g.bits().clone()


def _complex(bits, shape):
    return torch.view_as_complex(bits.view(torch.float32).view(*shape, 2))


def twice(r, tag, words, ws_words, call, operands, reduced=False):
    """`call(out, ws)` of runner r on two fresh guarded outputs and workspaces: status 0, guards intact, every word written, identical bits,
    operands (pairs of a Guarded and its bits) unchanged.  Returns the bits of the output."""
    results = []
    for _ in range(2):
        out, ws = Guarded(words, r.device), Guarded(ws_words, r.device)
        rc = call(out, ws)
        assert rc == 0, f"{tag}: error {rc}: {r.err()}"
        bits = out.bits()
        assert out.guards_intact(), f"{tag}: write outside the output"
        assert ws.guards_intact(), f"{tag}: write outside the workspace"
        assert not bool((bits == POISON).any()), (f"{tag}: {int((bits == POISON).sum())} output words hold the guard pattern: never "
                                                  "written, or computed from a read outside the operands")
        if reduced:
            assert not bool((ws.bits() == POISON).any()), f"{tag}: a group left part of its partial plane unwritten"
        results.append(bits.clone())
    assert torch.equal(results[0], results[1]), f"{tag}: two identical calls differ"
    for g, before in operands:
        assert g.guards_intact() and torch.equal(g.bits(), before), f"{tag}: the call modified an operand"
    return results[0]


def _ratio(tag, err, bound):
    """the worst err / bound over the elements; where the bound is zero the error must be"""
    assert not bool(torch.isnan(err).any()), f"{tag}: NaN in the result"
    zero = bound == 0
    assert bool((err[zero] == 0).all()), f"{tag}: an element that is exactly zero is not"
    ratio = torch.where(zero, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max())
    at = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
    print(f"{tag}: worst element {at} error / bound {worst:.3g}")
    assert worst <= 1.0, f"{tag}: element {at} is {worst:.3g} times its bound"
    return worst


def measurements(v2, gen, zero_where=None):
    """fp32 measurements for the AMPLITUDE epilogue of values with |v|^2 = v2: up to 2 |v|^2, a fifth of them zero; on the
    elements of `zero_where` (where v is zero) positive numbers and zeros instead"""
    y = (v2 * torch.rand(v2.shape, generator=gen).double() * 2).float()
    if zero_where is not None:
        y[zero_where] = (torch.rand(v2.shape, generator=gen) + 0.5)[zero_where]
    y.view(-1)[::5] = 0.0
    return y


def check_epilogues(tag, v, run, gen, zero_where=None):
    """ABS2, WEIGHT and AMPLITUDE against the fp64 epilogue of v, the kernel's own NONE output (complex64 on the CPU).
    run(epilogue, aux) -> the bits of the output.  Returns the worst error / bound of ABS2 and of AMPLITUDE."""
    vd = v.to(C128)
    v2 = vd.abs().square()
    got = run(ABS2, None).view(torch.float32).view(v.shape).double()
    worst = {"abs2": _ratio(f"{tag} abs2", (got - v2).abs(), 2 * U * v2)}
    w = torch.randn(v.shape, generator=gen)
    got = _complex(run(WEIGHT, w), v.shape)
    assert torch.equal(torch.view_as_real(got), torch.stack((v.real * w, v.imag * w), -1)), f"{tag} weight: not the fp32 product"
    y = measurements(v2, gen, zero_where)
    got = _complex(run(AMPLITUDE, y), v.shape)
    assert bool(torch.isfinite(torch.view_as_real(got)).all()), f"{tag} amplitude: not finite"
    s = torch.sqrt(y.double() / (v2 + float(torch.tensor(EPS, dtype=torch.float32))))
    va = vd.abs()
    worst["amplitude"] = _ratio(f"{tag} amplitude", (got.to(C128) - vd * (1 - s)).abs(), va * (4 * U * s + 2 * U * (1 - s).abs()))
    zero = y == 0
    assert bool(zero.any()) and torch.equal(torch.view_as_real(got)[zero], torch.view_as_real(v)[zero]), \
        f"{tag} amplitude: where y = 0 the result is v itself"
    return worst


# ------------------------------------------------------------------ the structured operator
def geometry(c, adjoint):
    """((H_in, W_in), (H_out, W_out), (H_work, W_work), top, left, diag_planes) of the call"""
    work = (max(c.hin, c.hout), max(c.win, c.wout))
    off = lambda d: {"zero": 0, "centre": math.ceil(d / 2), "far": d}[c.pos]
    top, left = off(abs(c.hin - c.hout)), off(abs(c.win - c.wout))
    a, b = ((c.hout, c.wout), (c.hin, c.win)) if adjoint else ((c.hin, c.win), (c.hout, c.wout))
    return a, b, work, top, left, c.diag_planes or c.planes


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


def _dft(n, inverse):
    """the DFT matrix of length 1, 2 or 4 with exact entries"""
    w = [1, -1j, -1, 1j] if not inverse else [1, 1j, -1, -1j]
    return torch.tensor([[w[(j * k * (4 // n)) % 4] for k in range(n)] for j in range(n)], dtype=C128)


def _fft2(t, inverse, exact):
    """the orthonormal 2-D transform in complex128; `exact`: by the exact matrices of sides 1, 2, 4 and a power-of-two scale"""
    if not exact:
        return torch.fft.ifft2(t, norm="ortho") if inverse else torch.fft.fft2(t, norm="ortho")
    H, W = t.shape[-2:]
    return (_dft(H, inverse) @ t @ _dft(W, inverse)) * (1.0 / math.sqrt(H * W))


def restated(x, diag, c, adjoint, exact=False):
    """complex128: pad per axis, ([F]; D_i, F ...) or its mirror, trim per axis.  x [planes, H_in, W_in], diag [L, diag_planes,
    H_work, W_work].  Returns (the result [planes, H_out, W_out], the same before the trim [planes, H_work, W_work])"""
    (hi, wi), (ho, wo), (hw, ww), top, left, dplanes = geometry(c, adjoint)
    L, half = math.floor(c.layers), c.layers - math.floor(c.layers) == 0.5
    w = _fit(_fit(x.to(C128), hw, top, 1), ww, left, 2)
    D = [diag[i].to(C128)[torch.arange(c.planes) % dplanes] for i in range(L)]
    if not adjoint:
        if half:
            w = _fft2(w, False, exact)
        for i in range(L):
            w = _fft2(D[i] * w, False, exact)
    else:
        for i in range(L):
            w = D[L - 1 - i].conj() * _fft2(w, True, exact)
        if half:
            w = _fft2(w, True, exact)
    return _fit(_fit(w, ho, top, 1), wo, left, 2), w


def _structured_call(r, c, adjoint, xb, db, epilogue=NONE, ab=None):
    (hi, wi), (ho, wo), (hw, ww), top, left, dplanes = geometry(c, adjoint)
    L, half = math.floor(c.layers), int(c.layers - math.floor(c.layers) == 0.5)
    return (lambda out, ws: r.cstructured_raw(xb.t.data_ptr(), out.t.data_ptr(), db.t.data_ptr() if L else 0,
                                                      ab.t.data_ptr() if ab else 0, c.planes, hi, wi, ho, wo, hw, ww, top, left,
                                                      dplanes, L, half, adjoint, epilogue))


def _structured_operands(c, adjoint, gen, exact):
    (hi, wi), _, (hw, ww), _, _, dplanes = geometry(c, adjoint)
    L = math.floor(c.layers)
    if exact:
        ri = lambda *shape: torch.randint(-4, 5, shape, generator=gen).float()
        x = torch.complex(ri(c.planes, hi, wi), ri(c.planes, hi, wi))
        units = torch.tensor([1, 1j, -1, -1j], dtype=torch.complex64)
        diag = units[torch.randint(0, 4, (max(L, 1), dplanes, hw, ww), generator=gen)]
    else:
        x = _randc(gen, c.planes, hi, wi)
        diag = torch.polar(torch.ones(max(L, 1), dplanes, hw, ww), torch.rand(max(L, 1), dplanes, hw, ww, generator=gen) * 2 * math.pi)
    return x.to(torch.complex64), diag[:L].to(torch.complex64)


def run_structured(r, c, adjoint):
    """runs one case of STRUCTURED as B or B^H on runner r; returns the worst element error / bound of the
    transforms and of the epilogues"""
    (hi, wi), (ho, wo), (hw, ww), top, left, dplanes = geometry(c, adjoint)
    assert lds_bytes(hw, ww) <= MAX_LDS
    tag = f"{c.id}-{'Bh' if adjoint else 'B'}"
    L, half = math.floor(c.layers), int(c.layers - math.floor(c.layers) == 0.5)
    gen = torch.Generator().manual_seed(_seed(tag))
    x, diag = _structured_operands(c, adjoint, gen, False)
    (xb, xbits), (db, dbits) = _guarded(r, x), _guarded(r, diag)
    ref, full = restated(x, diag, c, adjoint)
    shape, n = (c.planes, ho, wo), c.planes * ho * wo
    bits = twice(r, tag, 2 * n, 0, _structured_call(r, c, adjoint, xb, db), [(xb, xbits), (db, dbits)])
    v = _complex(bits, shape)
    norm = torch.linalg.vector_norm(full, dim=(1, 2)).view(-1, 1, 1)
    bound = ((L + half) * r.per(hw, ww) + L) * U * norm.expand(shape)
    worst = _ratio(tag, (v.to(C128) - ref).abs(), bound)

    def run(epilogue, aux):
        ab, abits = _guarded(r, aux) if aux is not None else (None, None)
        ops = [(xb, xbits), (db, dbits)] + ([(ab, abits)] if ab else [])
        return twice(r, f"{tag} epilogue {epilogue}", n * (1 if epilogue == ABS2 else 2), 0,
                     _structured_call(r, c, adjoint, xb, db, epilogue, ab), ops)

    return {"transform": worst, **check_epilogues(tag, v, run, gen)}


def run_exact(r, c, adjoint):
    """Gaussian integers through planes of sides 1, 2 and 4: bit for bit the complex128 result"""
    (hi, wi), (ho, wo), (hw, ww), top, left, dplanes = geometry(c, adjoint)
    assert {hw, ww} <= {1, 2, 4}
    tag = f"{c.id}-{'Bh' if adjoint else 'B'}"
    gen = torch.Generator().manual_seed(_seed(tag))
    x, diag = _structured_operands(c, adjoint, gen, True)
    (xb, xbits), (db, dbits) = _guarded(r, x), _guarded(r, diag)
    ref, _ = restated(x, diag, c, adjoint, exact=True)
    bits = twice(r, tag, 2 * c.planes * ho * wo, 0, _structured_call(r, c, adjoint, xb, db), [(xb, xbits), (db, dbits)])
    got = _complex(bits, (c.planes, ho, wo)).to(C128)
    wrong = (got.real != ref.real) | (got.imag != ref.imag)
    assert bool((ref != 0).any()) and not bool(wrong.any()), \
        f"{tag}: {int(wrong.sum())} of {wrong.numel()} outputs are not exact, the first at {tuple(int(i) for i in wrong.nonzero()[0])}"


def run_fits_scan(r):
    l = r.lib
    for H in range(1, 11001):
        for W in range(1, 11000 // H + 1):
            f = fits(H, W)
            assert f == bool(l.dinv_cstructured_fits(H, W)), (H, W)
            assert not f or H * W <= THREADS * MAX_ACC, (H, W)
    assert not l.dinv_cstructured_fits(0, 4) and not l.dinv_cstructured_fits(4, 0) and not l.dinv_cstructured_fits(4096, 4096)
    n = 1
    while l.dinv_cstructured_fits(n + 1, n + 1):
        n += 1
    assert n == largest_fused_square() == SQUARE and 90 <= n <= 110


def run_structured_rejections(r):
    """calls dinv_cstructured_apply must refuse: a non-zero status, the reason in dinv_last_error, no launch and no write"""
    P, H, W = 2, 8, 12
    x, d, aux = Guarded(2 * P * H * W, r.device), Guarded(2 * P * H * W, r.device), Guarded(P * H * W, r.device)
    for b in (x, d, aux):
        b.t.zero_()
    out = Guarded(2 * P * H * W, r.device)
    X, D, A, O = (b.t.data_ptr() for b in (x, d, aux, out))
    too_big = SQUARE + 1
    #        x  out diag aux  in      out     work     top left dp L half epilogue plans        reason
    bad = [(X, O, D, 0, (5, 12), (8, 12), (8, 13), 1, 0, P, 1, 0, NONE, (None, None), "working size"),
           (X, O, D, 0, (5, 12), (8, 9), (8, 9), 1, 0, P, 1, 0, NONE, (None, None), "working size"),
           (X, O, D, 0, (5, 12), (8, 12), (8, 12), 4, 0, P, 1, 0, NONE, (None, None), "offsets"),
           (X, O, D, 0, (8, 12), (8, 9), (8, 12), 0, 4, P, 1, 0, NONE, (None, None), "offsets"),
           (X, O, D, 0, (5, 12), (8, 12), (8, 12), -1, 0, P, 1, 0, NONE, (None, None), "offsets"),
           (X, O, 0, 0, (8, 12), (8, 12), (8, 12), 0, 0, P, 1, 0, NONE, (None, None), "without diagonals"),
           (X, O, D, 0, (8, 12), (8, 12), (8, 12), 0, 0, 0, 1, 0, NONE, (None, None), "without diagonals"),
           (X, O, 0, 0, (8, 12), (8, 12), (8, 12), 0, 0, P, 0, 0, NONE, (None, None), "at least one transform"),
           (X, O, D, 0, (8, 12), (8, 12), (8, 12), 0, 0, P, 1, 2, NONE, (None, None), "at least one transform"),
           (O, O, D, 0, (8, 12), (8, 12), (8, 12), 0, 0, P, 1, 0, NONE, (None, None), "distinct"),
           (X, O, D, 0, (8, 12), (8, 12), (8, 12), 0, 0, P, 1, 0, NONE, (16, None), "plans are for lengths"),
           (X, O, D, 0, (8, 12), (8, 12), (8, 12), 0, 0, P, 1, 0, NONE, (None, 12), "plans are for lengths"),
           (X, O, D, 0, (too_big,) * 2, (too_big,) * 2, (too_big,) * 2, 0, 0, P, 1, 0, NONE, (None, None), "LDS"),
           (X, O, D, 0, (8, 12), (8, 12), (8, 12), 0, 0, P, 1, 0, WEIGHT, (None, None), "needs a real array"),
           (X, O, D, O, (8, 12), (8, 12), (8, 12), 0, 0, P, 1, 0, AMPLITUDE, (None, None), "needs a real array"),
           (X, O, D, A, (8, 12), (8, 12), (8, 12), 0, 0, P, 1, 0, 4, (None, None), "unknown epilogue"),
           (X, O, D, 0, (0, 12), (8, 12), (8, 12), 0, 0, P, 1, 0, NONE, (None, None), "empty side")]
    for xp, op, dp_, ap, (hi, wi), (ho, wo), (hw, ww), top, left, dplanes, L, half, ep, (pw, ph), why in bad:
        rc = r.cstructured_raw(xp, op, dp_, ap, P, hi, wi, ho, wo, hw, ww, top, left, dplanes, L, half, 0, ep, pw, ph)
        assert rc != 0 and why in r.err(), f"cstructured ({why}): status {rc}, message {r.err()!r}"
    r.sync()
    assert out.untouched(), "a refused cstructured call wrote to its output"
    # no planes: nothing to do, whatever the pointers
    assert r.cstructured_raw(0, 0, 0, 0, 0, 8, 12, 8, 12, 8, 12, 0, 0, 1, 1, 0, 0, NONE, launches=0) == 0, r.err()


# ------------------------------------------------------------------ ptychography
def _ptycho_data(c, gen):
    B, L, H, W = c.batch, c.L, c.H, c.W
    x = _randc(gen, B, H, W).to(torch.complex64)
    probe = (_randc(gen, L, H, W) if c.cplx else torch.randn(L, H, W, generator=gen))
    probe = probe.to(torch.complex64 if c.cplx else torch.float32)
    if c.zero_plane:
        probe[L // 2] = 0
    yadj = _randc(gen, B, L, H, W).to(torch.complex64)
    return x, probe, yadj


def _adjoint_bound(P, per, t, dt):
    """the bound of sum_l conj(p_l) F^-1 t_l per element: P [L, H, W] complex128, t [B, L, H, W] exact, dt [B, L] the l2 error of
    the computed t_l (zero for the adjoint operation itself)"""
    L = P.shape[0]
    w = torch.fft.ifft2(t, norm="ortho")
    tn = torch.linalg.vector_norm(t, dim=(2, 3))
    pa = P.abs().unsqueeze(0)
    line = (dt + per * U * (tn + dt)).view(*dt.shape, 1, 1)
    return (pa * line).sum(1) + (L + 2) * U * (pa * (w.abs() + dt.view(*dt.shape, 1, 1))).sum(1)


def run_ptycho(r, c):
    """runs one case of PTYCHO on runner r - the forward operation with its four epilogues, then for every group argument of
    the case the adjoint and the two normal operations; returns the worst element error / bound of each kind of check"""
    B, L, H, W = c.batch, c.L, c.H, c.W
    n, shape = B * L * H * W, (B, L, H, W)
    gen = torch.Generator().manual_seed(_seed(c.id))
    x, probe, yadj = _ptycho_data(c, gen)
    (xb, xbits), (pb, pbits), (yb, ybits) = _guarded(r, x), _guarded(r, probe), _guarded(r, yadj)
    P = probe.to(C128)
    per = r.per(H, W)
    PX = P.unsqueeze(0) * x.to(C128).unsqueeze(1)
    Z = torch.fft.fft2(PX, norm="ortho")
    a = (per + 1) * U * torch.linalg.vector_norm(PX, dim=(2, 3))                 # [B, L]: the forward bound of a plane
    zero_where = torch.zeros(shape, dtype=torch.bool)
    if c.zero_plane:
        zero_where[:, L // 2] = True

    def call(src, op, epilogue, group, ab, ws_bytes):
        return (lambda out, ws: r.ptycho_raw(src.t.data_ptr(), out.t.data_ptr(), pb.t.data_ptr(), c.cplx,
                                                     ab.t.data_ptr() if ab else 0, B, L, H, W, op, epilogue, group,
                                                     ws.t.data_ptr() if ws.n else 0, ws_bytes))

    def forward(epilogue, aux):
        ab, abits = _guarded(r, aux) if aux is not None else (None, None)
        ops = [(xb, xbits), (pb, pbits)] + ([(ab, abits)] if ab else [])
        assert r.ptycho_workspace_bytes(B, L, H, W, FORWARD, 0) == 0
        return twice(r, f"{c.id} forward epilogue {epilogue}", n * (1 if epilogue == ABS2 else 2), 0,
                     call(xb, FORWARD, epilogue, 0, ab, 0), ops)

    # ---- forward
    v = _complex(forward(NONE, None), shape)
    worst = {"forward": _ratio(f"{c.id} forward", (v.to(C128) - Z).abs(), a.view(B, L, 1, 1).expand(shape)), "adjoint": 0.0, "normal": 0.0}
    worst.update(check_epilogues(f"{c.id} forward", v, forward, gen, zero_where if c.zero_plane else None))
    if c.zero_plane:
        y0 = measurements(Z.abs().square(), gen, zero_where)
        assert bool((y0[zero_where] > 0).any()) and bool((y0[zero_where] == 0).any())
        got = _complex(forward(AMPLITUDE, y0), shape)
        assert bool(torch.isfinite(torch.view_as_real(got)).all()) and bool((got[zero_where] == 0).all()), \
            f"{c.id}: AMPLITUDE on a plane whose probe is zero is not exactly zero"
    # ---- the real arrays of the normal operation, their stored forward results and the fp64 bounds
    wts = torch.randn(shape, generator=gen)
    meas = measurements(Z.abs().square(), gen, zero_where if c.zero_plane else None)
    za, wd = Z.abs(), wts.double()
    A = a.view(B, L, 1, 1)
    s = torch.sqrt(meas.double() / (za.square() + EPS))
    covered = (za >= 8 * A) & (za > 0)
    d_cov = A * (1 - s).abs() + s * A * za / (za - A).clamp_min(1e-300) + (za + A) * (4 * U * s + 2 * U * (1 - s).abs())
    d_amp = torch.where(covered, d_cov, A + 2.01 * meas.double().sqrt() + 4 * U * (za + A))
    stages = {WEIGHT: (wts, Z * wd, A * wd.abs() + U * (Z * wd).abs()), AMPLITUDE: (meas, Z * (1 - s), d_amp)}
    stored = {}
    for ep, (aux, _, _) in stages.items():
        stored[ep] = _guarded(r, _complex(forward(ep, aux), shape))
    # ---- adjoint and normal at every group argument
    hw2 = 2 * B * H * W
    for group in c.forced:
        for op in (ADJOINT, NORMAL):
            assert r.ptycho_workspace_bytes(B, L, H, W, op, group) == ptycho_workspace_bytes(B, L, H, W, op, group, r.cus), \
                f"{c.id} group {group}: workspace bytes against the restated rule at {r.cus} compute units"
        nbytes = ptycho_workspace_bytes(B, L, H, W, ADJOINT, group, r.cus)
        G = ptycho_group(B, L, H, W, group, r.cus)
        tag = f"{c.id} group {group} (G {G}, groups {cdiv(L, G)})"
        run = lambda src, op, ep, ab, ops: _complex(twice(r, f"{tag} op {op} epilogue {ep}", hw2, nbytes // 4,
                                                          call(src, op, ep, group, ab, nbytes), ops, reduced=nbytes > 0), (B, H, W))
        got = run(yb, ADJOINT, NONE, None, [(yb, ybits), (pb, pbits)])
        yd = yadj.to(C128)
        ref = (P.conj().unsqueeze(0) * torch.fft.ifft2(yd, norm="ortho")).sum(1)
        worst["adjoint"] = max(worst["adjoint"], _ratio(f"{tag} adjoint", (got.to(C128) - ref).abs(),
                                                        _adjoint_bound(P, per, yd, torch.zeros(B, L, dtype=torch.float64))))
        for ep, (aux, t, dt) in stages.items():
            ab, abits = _guarded(r, aux)
            got = run(xb, NORMAL, ep, ab, [(xb, xbits), (pb, pbits), (ab, abits)])
            assert bool(torch.isfinite(torch.view_as_real(got)).all()), f"{tag} normal epilogue {ep}: not finite"
            sb, sbits = stored[ep]
            composed = run(sb, ADJOINT, NONE, None, [(sb, sbits), (pb, pbits)])
            assert torch.equal(torch.view_as_real(got).view(torch.int32), torch.view_as_real(composed).view(torch.int32)), \
                f"{tag} normal epilogue {ep}: not the bits of the adjoint operation on the stored forward result"
            ref = (P.conj().unsqueeze(0) * torch.fft.ifft2(t, norm="ortho")).sum(1)
            bound = _adjoint_bound(P, per, t, torch.linalg.vector_norm(dt, dim=(2, 3)))
            worst["normal"] = max(worst["normal"], _ratio(f"{tag} normal epilogue {ep}", (got.to(C128) - ref).abs(), bound))
    return worst


def run_workspace_scan(r):
    planes = sorted({(c.H, c.W) for c in PTYCHO})
    seen = set()
    for H, W in planes:
        for L in (1, 2, 5, 9):
            for batch in (1, 3, 5, 7, 20, 40, 300, 600):
                for group in (0, 1, 2, max(L - 1, 1), L, L + 3):
                    for op in (FORWARD, ADJOINT, NORMAL):
                        want = ptycho_workspace_bytes(batch, L, H, W, op, group, r.cus)
                        assert r.ptycho_workspace_bytes(batch, L, H, W, op, group) == want, (batch, L, H, W, op, group, r.cus)
                    seen.add(ptycho_group(batch, L, H, W, 0, r.cus))
    assert len(seen) > 2 and r.ptycho_workspace_bytes(0, 5, 16, 16, ADJOINT, 0) == 0


def run_ptycho_rejections(r):
    """calls dinv_ptycho_apply must refuse: a non-zero status, the reason in dinv_last_error, no launch and no write"""
    B, L, H, W = 2, 5, 8, 12
    need = ptycho_workspace_bytes(B, L, H, W, ADJOINT, 2, r.cus)
    assert need == B * 3 * H * W * 8
    x, probe, aux = Guarded(2 * B * L * H * W, r.device), Guarded(2 * L * H * W, r.device), Guarded(B * L * H * W, r.device)
    for b in (x, probe, aux):
        b.t.zero_()
    out, ws = Guarded(2 * B * L * H * W, r.device), Guarded(need // 4, r.device)
    X, P, A, O, WS = (b.t.data_ptr() for b in (x, probe, aux, out, ws))
    too_big = SQUARE + 1
    #        x  out aux H  W  op       epilogue   group ws bytes    plans         reason
    bad = [(X, O, A, H, W, ADJOINT, WEIGHT, 0, WS, need, (None, None), "adjoint has no epilogue"),
           (X, O, 0, H, W, ADJOINT, ABS2, 0, WS, need, (None, None), "adjoint has no epilogue"),
           (X, O, 0, H, W, NORMAL, NONE, 0, WS, need, (None, None), "normal operation"),
           (X, O, 0, H, W, NORMAL, ABS2, 0, WS, need, (None, None), "normal operation"),
           (X, O, 0, H, W, ADJOINT, NONE, -1, WS, need, (None, None), "group"),
           (X, O, A, H, W, NORMAL, WEIGHT, -2, WS, need, (None, None), "group"),
           (X, O, 0, H, W, ADJOINT, NONE, 2, WS, need - 1, (None, None), "workspace"),
           (X, O, 0, H, W, ADJOINT, NONE, 2, 0, need, (None, None), "workspace"),
           (X, O, 0, H, W, ADJOINT, NONE, 2, 0, 0, (None, None), "workspace"),
           (X, O, 0, H, W, ADJOINT, NONE, 2, X, need, (None, None), "workspace"),
           (X, O, A, H, W, NORMAL, AMPLITUDE, 2, O, need, (None, None), "workspace"),
           (X, O, 0, H, W, FORWARD, NONE, 0, WS, need, (16, None), "plans are for lengths"),
           (X, O, 0, H, W, ADJOINT, NONE, 0, WS, need, (None, 12), "plans are for lengths"),
           (X, O, 0, too_big, too_big, FORWARD, NONE, 0, WS, need, (None, None), "LDS"),
           (X, O, 0, too_big, too_big, ADJOINT, NONE, 0, WS, need, (None, None), "LDS"),
           (O, O, 0, H, W, FORWARD, NONE, 0, WS, need, (None, None), "distinct"),
           (X, O, 0, H, W, FORWARD, WEIGHT, 0, WS, need, (None, None), "needs a real array"),
           (X, O, O, H, W, FORWARD, AMPLITUDE, 0, WS, need, (None, None), "needs a real array"),
           (X, O, 0, H, W, 3, NONE, 0, WS, need, (None, None), "unknown operation"),
           (X, O, A, H, W, FORWARD, 4, 0, WS, need, (None, None), "unknown epilogue")]
    for xp, op_, ap, h, w, op, ep, group, wp, wbytes, (pw, ph), why in bad:
        rc = r.ptycho_raw(xp, op_, P, 1, ap, B, L, h, w, op, ep, group, wp, wbytes, pw, ph)
        assert rc != 0 and why in r.err(), f"ptycho ({why}, op {op}, epilogue {ep}): status {rc}, message {r.err()!r}"
    r.sync()
    assert out.untouched() and ws.untouched(), "a refused ptycho call wrote to its output or workspace"
    # no images: nothing to do, whatever the pointers
    assert r.ptycho_raw(0, 0, 0, 1, 0, 0, L, H, W, ADJOINT, NONE, 0, 0, 0) == 0, r.err()
    assert r.ptycho_raw(0, 0, 0, 0, 0, 0, L, H, W, FORWARD, ABS2, 0, 0, 0) == 0, r.err()
