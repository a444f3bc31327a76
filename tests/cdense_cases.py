"""Shared by tests/test_complex_operator_kernels_gpu.py (the gfx950 library) and tests/test_emu_complex_operator_cases.py (the
same kernel sources on the host emulation): one table of cases for the complex64 MFMA product of csrc/cdense.hip, each meant to
reach one dispatch path of dinv_cdense_apply at one of its edges, the Python restatement of the launcher's rules (NI, the row
chunks, the K split with its min_k = 2 I rule, the 16-byte load flags), the runner that calls the C entry points on guarded
buffers (tests/fft_cases.py Guarded) and the checks of every case.

Layout, exact.  Gaussian-integer operands with parts in [-4, 4]: a part of an output is a sum of 2 K products below 2^4, so
every partial sum is below 2^15 at K = 1024 and fp32 accumulates it without rounding in any order: the result must equal the
int64 complex product bit for bit.  The operands are drawn at random, so every row, column and k differs from every other and
the real parts differ from the imaginary ones: rows, columns or k's that the kernel swaps, drops or counts twice, a lost
conjugate and a wrong sign among the four v_mfma_f32_32x32x2_f32 of a complex multiply-accumulate all change the answer.  On
hardware this is the test of the accumulator-to-row map - the emulation holds the kernel's own formula.  |z|^2 (ABS2) is then
an integer evaluated in double and rounded once: the correctly rounded value, exact below 2^24.  Integer weights (WEIGHT) are
exact.

Rounding, elementwise.  randn operands.  Each part of an output is a sum of 2 K products accumulated by fused multiply-adds in
S slices and S - 1 additions, |xr||mr| + |xi||mi| <= |x||m|, so |got - exact| <= d = sqrt(2) gamma_{2K+S} sum_k |x_k||m_k| with
gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; the bound of
tests/test_emu_phase_retrieval.py within_gamma).  The epilogues are evaluated in double from the unrounded sum z' = Z + dz,
|dz| <= d, and rounded once, so with Z exact:
  ABS2       | |z'|^2 - |Z|^2 | <= 2 |Z| d + d^2, and the rounding u |Z|^2 (to first order)
  WEIGHT     (d + u |Z|) |w|
  AMPLITUDE  with s = sqrt(y / (|Z|^2 + eps)):  z'(1 - s') - Z (1 - s) = dz (1 - s) - z' (s' - s) and |s' - s| <= s d / (|Z| - d)
             (s is y^1/2 / |z| up to eps), |z'| <= |Z| + d: within d |1 - s| + s d |Z| / (|Z| - d) + 2 u |Z (1 - s)| where
             |Z| >= 8 d.  The other elements are excluded; they may be at most 1 % of a case, a condition on the fp64 data alone.
A fifth of y is zero: there the factor is exactly 1 and the AMPLITUDE output has the bits of the NONE output.

Every buffer is guarded: the input, the matrix, the real array of the epilogue, the output and the workspace.  The matrix is
allocated to the last element the contract lets the kernel read, (rows - 1) ldm + row length, and the columns between two rows
of a strided matrix keep the guard pattern, which is a NaN: a read outside the operands shows in the result."""
import ctypes
from dataclasses import dataclass

import torch

from fft_cases import POISON, Guarded

U = 2.0 ** -24
TILE, BLOCK_K, HALF_K, MAX_NI, TARGET_WAVES, MIN_SLICE_K = 32, 16, 8, 4, 1024, 64
NONE, ABS2, WEIGHT, AMPLITUDE = 0, 1, 2, 3
EPS = 1e-12
C128 = torch.complex128


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the launcher's rules, restated
def split_k(I, K, R):
    """(S, kchunk) of csrc/cdense.hip split_k: no slice shorter than 2 I k's (at most 64, at least one block of 16)"""
    tiles = cdiv(R, TILE) * cdiv(I, TILE * MAX_NI)
    min_k = min(MIN_SLICE_K, cdiv(2 * I, BLOCK_K) * BLOCK_K)
    s = max(1, min(TARGET_WAVES // tiles, cdiv(K, min_k)))
    c = cdiv(cdiv(K, s), BLOCK_K) * BLOCK_K
    return cdiv(K, c), c


def accumulators(I):
    """NI of cdense_partial_kernel<NI>"""
    return 4 if I > 2 * TILE else (2 if I > TILE else 1)


def row_chunks(I):
    return cdiv(I, TILE * MAX_NI) if accumulators(I) == 4 else 1


def workspace_bytes(I, K, R):
    S, _ = split_k(I, K, R)
    return S * I * R * 8 if S > 1 else 0


def expected_launches(I, K, R):
    S, _ = split_k(I, K, R)
    return [f"cdense_partial_kernel<{accumulators(I)}>"] + (["cdense_reduce_kernel"] if S > 1 else [])


def ldm_of(c):
    return (c.R if c.transposed else c.K) + c.pad


def vector_loads(c):
    """(vec_in, vec_m) of the launcher for case c on Guarded buffers (16-byte aligned before the `off` complex elements)"""
    return c.off % 2 == 0 and c.K % 2 == 0, not c.transposed and ldm_of(c) % 2 == 0


# ------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    I: int
    K: int
    R: int
    transposed: int = 0
    conj: int = 0
    pad: int = 0                # ldm = row length + pad
    off: int = 0                # complex elements (8 bytes each) by which `in` is off 16-byte alignment
    emu: bool = True

    @property
    def id(self):
        S, c = split_k(self.I, self.K, self.R)
        return (f"ni{accumulators(self.I)}-chunks{row_chunks(self.I)}-s{S}-kc{c}-i{self.I}-k{self.K}-r{self.R}"
                + ("-transposed" if self.transposed else "-rows") + ("-conj" if self.conj else "")
                + (f"-ldm+{self.pad}" if self.pad else "") + ("-in+8B" if self.off else ""))


_T = [
    # NI = 1: I <= 32.  K walks the edges of the 16-k block with 8 per half wave: the upper half idle (1, 7, 8), a partial 8
    # (7, 9, 15, 17, 31, 33, 63, 65, 97), one slice against several.  min_k = 16 up to I = 8 and 32 from I = 9, so K = 17
    # and 31 are two slices at I <= 8 and one at I = 9; K = 33 two at I = 9; 1000 ends its last slice short, 1024 full
    (1, 1, 1, 0, 0, 0, 0), (4, 7, 31, 1, 1, 0, 0), (5, 8, 32, 0, 1, 4, 0), (8, 9, 33, 1, 0, 3, 0), (9, 15, 70, 0, 0, 0, 1),
    (31, 16, 32, 1, 1, 4, 0), (32, 17, 33, 0, 1, 3, 1), (8, 17, 70, 0, 0, 0, 0), (9, 17, 31, 1, 0, 0, 0), (8, 31, 33, 1, 1, 0, 1),
    (9, 31, 1, 0, 1, 4, 0), (9, 33, 32, 0, 0, 0, 0), (5, 63, 31, 1, 0, 3, 0), (4, 64, 33, 0, 1, 0, 0), (31, 65, 1, 1, 1, 3, 0),
    (32, 97, 70, 0, 0, 4, 1), (5, 1000, 33, 0, 1, 0, 0, False), (4, 1024, 70, 1, 0, 0, 0, False),
    (1, 1000, 31, 1, 1, 4, 0), (32, 64, 70, 0, 0, 0, 0),
    # NI = 2: 33 <= I <= 64
    (33, 1, 33, 0, 1, 0, 0), (33, 16, 70, 1, 0, 0, 0), (64, 17, 32, 0, 0, 3, 0), (64, 65, 31, 1, 1, 4, 1),
    (33, 1000, 70, 0, 0, 0, 1, False), (64, 1024, 33, 1, 0, 3, 0, False), (33, 63, 1, 0, 1, 4, 0), (64, 8, 70, 0, 0, 0, 0), (33, 9, 31, 1, 1, 0, 0), (64, 64, 32, 0, 1, 0, 0),
    # NI = 4, one chunk of rows: 65 <= I <= 128
    (65, 1, 32, 1, 0, 0, 0), (65, 33, 70, 0, 1, 0, 0), (128, 15, 33, 1, 1, 3, 0), (128, 64, 31, 0, 0, 4, 1),
    (65, 1000, 70, 1, 0, 0, 0, False), (128, 1024, 1, 0, 1, 0, 0, False), (128, 97, 70, 0, 0, 3, 1), (65, 7, 31, 0, 0, 0, 0),
    # NI = 4, two chunks with one row in the second
    (129, 31, 33, 0, 1, 0, 0), (129, 65, 70, 1, 1, 4, 0, False), (129, 1000, 32, 0, 0, 0, 1, False), (129, 16, 31, 1, 0, 3, 0),
    # NI = 4, three chunks with one row in the third (the largest take the emulation more than a few seconds)
    (257, 17, 70, 0, 0, 0, 0), (257, 64, 33, 1, 1, 0, 1), (257, 1024, 70, 0, 1, 4, 0, False), (257, 97, 31, 1, 0, 3, 0),
    (257, 1000, 1, 0, 0, 3, 1, False), (257, 8, 32, 0, 1, 0, 0),
    # rows of an odd K inside a matrix of 16-byte aligned rows (ldm = K + 1): the 16-byte loads stay on and the last 8 of a row is
    # one element short, so a load that took it as whole would read the poisoned column after the row
    (5, 7, 33, 0, 0, 1, 0), (9, 15, 32, 0, 1, 1, 0), (33, 31, 32, 0, 0, 1, 0), (65, 63, 70, 0, 1, 1, 0), (8, 97, 31, 0, 0, 1, 0),
    # an even K that is no multiple of 8 (beside the K's of the real table): the 16-byte loads of `in` stay on and its last 8 is
    # short; with an even ldm the same holds for M
    (5, 10, 33, 0, 0, 0, 0), (33, 70, 31, 0, 1, 2, 0), (65, 22, 32, 0, 0, 0, 0), (129, 1022, 33, 0, 1, 0, 0, False),
]
CASES = [Case(*t) for t in _T]
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"


# ------------------------------------------------------------------ the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.cdense), `device` of its
    buffers, `stream()` -> the stream argument and - on the emulation - `reset()` / `launches()`, the kernels launched since the
    last reset as the launcher spells them"""

    def __init__(self, lib, device, stream, reset=None, launches=None):
        self.lib, self.device, self._stream = lib, torch.device(device), stream
        self.reset, self.launches = reset, launches

    def err(self):
        return self.lib.dinv_last_error().decode()

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def workspace_bytes(self, I, K, R):
        return int(self.lib.dinv_cdense_workspace_bytes(I, K, R))

    def raw(self, x, m, out, aux, I, K, R, ldm, transposed, conj, epilogue, ws, ws_bytes):
        """the entry point on raw addresses; returns its status"""
        if self.reset:
            self.reset()
        vp = ctypes.c_void_p
        return self.lib.dinv_cdense_apply(vp(x), vp(m), vp(out), vp(aux), I, K, R, ldm, transposed, conj, epilogue, EPS, vp(ws),
                                          ws_bytes, self._stream())

    def apply(self, x_ptr, m_ptr, out_ptr, aux_ptr, c, epilogue, ws):
        rc = self.raw(x_ptr, m_ptr, out_ptr, aux_ptr, c.I, c.K, c.R, ldm_of(c), c.transposed, c.conj, epilogue,
                      ws.t.data_ptr() if ws.n else 0, ws.n * 4)
        assert rc == 0, f"{c.id}: error {rc}: {self.err()}"
        if self.launches is not None:
            got, want = self.launches(), expected_launches(c.I, c.K, c.R)
            assert got == want, f"{c.id}: launched {got}, the restated dispatch expects {want}"


def _pairs(z):
    """complex [*] -> fp32 words, interleaved"""
    return torch.view_as_real(z.to(torch.complex64).contiguous()).reshape(-1)


class Operands:
    """guarded device copies of x [I, K] and of op(M) = M [R, K] stored as the case says: transposed as [K, R], conjugated when
    the kernel is to conjugate it back"""

    def __init__(self, r, c, x, M):
        self.c = c
        self.xb = Guarded(2 * (c.I * c.K + c.off), r.device)
        self.xb.t[2 * c.off:].copy_(_pairs(x))
        self.xp = self.xb.t.data_ptr() + 8 * c.off
        store = M.conj() if c.conj else M
        store = (store.t() if c.transposed else store).resolve_conj()
        rows, length = store.shape
        ldm = length + c.pad
        assert ldm == ldm_of(c)
        self.mb = Guarded(2 * ((rows - 1) * ldm + length), r.device)
        self.mb.t.as_strided((rows, length, 2), (2 * ldm, 2, 1)).copy_(torch.view_as_real(store.to(torch.complex64)))
        self.xbits, self.mbits = self.xb.bits().clone(), self.mb.bits().clone()

    def intact(self):
        return (self.xb.guards_intact() and self.mb.guards_intact() and torch.equal(self.xb.bits(), self.xbits)
                and torch.equal(self.mb.bits(), self.mbits))


def product(r, c, ops, epilogue=NONE, aux=None):
    """two guarded calls that must agree; returns the result on the CPU: complex [I, R], or real for ABS2"""
    S, _ = split_k(c.I, c.K, c.R)
    nbytes = r.workspace_bytes(c.I, c.K, c.R)
    assert nbytes == workspace_bytes(c.I, c.K, c.R), f"{c.id}: workspace of {nbytes} bytes, the restated split has S = {S}"
    tag = f"{c.id} epilogue {epilogue}"
    words = c.I * c.R * (1 if epilogue == ABS2 else 2)
    ab = None
    if aux is not None:
        ab = Guarded(c.I * c.R, r.device)
        ab.t.copy_(aux.reshape(-1))
        abits = ab.bits().clone()
    results = []
    for _ in range(2):
        out, ws = Guarded(words, r.device), Guarded(nbytes // 4, r.device)
        r.apply(ops.xp, ops.mb.t.data_ptr(), out.t.data_ptr(), ab.t.data_ptr() if ab else 0, c, epilogue, ws)
        bits = out.bits()
        assert out.guards_intact(), f"{tag}: write outside the output"
        assert ws.guards_intact(), f"{tag}: write outside the workspace"
        assert not bool((bits == POISON).any()), (f"{tag}: {int((bits == POISON).sum())} output words hold the guard pattern: "
                                                  "never written, or computed from a read outside the operands")
        if S > 1:
            assert not bool((ws.bits() == POISON).any()), f"{tag}: a slice left part of its partial tile unwritten"
        results.append(bits.clone())
    assert torch.equal(results[0], results[1]), f"{tag}: two identical calls differ"
    assert ops.intact(), f"{tag}: the call modified an operand"
    assert ab is None or (ab.guards_intact() and torch.equal(ab.bits(), abits)), f"{tag}: the call modified the real array"
    got = results[0].view(torch.float32)
    return got.view(c.I, c.R) if epilogue == ABS2 else torch.view_as_complex(got.view(c.I, c.R, 2))


def _seed(c):
    return c.I * 1009 + c.K * 31 + c.R * 7 + c.transposed * 3 + c.conj * 5 + c.pad * 11 + c.off * 13


def rounding_data(c):
    """the randn operands of case c with everything the rounding checks derive from them in fp64: x, M, Z = x M^T, the
    elementwise bound d, the weights w, the measurements y (a fifth zero), s and the elements the AMPLITUDE bound covers"""
    gen = torch.Generator().manual_seed(_seed(c) + 1)
    S, _ = split_k(c.I, c.K, c.R)
    x = torch.complex(torch.randn(c.I, c.K, generator=gen), torch.randn(c.I, c.K, generator=gen))
    M = torch.complex(torch.randn(c.R, c.K, generator=gen), torch.randn(c.R, c.K, generator=gen))
    w = torch.randn(c.I, c.R, generator=gen)
    xd, Md = x.to(C128), M.to(C128)
    Z = xd @ Md.t()
    n = 2 * c.K + S
    d = 2.0 ** 0.5 * (n * U / (1 - n * U)) * (xd.abs() @ Md.abs().t())
    y = (Z.abs().square() * torch.rand(c.I, c.R, generator=gen).double() * 2).float()
    y.view(-1)[::5] = 0.0
    s = torch.sqrt(y.double() / (Z.abs().square() + EPS))
    covered = Z.abs() >= 8 * d
    return dict(x=x, M=M, w=w, y=y, Z=Z, d=d, s=s, covered=covered, n=n)


def excluded_fraction(c):
    return 1.0 - float(rounding_data(c)["covered"].double().mean())


def _worst(c, what, err, bound, mask=None):
    ratio = err / bound
    if mask is not None:
        ratio = torch.where(mask, ratio, torch.zeros_like(ratio))
    assert not bool(torch.isnan(ratio).any()), f"{c.id} {what}: NaN in the result"
    worst = float(ratio.max())
    at = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
    print(f"{c.id} {what}: worst element {at} error / bound {worst:.3g}")
    assert worst <= 1.0, f"{c.id} {what}: element {at} is {worst:.3g} times its bound"
    return worst


def run_case(r, c):
    """runs case c on runner r, asserts everything the module docstring lists and returns the worst |error| / bound of each
    rounding check"""
    gen = torch.Generator().manual_seed(_seed(c))
    # ---- layout, exact
    ri = lambda *shape: torch.randint(-4, 5, shape, generator=gen)
    xr, xi, mr, mi = ri(c.I, c.K), ri(c.I, c.K), ri(c.R, c.K), ri(c.R, c.K)
    wi = ri(c.I, c.R)
    wr_, wi_ = xr @ mr.t() - xi @ mi.t(), xr @ mi.t() + xi @ mr.t()        # int64
    assert int((xr.abs() @ mr.abs().t() + xi.abs() @ mi.abs().t()).max()) < 2 ** 24
    assert int((xr.abs() @ mi.abs().t() + xi.abs() @ mr.abs().t()).max()) < 2 ** 24
    ops = Operands(r, c, torch.complex(xr.float(), xi.float()), torch.complex(mr.float(), mi.float()))

    def exact(what, got, want):
        wrong = got.double() != want.double()
        assert not bool(wrong.any()), (f"{c.id} {what}: {int(wrong.sum())} of {wrong.numel()} integer outputs are wrong, the first "
                                       f"at (i, r) = {tuple(int(v) for v in wrong.nonzero()[0])}")

    got = product(r, c, ops)
    exact("real part", got.real, wr_)
    exact("imaginary part", got.imag, wi_)
    abs2 = wr_ * wr_ + wi_ * wi_
    assert bool((abs2 < 2 ** 24).any())
    exact("abs2", product(r, c, ops, ABS2), abs2.double().float())           # one rounding of the integer: exact below 2^24
    got = product(r, c, ops, WEIGHT, wi.float())
    exact("weighted real part", got.real, wr_ * wi)
    exact("weighted imaginary part", got.imag, wi_ * wi)
    # ---- rounding, elementwise
    D = rounding_data(c)
    Z, d, s, w, y = D["Z"], D["d"], D["s"], D["w"].double(), D["y"]
    ops = Operands(r, c, D["x"], D["M"])
    plain = product(r, c, ops)
    worst = {"sum": _worst(c, f"gamma_{D['n']}", (plain.to(C128) - Z).abs(), d)}
    za = Z.abs()
    got = product(r, c, ops, ABS2)
    worst["abs2"] = _worst(c, "abs2", (got.double() - za.square()).abs(), 2 * za * d + d * d + U * za.square())
    got = product(r, c, ops, WEIGHT, D["w"])
    worst["weight"] = _worst(c, "weight", (got.to(C128) - Z * w).abs(), (d + U * za) * w.abs())
    got = product(r, c, ops, AMPLITUDE, y)
    assert bool(torch.isfinite(torch.view_as_real(got)).all()), f"{c.id} amplitude: not finite"
    covered = D["covered"]
    excluded = 1.0 - float(covered.double().mean())
    assert excluded <= 0.01, f"{c.id}: {excluded:.2%} of the elements have |Z| < 8 d: another seed, not another cap"
    bound = d * (1 - s).abs() + s * d * za / (za - d).clamp_min(1e-300) + 2 * U * (Z * (1 - s)).abs()
    worst["amplitude"] = _worst(c, "amplitude", (got.to(C128) - Z * (1 - s)).abs(), bound, covered)
    zero = y == 0
    assert bool(zero.any()) and torch.equal(torch.view_as_real(got)[zero].view(torch.int32),
                                            torch.view_as_real(plain)[zero].view(torch.int32)), \
        f"{c.id} amplitude: where y = 0 the factor is exactly 1"
    return worst


# ------------------------------------------------------------------ refusals
def run_rejections(r):
    """calls dinv_cdense_apply must refuse: a non-zero status, the reason in dinv_last_error, no launch and no write"""
    I, K, R = 4, 40, 33
    S, _ = split_k(I, K, R)
    assert S > 1
    need = workspace_bytes(I, K, R)
    x, M, aux = Guarded(2 * I * K, r.device), Guarded(2 * R * K, r.device), Guarded(I * R, r.device)
    for b in (x, M, aux):
        b.t.zero_()
    out, ws = Guarded(2 * I * R, r.device), Guarded(need // 4, r.device)
    X, MM, O, A, WS = (b.t.data_ptr() for b in (x, M, out, aux, ws))
    #        x  m   out aux K  ldm    transposed epilogue ws  bytes      reason
    bad = [(X, MM, O, 0, K, K - 1, 0, NONE, WS, need, "row stride"),
           (X, MM, O, 0, K, R - 1, 1, NONE, WS, need, "row stride"),
           (X, MM, O, 0, K, K, 0, NONE, 0, 0, "workspace"),
           (X, MM, O, 0, K, K, 0, NONE, 0, need, "workspace"),
           (X, MM, O, 0, K, K, 0, NONE, WS, need - 1, "workspace"),
           (O, MM, O, 0, K, K, 0, NONE, WS, need, "alias"),
           (X, MM, O, 0, K, K, 0, WEIGHT, WS, need, "needs a real array"),
           (X, MM, O, 0, K, K, 0, AMPLITUDE, WS, need, "needs a real array"),
           (X, MM, O, O, K, K, 0, WEIGHT, WS, need, "needs a real array"),
           (X, MM, O, A, K, K, 0, 4, WS, need, "unknown epilogue"),
           (X, MM, O, A, K, K, 0, -1, WS, need, "unknown epilogue"),
           (X, MM, O, 0, 0, K, 0, NONE, WS, need, "bad shape")]
    for xp, mp, op, ap, k, ldm, tr, ep, wp, wbytes, why in bad:
        rc = r.raw(xp, mp, op, ap, I, k, R, ldm, tr, 0, ep, wp, wbytes)
        assert rc != 0 and why in r.err(), f"cdense ({why}): status {rc}, message {r.err()!r}"
        if r.launches is not None:
            assert r.launches() == [], f"cdense ({why}): a refused call launched {r.launches()}"
    r.sync()
    assert out.untouched() and ws.untouched(), "a refused cdense call wrote to its output or workspace"
    # no rows: nothing to do, whatever the pointers
    assert r.raw(0, 0, 0, 0, 0, K, R, K, 0, 0, NONE, 0, 0) == 0, r.err()
    assert r.launches is None or r.launches() == []
