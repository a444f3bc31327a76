"""Shared by tests/test_operator_kernels_gpu.py (the gfx950 library) and tests/test_emu_operator_cases.py (the same kernel
sources on the host emulation): one table of cases for the fp32 MFMA product of csrc/dense.hip, each meant to reach one dispatch
path of dinv_dense_apply at one of its edges, the Python restatement of the launcher's rules (NI, the K split), the runner that
calls the C entry points on guarded buffers (tests/fft_cases.py Guarded) and the two checks of every case.

Layout, exact.  Integer operands in [-8, 8]: every product is below 2^7 and every partial sum below 2^17 at K = 1024, so fp32
accumulates them without rounding in any order and the result must equal the int64 product bit for bit.  The operands are
drawn at random, so every row, column and k differs from every other: a pair of rows, columns or k's that the kernel swaps,
drops or counts twice changes the answer.  On hardware this is the test of the accumulator-to-row map of
v_mfma_f32_32x32x2_f32 - the emulation holds the same formula as the kernel and cannot tell a wrong map from a right one.

Rounding, elementwise.  randn operands.  An output is a sum of K products accumulated by fused multiply-adds in S slices and
S - 1 additions of the slices, so |got - exact| <= gamma_{K+S} sum_k |in[i, k]| |M[r, k]| with gamma_n = n u / (1 - n u),
u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  Derived, not measured.

Every buffer is guarded: the input, the matrix, the output and the workspace.  The matrix is allocated to the last element the
contract lets the kernel read, (rows - 1) ldm + row length, and the columns between two rows of a strided matrix keep the guard
pattern, which is a NaN: a read outside the operands shows in the result."""
import ctypes
from dataclasses import dataclass

import torch

from fft_cases import POISON, Guarded

U = 2.0 ** -24
TILE, BLOCK_K, MAX_NI, TARGET_WAVES, MIN_SLICE_K = 32, 32, 4, 1024, 64


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the launcher's rules, restated
def split_k(I, K, R):
    """(S, kchunk) of csrc/dense.hip split_k"""
    tiles = cdiv(R, TILE) * cdiv(I, TILE * MAX_NI)
    s = max(1, min(TARGET_WAVES // tiles, cdiv(K, MIN_SLICE_K)))
    c = cdiv(cdiv(K, s), BLOCK_K) * BLOCK_K
    return cdiv(K, c), c


def accumulators(I):
    """NI of dense_partial_kernel<NI>"""
    return 4 if I > 2 * TILE else (2 if I > TILE else 1)


def row_chunks(I):
    return cdiv(I, TILE * MAX_NI) if accumulators(I) == 4 else 1


def expected_launches(I, K, R):
    S, _ = split_k(I, K, R)
    return [f"dense_partial_kernel<{accumulators(I)}>"] + (["dense_reduce_kernel"] if S > 1 else [])


def vector_loads(c):
    """(vec_in, vec_m) of the launcher for case c on Guarded buffers (16-byte aligned before the `off` words)"""
    ldm = (c.R if c.transposed else c.K) + c.pad
    return c.off == 0 and c.K % 4 == 0, not c.transposed and ldm % 4 == 0


# ------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    I: int
    K: int
    R: int
    transposed: int = 0
    pad: int = 0                # ldm = row length + pad
    off: int = 0                # words by which `in` is off 16-byte alignment
    emu: bool = True

    @property
    def id(self):
        S, _ = split_k(self.I, self.K, self.R)
        return (f"ni{accumulators(self.I)}-chunks{row_chunks(self.I)}-s{S}-i{self.I}-k{self.K}-r{self.R}"
                + ("-transposed" if self.transposed else "-rows") + (f"-ldm+{self.pad}" if self.pad else "")
                + ("-in+4B" if self.off else ""))


_T = [
    # NI = 1: I <= 32.  K walks the edges of the 32-k block: the upper half wave idle (1, 15, 16, 33), a partial 16 (15, 17, 31,
    # 33, 63, 65, 97), one slice (K <= 64) against several with a short last one (1000) or a full one (1024)
    (1, 1, 1, 0, 0, 0), (4, 15, 31, 1, 0, 0), (5, 16, 32, 0, 4, 0), (31, 17, 33, 1, 3, 0), (32, 31, 70, 0, 0, 1),
    (32, 32, 32, 1, 4, 0), (1, 33, 70, 0, 3, 1), (5, 63, 31, 1, 0, 0), (4, 64, 33, 0, 0, 0), (31, 65, 1, 1, 3, 0),
    (32, 97, 70, 0, 4, 1), (5, 1000, 33, 0, 0, 0), (4, 1024, 70, 1, 0, 1), (1, 1000, 31, 1, 4, 0),
    # NI = 2: 33 <= I <= 64
    (33, 1, 33, 0, 0, 0), (33, 32, 70, 1, 0, 0), (64, 17, 32, 0, 3, 0), (64, 65, 31, 1, 4, 1), (33, 1000, 70, 0, 0, 1),
    (64, 1024, 33, 1, 3, 0), (33, 63, 1, 0, 4, 0), (64, 16, 70, 0, 0, 0),
    # NI = 4, one chunk of rows: 65 <= I <= 128
    (65, 1, 32, 1, 0, 0), (65, 33, 70, 0, 0, 0), (128, 15, 33, 1, 3, 0), (128, 64, 31, 0, 4, 1), (65, 1000, 70, 1, 0, 0),
    (128, 1024, 1, 0, 0, 0), (128, 97, 70, 0, 3, 1),
    # NI = 4, two chunks with one row in the second
    (129, 31, 33, 0, 0, 0), (129, 65, 70, 1, 4, 0), (129, 1000, 32, 0, 0, 1), (129, 16, 31, 1, 3, 0),
    # NI = 4, three chunks with one row in the third (the largest takes the emulation more than a few seconds)
    (257, 17, 70, 0, 0, 0), (257, 64, 33, 1, 0, 1), (257, 1024, 70, 0, 4, 0, False), (257, 97, 31, 1, 3, 0), (257, 1000, 1, 0, 3, 1),
    (257, 32, 32, 0, 0, 0),
    # rows of K = 15 mod 16 floats inside a matrix of 16-byte aligned rows (ldm = K + 1): the 16-byte loads stay on and the last
    # 16 of a row is one float short, so a load that took it as whole would read the poisoned column after the row
    (5, 15, 33, 0, 1, 0), (33, 31, 32, 0, 1, 0), (65, 63, 70, 0, 1, 0),
]
CASES = [Case(*t) for t in _T]
assert len({c.id for c in CASES}) == len(CASES), "duplicate case ids"


# ------------------------------------------------------------------ the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.dense), `device` of its
    buffers, `stream()` -> the stream argument and - on the emulation - `reset()` / `launches()`, the kernels launched since the
    last reset as the launcher spells them"""

    def __init__(self, lib, device, stream, reset=None, launches=None):
        self.lib, self.device, self._stream = lib, torch.device(device), stream
        self.reset, self.launches = reset, launches

    def err(self):
        return self.lib.dinv_last_error().decode()

    def workspace_bytes(self, I, K, R):
        return int(self.lib.dinv_dense_workspace_bytes(I, K, R))

    def apply(self, x_ptr, m_ptr, out_ptr, c, ws):
        if self.reset:
            self.reset()
        ldm = (c.R if c.transposed else c.K) + c.pad
        rc = self.lib.dinv_dense_apply(ctypes.c_void_p(x_ptr), ctypes.c_void_p(m_ptr), ctypes.c_void_p(out_ptr), c.I, c.K, c.R,
                                       ldm, c.transposed, ctypes.c_void_p(ws.t.data_ptr() if ws.n else 0), ws.n * 4,
                                       self._stream())
        assert rc == 0, f"{c.id}: error {rc}: {self.err()}"
        if self.launches is not None:
            got, want = self.launches(), expected_launches(c.I, c.K, c.R)
            assert got == want, f"{c.id}: launched {got}, the restated dispatch expects {want}"


def _operands(r, c, x, M):
    """guarded device copies of x [I, K] and of M [R, K] stored as the case says; returns (x buffer, x pointer, M buffer)"""
    xb = Guarded(c.I * c.K + c.off, r.device)
    xb.t[c.off:].copy_(x.reshape(-1))
    store = M.t() if c.transposed else M
    rows, length = store.shape
    ldm = length + c.pad
    mb = Guarded((rows - 1) * ldm + length, r.device)
    mb.t.as_strided((rows, length), (ldm, 1)).copy_(store)
    return xb, xb.t.data_ptr() + 4 * c.off, mb


def _product(r, c, x, M):
    """one guarded call and a second one; returns the result on the CPU"""
    S, _ = split_k(c.I, c.K, c.R)
    nbytes = r.workspace_bytes(c.I, c.K, c.R)
    assert nbytes == (S * c.I * c.R * 4 if S > 1 else 0), f"{c.id}: workspace of {nbytes} bytes, the restated split has S = {S}"
    xb, xp, mb = _operands(r, c, x, M)
    xbits, mbits = xb.bits().clone(), mb.bits().clone()
    results = []
    for _ in range(2):
        out, ws = Guarded(c.I * c.R, r.device), Guarded(nbytes // 4, r.device)
        r.apply(xp, mb.t.data_ptr(), out.t.data_ptr(), c, ws)
        bits = out.bits()
        assert out.guards_intact(), f"{c.id}: write outside the output"
        assert ws.guards_intact(), f"{c.id}: write outside the workspace"
        assert not bool((bits == POISON).any()), (f"{c.id}: {int((bits == POISON).sum())} outputs hold the guard pattern: "
                                                  "never written, or computed from a read outside the operands")
        if S > 1:
            assert not bool((ws.bits() == POISON).any()), f"{c.id}: a slice left part of its partial tile unwritten"
        results.append(bits.clone())
    assert torch.equal(results[0], results[1]), f"{c.id}: two identical calls differ"
    assert xb.guards_intact() and mb.guards_intact() and torch.equal(xb.bits(), xbits) and torch.equal(mb.bits(), mbits), \
        f"{c.id}: the call modified an operand"
    return results[0].view(torch.float32).view(c.I, c.R)


def run_case(r, c):
    """runs case c on runner r, asserts everything the module docstring lists and returns the worst |error| / bound"""
    gen = torch.Generator().manual_seed(c.I * 1009 + c.K * 31 + c.R * 7 + c.transposed * 3 + c.pad + c.off)
    S, _ = split_k(c.I, c.K, c.R)
    # layout, exact
    xi = torch.randint(-8, 9, (c.I, c.K), generator=gen)
    Mi = torch.randint(-8, 9, (c.R, c.K), generator=gen)
    want = xi @ Mi.t()
    assert int((xi.abs() @ Mi.abs().t()).max()) < 2 ** 24
    got = _product(r, c, xi.float(), Mi.float())
    wrong = got.double() != want.double()
    assert not bool(wrong.any()), (f"{c.id}: {int(wrong.sum())} of {wrong.numel()} integer outputs are wrong, the first at (i, r) = "
                                   f"{tuple(int(v) for v in wrong.nonzero()[0])}")
    # rounding, elementwise
    x, M = torch.randn(c.I, c.K, generator=gen), torch.randn(c.R, c.K, generator=gen)
    got = _product(r, c, x, M)
    n = c.K + S
    gamma = n * U / (1 - n * U)
    xd, Md = x.double(), M.double()
    ratio = (got.double() - xd @ Md.t()).abs() / (gamma * (xd.abs() @ Md.abs().t()))
    assert not bool(torch.isnan(ratio).any()), f"{c.id}: NaN in the result"
    worst = float(ratio.max())
    at = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
    print(f"{c.id}: worst element {at} error / bound {worst:.3g} (gamma_{n} = {gamma:.3g})")
    assert worst <= 1.0, f"{c.id}: element {at} is {worst:.3g} times its bound gamma_{n} |x| |M|^T"
    return worst
