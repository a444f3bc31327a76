"""Shared by tests/test_fft_gpu.py (the gfx950 library) and tests/test_emu_fft.py (the same kernel sources on the host emulation):
one table of FFT-engine cases, each meant to reach one dispatch path of csrc/fft_launch.hpp at one of its edges, the runner that
calls the C entry points (dinv_fft_c2c_axis, dinv_rfft2, dinv_irfft2, dinv_blurfft_apply) on guarded buffers, and the complex128
references.

Every output lives inside a larger allocation, at a 16-byte-aligned offset, with a 4 KiB guard band on each side filled with a
fixed NaN bit pattern (the output itself starts as the same pattern, so a bin the kernel never writes is NaN).  After the call
the guard bands must be bit-identical: a write outside the tensor lands in owned memory and is reported, not a fault."""
import ctypes
import math
from dataclasses import dataclass, field

import torch

GUARD = 1024                      # fp32 words per guard band (4 KiB)
POISON = 0x7FC5A5A5               # a quiet-NaN bit pattern no kernel produces


# ------------------------------------------------------------------ the fp64 restatement of the BlurFFT symbol
def _symbol_ref(X, m, a, flags, add):
    """SYMBOL of include/deepinv_amd.h (dinv_blurfft_apply) in fp64 with the reference's expressions (blur.py:639-657,
    forward.py:1080-1117, 1212-1252): X complex [P,H,Wh], m real pairs [Ps,H,Wh,2], a complex [Ps,H,Wh]"""
    P, Ps = X.shape[0], m.shape[0]
    m = m.double().repeat(P // Ps, 1, 1, 1)
    a = a.to(torch.complex128).repeat(P // Ps, 1, 1)
    v = X.to(torch.complex128)
    if flags & 1:
        v = v * torch.conj(a)
    v = torch.view_as_real(v)
    mode = (flags >> 4) & 7
    if mode == 1:
        v = m * v
    elif mode == 2:
        v = m * m * v
    elif mode == 3:
        v = v / (m * m + add)
    elif mode == 4:
        v = v * torch.where(m > 1e-5, 1 / m, torch.zeros_like(m))
    v = torch.view_as_complex(v.contiguous())
    if flags & 2:
        v = v * a
    return v


BLURFFT_FLAGS = [0x10 | 2, 1 | 0x10, 0x20, 1 | 0x20 | 2, 0x30, 1 | 0x40, 0]

# ------------------------------------------------------------------ error bounds (max over transforms of ||out - ref|| / ||ref||)
# Measured on the host emulation of the kernel sources (fp32 kernel arithmetic; `python -m pytest tests/test_emu_fft.py -s` prints
# every case's worst line): the worst per-line error of each path family over its emulated cases, and the bound at about 4x that.
BOUNDS = {
    "rows-v4": 7e-7,              # worst 1.65e-7 (rows-v4-64-n31-inv)
    "rows-wave": 5e-7,            # worst 1.2e-7 (rows-wave-512-n5-fwd)
    "rows-generic": 2.4e-6,       # worst 5.8e-7 (rows-generic-1021-n3-inv-centred)
    "rows-generic-lds": 6e-6,     # worst 1.4e-6 (N = 5851: one radix-5851 generic stage, 5851-term fp32 sums)
    "cols-static": 9e-7,          # worst 2.1e-7 (cols-static-512-p3-q257-fwd-centred)
    "cols-generic": 2.5e-6,       # worst 6.3e-7 (cols-generic-1021-p3-q100-inv-centred)
    "rfft2": 2e-6,                # worst 4.7e-7 (rfft2-h320-w17-p3)
    "irfft2": 1.6e-6,             # worst 4.0e-7 (irfft2-h320-w17-p3)
    "rfft2-narrow": 8e-6,         # worst 2.1e-6 (irfft2-h512-w2-p3): W <= 3, rows of 1 or 2 bins
    "blurfft": 2.2e-6,            # worst 5.5e-7 (blurfft-fused-h512-w64-p3-ps3)
}


# ------------------------------------------------------------------ static dispatch facts of csrc/fft_launch.hpp (restated)
STATIC_ROWS = (64, 128, 256, 320, 512)                  # DINV_STATIC_SIZES
WAVE_ROWS = (256, 320, 512)                             # C2CIo has Raw4 and N >= 256
STATIC_COLS = (16, 32, 64, 128, 256, 320, 512)
FUSED_BLUR_H = (64, 128, 256, 320, 512)
KMAX_GRID = 256 * 8
KMAX_LDS = 160 * 1024


def rows_tile(n):           # RowsL<N>
    return 8 if n >= 512 else (16 if n >= 128 else 32)


def cols_tile(n):           # ColsL<N>
    return 256 if n == 16 else 16


def fft_lds_bytes(n, generic, lines):
    """fft_core.hpp fft_lds_bytes"""
    ls = n + 1 if n % 2 == 0 else n
    b = n * 8 + ((n * 4 + 15) // 16) * 16
    b = ((b + 15) // 16) * 16
    return b + lines * ls * 8 * (2 if generic else 1)


def rows_lines_per_block(n, generic):
    """fft_launch.hpp rows_lines_per_block"""
    ls = n + 1 if n % 2 == 0 else n
    return max(1, min(64, 24576 // (ls * 8 * (2 if generic else 1))))


def generic_rows_lds(n):
    """LDS bytes of the generic rows kernel for length n (the plan's `generic` flag: a prime factor above 5)"""
    m = n
    for p in (2, 3, 5):
        while m % p == 0:
            m //= p
    generic = m > 1 or n == 1
    return fft_lds_bytes(n, generic, rows_lines_per_block(n, generic)), generic


def lds_limit_lengths():
    """(largest admitted n without a prime factor above 5, largest admitted n with one, smallest rejected n above both)"""
    smooth = prime = None
    n = 1
    while True:
        lds, gen = generic_rows_lds(n)
        if lds <= KMAX_LDS and n not in STATIC_ROWS:
            if gen:
                prime = n
            else:
                smooth = n
        if lds > KMAX_LDS and not gen and smooth is not None and prime is not None:
            return smooth, prime, n
        n += 1


# ------------------------------------------------------------------ the case table
@dataclass
class Case:
    id: str
    kind: str                   # c2c | rfft2 | irfft2 | blurfft | lds_reject
    family: str                 # key of BOUNDS
    emu: bool                   # small enough for the host emulation
    n: int = 0                  # c2c: transform length
    outer: int = 1              # c2c: lines (rows) or outer count (columns); rfft2 / blurfft: planes P
    inner: int = 1              # c2c: 1 = rows pass, else Q
    inverse: int = 0
    centered: int = 0
    H: int = 0
    W: int = 0
    Ps: int = 1
    extra: dict = field(default_factory=dict)


def _c2c(cases, family, n, outer, inner, inverse=0, centered=0, emu=True, tag=""):
    path = "rows" if inner == 1 else "cols"
    cid = f"{family}-{n}-{'n' if inner == 1 else 'p'}{outer}" + (f"-q{inner}" if inner > 1 else "")
    cid += ("-inv" if inverse else "-fwd") + ("-centred" if centered else "") + tag
    assert cid.startswith(path)
    cases.append(Case(cid, "c2c", family, emu, n=n, outer=outer, inner=inner, inverse=inverse, centered=centered))


def build_cases():
    cases = []
    # rows, fft_rows_static_v4_kernel: one line, a tile minus / plus one line, and a tail past kMaxGrid tiles (grid-stride)
    for n in (64, 128):
        L = rows_tile(n)
        for i, nl in enumerate((1, L - 1, L + 1)):
            _c2c(cases, "rows-v4", n, nl, 1, inverse=i % 2, centered=(i + 1) % 2)
        big = 65536 + 37 if n == 64 else 32768 + 5
        assert big > KMAX_GRID * L
        _c2c(cases, "rows-v4", n, big, 1, centered=1, emu=False)
        _c2c(cases, "rows-v4", n, big, 1, inverse=1, emu=False)
    # rows, fft_rows_wave_kernel (LW = 4 rows per wave tile): partial tiles, one full resident grid, and 2 * 8192 + 3 rows where
    # the persistent loop runs a second round with the next tile's loads prefetched
    for n in WAVE_ROWS:
        for nl in (1, 3, 4, 5, 8191, 2 * 8192 + 3):
            for inverse in (0, 1):
                for centered in (0, 1):
                    _c2c(cases, "rows-wave", n, nl, 1, inverse, centered, emu=nl <= 5)
    # rows, generic engine (fft_rows_kernel, dynamic LDS)
    for n in (1, 2, 3, 7, 17, 100, 243, 1000, 1021, 2048, 4096):
        for nl in (1, 3):
            _c2c(cases, "rows-generic", n, nl, 1, inverse=nl == 3, centered=(n % 2 == 1 and nl == 3))
    lpb = rows_lines_per_block(100, False)
    _c2c(cases, "rows-generic", 100, 2 * lpb + 1, 1, centered=1)          # several blocks, a partial last one
    # the LDS limit of the generic rows path: the largest admitted length without / with a prime factor, and one above
    smooth, prime, rejected = lds_limit_lengths()
    _c2c(cases, "rows-generic-lds", smooth, 3, 1, centered=1, tag="-lds-limit")
    _c2c(cases, "rows-generic-lds", prime, 3, 1, inverse=1, tag="-lds-limit")
    cases.append(Case(f"rows-generic-{rejected}-lds-reject", "lds_reject", "rows-generic-lds", True, n=rejected, outer=2))
    # columns, fft_cols_static_kernel: Q around the 16-column strip (256 at N = 16), outer 1 and 3
    for n in STATIC_COLS:
        for i, q in enumerate((2, 15, 16, 17, 255, 257)):
            outer = 3 if i % 2 else 1
            _c2c(cases, "cols-static", n, outer, q, inverse=i % 3 == 1, centered=i % 3 == 2)
    qt = -(-33 // cols_tile(32))
    _c2c(cases, "cols-static", 32, 2 * KMAX_GRID // qt + 5, 33, centered=1, emu=False)       # > 2 x kMaxGrid column tiles
    # columns, generic engine
    for n in (5, 17, 100, 1021, 2048):
        for i, q in enumerate((2, 3, 33, 100)):
            _c2c(cases, "cols-generic", n, 3 if i % 2 else 1, q, inverse=i % 2, centered=i >= 2)
    # rfft2 / irfft2: every static W (scalar rows kernel, RealRowsLoadIo / HalfRowsStoreRealIo), every static H (columns)
    hw = [(1, 1), (1, 2), (16, 3), (17, 17), (32, 64), (64, 100), (128, 128), (256, 256), (320, 320), (512, 512), (17, 64),
          (100, 128), (16, 512), (320, 17), (512, 2), (3, 256), (128, 320), (64, 1)]
    for H, W in hw:
        P = 3 if H * W <= 128 * 128 else 1
        narrow = W <= 3
        cases.append(Case(f"rfft2-h{H}-w{W}-p{P}", "rfft2", "rfft2-narrow" if narrow else "rfft2", True, outer=P, H=H, W=W))
        cases.append(Case(f"irfft2-h{H}-w{W}-p{P}", "irfft2", "rfft2-narrow" if narrow else "irfft2", True, outer=P, H=H, W=W))
    big = (2 * KMAX_GRID * rows_tile(128)) // 32 + 3           # P x 32 rows of 128: > 2 x kMaxGrid tiles of the row pass
    cases.append(Case(f"rfft2-h32-w128-p{big}-grid", "rfft2", "rfft2", False, outer=big, H=32, W=128))
    cases.append(Case(f"irfft2-h32-w128-p{big}-grid", "irfft2", "irfft2", False, outer=big, H=32, W=128))
    # dinv_blurfft_apply: fused column pass (H static) and the three-pass form; every flag combination runs inside each case
    for H, W, P, Ps in ((64, 64, 6, 3), (64, 255, 4, 4), (128, 255, 6, 3), (128, 64, 2, 2), (256, 256, 4, 2), (320, 320, 2, 2),
                        (512, 256, 2, 1), (512, 64, 3, 3), (16, 64, 6, 6), (16, 320, 2, 1), (17, 255, 3, 3), (100, 256, 4, 2),
                        (100, 320, 2, 2)):
        cases.append(Case(f"blurfft-{'fused' if H in FUSED_BLUR_H else '3pass'}-h{H}-w{W}-p{P}-ps{Ps}", "blurfft", "blurfft", True,
                          outer=P, H=H, W=W, Ps=Ps))
    P = 1700                                        # 1700 planes x 5 strips of 16 columns: > 4 x kMaxGrid fused tiles (its grid)
    cases.append(Case(f"blurfft-fused-h64-w128-p{P}-ps4-grid", "blurfft", "blurfft", False, outer=P, H=64, W=128, Ps=4,
                      extra={"flags": [0x10 | 2, 1 | 0x30]}))
    ids = [c.id for c in cases]
    assert len(ids) == len(set(ids)), "duplicate case ids"
    return cases


CASES = build_cases()


# ------------------------------------------------------------------ references and the error measure
def c2c_ref(x, axis, inverse, centered, scale):
    """x complex128 (CPU); unnormalised transform along `axis` times `scale`, with ifftshift / fftshift around it when centred"""
    if centered:
        x = torch.fft.ifftshift(x, dim=axis)
    y = torch.fft.ifft(x, dim=axis, norm="forward") if inverse else torch.fft.fft(x, dim=axis, norm="backward")
    if centered:
        y = torch.fft.fftshift(y, dim=axis)
    return y * scale


def worst_line_error(out, ref):
    """max over lines (last dim) of ||out - ref|| / ||ref||, in fp64; NaN (an unwritten output) counts as infinite"""
    o = out.detach().cpu().to(torch.complex128 if out.is_complex() or ref.is_complex() else torch.float64)
    r = ref.detach().cpu().to(o.dtype)
    n = r.shape[-1]
    o, r = o.reshape(-1, n), r.reshape(-1, n)
    num = (o - r).abs().pow(2).sum(-1).sqrt()
    den = r.abs().pow(2).sum(-1).sqrt()
    # lines of a few points (W = 1, 2, 3) can be short by chance: measure those against a quarter of the RMS line norm instead,
    # which leaves a wrong line an O(1) error
    den = torch.maximum(den, 0.25 * den.pow(2).mean().sqrt())
    e = num / den
    if torch.isnan(e).any():
        return float("inf")
    return float(e.max())


# ------------------------------------------------------------------ the runner
class Guarded:
    """`n` fp32 words at a 16-byte-aligned offset inside an allocation with GUARD poisoned words on either side"""

    def __init__(self, n, device):
        self.n = int(n)
        self.full = torch.full((2 * GUARD + self.n,), POISON, dtype=torch.int32, device=device)
        self.t = self.full[GUARD:GUARD + self.n].view(torch.float32)
        assert self.t.data_ptr() % 16 == 0

    def guards_intact(self):
        f = self.full
        return bool((f[:GUARD] == POISON).all()) and bool((f[GUARD + self.n:] == POISON).all())

    def untouched(self):
        return bool((self.full == POISON).all())

    def bits(self):
        return self.t.view(torch.int32).cpu()


class Runner:
    """the C entry points over one library: `lib` (ctypes), `device` of its buffers, `plan(n)` -> (plan struct, table tensor),
    `stream()` -> the stream argument"""

    def __init__(self, lib, device, plan, stream):
        self.lib, self.device, self._plan, self._stream = lib, torch.device(device), plan, stream

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(f"error {rc}: {self.lib.dinv_last_error().decode()}")

    def guarded(self, n):
        return Guarded(n, self.device)

    def dev(self, t):
        return t.contiguous().to(self.device)

    # ---- one-axis C2C
    def c2c(self, buf_in, buf_out, outer, inner, n, inverse, centered, scale):
        plan, table = self._plan(n)
        return self.lib.dinv_fft_c2c_axis(ctypes.c_void_p(buf_in.data_ptr()), ctypes.c_void_p(buf_out.data_ptr()),
                                          ctypes.c_int64(outer), ctypes.c_int64(inner), ctypes.byref(plan),
                                          ctypes.c_void_p(table.data_ptr()), ctypes.c_int32(inverse), ctypes.c_int32(centered),
                                          ctypes.c_float(scale), self._stream())

    def rfft2(self, x, out, P, H, W, scale):
        ph, th = self._plan(H)
        pw, tw = self._plan(W)
        return self.lib.dinv_rfft2(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_int64(P),
                                   ctypes.byref(ph), ctypes.c_void_p(th.data_ptr()), ctypes.byref(pw),
                                   ctypes.c_void_p(tw.data_ptr()), ctypes.c_float(scale), self._stream())

    def irfft2(self, spec, out, ws, P, H, W, scale):
        ph, th = self._plan(H)
        pw, tw = self._plan(W)
        return self.lib.dinv_irfft2(ctypes.c_void_p(spec.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_int64(P),
                                    ctypes.byref(ph), ctypes.c_void_p(th.data_ptr()), ctypes.byref(pw),
                                    ctypes.c_void_p(tw.data_ptr()), ctypes.c_float(scale), ctypes.c_void_p(ws.data_ptr()),
                                    ctypes.c_size_t(ws.numel() * ws.element_size()), self._stream())

    def blurfft(self, x, out, ws, P, H, W, m, a, Ps, flags, add, scale):
        ph, th = self._plan(H)
        pw, tw = self._plan(W)
        return self.lib.dinv_blurfft_apply(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_int64(P),
                                           ctypes.byref(ph), ctypes.c_void_p(th.data_ptr()), ctypes.byref(pw),
                                           ctypes.c_void_p(tw.data_ptr()), ctypes.c_void_p(m.data_ptr()),
                                           ctypes.c_void_p(a.data_ptr()), ctypes.c_int64(Ps), ctypes.c_int32(flags),
                                           ctypes.c_float(add), ctypes.c_float(scale), ctypes.c_void_p(ws.data_ptr()),
                                           ctypes.c_size_t(ws.numel() * ws.element_size()), self._stream())


def _randc(shape, gen):
    return torch.complex(torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen))


def _seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id)) % (2 ** 31)


def run_case(r, case):
    """runs `case` on runner `r`, asserts everything it checks and returns the worst per-transform error"""
    gen = torch.Generator().manual_seed(_seed(case))
    bound = BOUNDS[case.family]
    if case.kind in ("c2c", "lds_reject"):
        return _run_c2c(r, case, gen, bound)
    if case.kind == "rfft2":
        return _run_rfft2(r, case, gen, bound)
    if case.kind == "irfft2":
        return _run_irfft2(r, case, gen, bound)
    return _run_blurfft(r, case, gen, bound)


def _run_c2c(r, case, gen, bound):
    n, outer, inner = case.n, case.outer, case.inner
    shape = (outer, n, inner)
    x = _randc(shape, gen).to(torch.complex64)
    xr = torch.view_as_real(x).reshape(-1)
    xd = r.dev(xr)
    words = xr.numel()
    scale = 1.0 / math.sqrt(n) if n % 3 else 1.0 / n
    if case.kind == "lds_reject":
        out = r.guarded(words)
        rc = r.c2c(xd, out.t, outer * inner, 1, n, 0, 0, scale)
        assert rc != 0, f"length {n} is above the LDS limit of the generic rows path but the call succeeded"
        assert "LDS" in r.lib.dinv_last_error().decode()
        if r.device.type == "cuda":
            torch.cuda.synchronize(r.device)
        assert out.untouched(), "a rejected call wrote to its output"
        return 0.0
    out = r.guarded(words)
    r.check(r.c2c(xd, out.t, outer, inner, n, case.inverse, case.centered, scale))
    res = torch.view_as_complex(out.t.view(*shape, 2).cpu())
    assert out.guards_intact(), "write outside the output tensor"
    assert torch.equal(xd.cpu(), xr), "out-of-place call modified its input"
    ref = c2c_ref(x.to(torch.complex128), 1, case.inverse, case.centered, scale)
    err = worst_line_error(res.transpose(1, 2), ref.transpose(1, 2))
    assert err < bound, f"{case.id}: worst per-transform error {err:.3g} >= {bound:.3g}"
    bits = out.bits().clone()
    del out, res                                     # at most two output-sized buffers on the device at a time
    # a second identical call: bit-identical
    again = r.guarded(words)
    r.check(r.c2c(xd, again.t, outer, inner, n, case.inverse, case.centered, scale))
    assert torch.equal(again.bits(), bits), "two identical calls differ"
    assert again.guards_intact()
    del again
    # in place (in == out): bit-identical to out-of-place
    inpl = r.guarded(words)
    inpl.t.copy_(xd)
    r.check(r.c2c(inpl.t, inpl.t, outer, inner, n, case.inverse, case.centered, scale))
    assert inpl.guards_intact(), "in-place call wrote outside the tensor"
    assert torch.equal(inpl.bits(), bits), "in-place result differs from out-of-place"
    return err


def _run_rfft2(r, case, gen, bound):
    P, H, W = case.outer, case.H, case.W
    Wh = W // 2 + 1
    x = torch.randn(P, H, W, generator=gen)
    xd = r.dev(x)
    scale = 1.0 / math.sqrt(H * W)
    out = r.guarded(P * H * Wh * 2)
    r.check(r.rfft2(xd, out.t, P, H, W, scale))
    res = torch.view_as_complex(out.t.view(P, H, Wh, 2).cpu())
    assert out.guards_intact(), "write outside the half spectrum"
    assert torch.equal(xd.cpu(), x)
    ref = torch.fft.rfft2(x.double(), norm="ortho")
    err = worst_line_error(res, ref)
    assert err < bound, f"{case.id}: worst per-row error {err:.3g} >= {bound:.3g}"
    again = r.guarded(P * H * Wh * 2)
    r.check(r.rfft2(xd, again.t, P, H, W, scale))
    assert torch.equal(again.bits(), out.bits()), "two identical calls differ"
    return err


def _run_irfft2(r, case, gen, bound):
    """the input is an arbitrary (non-Hermitian) half spectrum: its DC and Nyquist bins carry imaginary parts, which c2r ignores"""
    P, H, W = case.outer, case.H, case.W
    Wh = W // 2 + 1
    spec = _randc((P, H, Wh), gen).to(torch.complex64)
    assert bool((spec[..., 0].imag != 0).all()) and (W % 2 or bool((spec[..., -1].imag != 0).all()))
    sr = torch.view_as_real(spec).contiguous()
    sd = r.dev(sr)
    scale = 1.0 / math.sqrt(H * W)
    ws = r.guarded(P * H * Wh * 2)                   # dinv_irfft2's workspace: P*H*(W/2+1) complex
    out = r.guarded(P * H * W)
    r.check(r.irfft2(sd, out.t, ws.t, P, H, W, scale))
    res = out.t.view(P, H, W).cpu()
    assert out.guards_intact(), "write outside the output"
    assert ws.guards_intact(), "write outside the workspace"
    assert torch.equal(sd.cpu(), sr), "irfft2 modified its input"
    ref = torch.fft.irfft2(spec.to(torch.complex128), s=(H, W), norm="ortho")
    err = worst_line_error(res, ref)
    assert err < bound, f"{case.id}: worst per-row error {err:.3g} >= {bound:.3g}"
    ws2, again = r.guarded(P * H * Wh * 2), r.guarded(P * H * W)
    r.check(r.irfft2(sd, again.t, ws2.t, P, H, W, scale))
    assert torch.equal(again.bits(), out.bits()), "two identical calls differ"
    return err


def _run_blurfft(r, case, gen, bound):
    P, H, W, Ps = case.outer, case.H, case.W, case.Ps
    Wh = W // 2 + 1
    x = torch.randn(P, H, W, generator=gen)
    m = torch.rand(Ps, H, Wh, 2, generator=gen) + 0.05
    m[:, 0, 0] = 1e-7                                # a singular value below the pseudo-inverse's threshold
    ph_ = torch.rand(Ps, H, Wh, generator=gen) * 6.28
    a = torch.polar(torch.ones_like(ph_), ph_).contiguous()
    xd, md, ad = r.dev(x), r.dev(m), r.dev(torch.view_as_real(a))
    nb = int(r.lib.dinv_blurfft_workspace_bytes(ctypes.c_int64(P), ctypes.c_int32(H), ctypes.c_int32(W)))
    X = torch.fft.rfft2(x.double(), norm="ortho")
    add, scale = 1.0 / 1.3, 1.0 / (H * W)
    worst = 0.0
    for flags in case.extra.get("flags", BLURFFT_FLAGS):
        ws = r.guarded(nb // 4)
        out = r.guarded(P * H * W)
        r.check(r.blurfft(xd, out.t, ws.t, P, H, W, md, ad, Ps, flags, add, scale))
        res = out.t.view(P, H, W).cpu()
        assert out.guards_intact(), f"flags {flags:#x}: write outside the output"
        assert ws.guards_intact(), f"flags {flags:#x}: write outside the workspace"
        ref = torch.fft.irfft2(_symbol_ref(X, m, a, flags, add), s=(H, W), norm="ortho")
        err = worst_line_error(res, ref)
        assert err < bound, f"{case.id} flags {flags:#x}: worst per-row error {err:.3g} >= {bound:.3g}"
        worst = max(worst, err)
        bits = out.bits().clone()
        del out, res
        again = r.guarded(P * H * W)
        r.check(r.blurfft(xd, again.t, ws.t, P, H, W, md, ad, Ps, flags, add, scale))
        assert torch.equal(again.bits(), bits), f"flags {flags:#x}: two identical calls differ"
    assert torch.equal(xd.cpu(), x)
    return worst
