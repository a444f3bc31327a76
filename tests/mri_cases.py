"""Shared by tests/test_mri_gpu.py (the gfx950 library) and tests/test_emu_mri_cases.py (the same kernel sources on the host
emulation): one table of MultiCoilMRI cases for csrc/mri.hip and csrc/mri_wave.hpp, each meant to reach named pipelines of
dinv_mri_forward (A), dinv_mri_adjoint (A^T) and dinv_mri_normal (A^T A) at one of their edges, the runner that calls them on
guarded buffers, and the complex128 references.

expected_kernels(case, op) restates the dispatch of the C sources (wave2d_ok, all_static with its W >= 64 rule, the fused expand
rule Q0 % 4 == 0 && N0 > 16, normal_ok, DINV_STATIC_SIZES, the rows-pass choice of fft_launch.hpp, the LDS limit of the combine
tile); on the emulation every call's launch log must match it.

Errors are measured per image against a scale that does not cancel: for A, ||y_bn - ref|| / ||S_n x_b||; for A^T,
||x_b - ref|| / sum_n ||S_bn||_inf ||M o y_bn||; for A^T A the same with M o M o F(S_n x_b) in place of y."""
import ctypes
import math
from dataclasses import dataclass

import torch

import fft_cases as F
from fft_cases import Guarded       # the guarded buffers of the FFT table

from deepinv_amd.hip import MriDesc


# ------------------------------------------------------------------ fp64 references (deepinv/physics/mri.py:254-324)
def _cfft(z, dims, inverse=False):
    f = torch.fft.ifftn if inverse else torch.fft.fftn
    return torch.fft.fftshift(f(torch.fft.ifftshift(z, dim=dims), dim=dims, norm="ortho"), dim=dims)


def _ref_forward(x, maps, mask):
    """x [B,2,*vol], maps complex [1|B,N,*vol], mask [1|B,2,*vol] -> y [B,2,N,*vol] in fp64"""
    xc = torch.complex(x[:, 0], x[:, 1]).to(torch.complex128)
    dims = tuple(range(-(x.ndim - 2), 0))
    k = _cfft(maps.to(torch.complex128) * xc[:, None], dims)
    y = torch.stack([k.real, k.imag], 1)
    return y * mask.double()[:, :, None]


def _ref_adjoint(y, maps, mask):
    """y [B,2,N,*vol] -> x [B,2,*vol] in fp64"""
    dims = tuple(range(-(y.ndim - 3), 0))
    ym = y.double() * mask.double()[:, :, None]
    u = _cfft(torch.complex(ym[:, 0], ym[:, 1]), dims, inverse=True)
    xc = (maps.to(torch.complex128).conj() * u).sum(1)
    return torch.stack([xc.real, xc.imag], 1)


# ------------------------------------------------------------------ error bounds (max over images of the measures above)
# Measured on the host emulation of the kernel sources (`python -m pytest tests/test_emu_mri_cases.py -s` prints every case's
# worst image per operator): the worst of each path family over its emulated cases, and the bound at about 4x that.
BOUNDS = {
    "A-wave": 9e-7,               # worst 2.3e-7 (512x256-b2-n1)
    "A-static": 8e-7,             # worst 2.0e-7 (32x32x128-b1-n2)
    "A-generic": 5.5e-6,          # worst 1.4e-6 (2x5851: one radix-5851 generic stage, 5851-term fp32 sums)
    "AT-wave": 8e-7,              # worst 2.0e-7 (320x320-b1-n1, no maps)
    "AT-static": 8e-7,            # worst 2.0e-7 (16x32x64-b2-n1, no maps)
    "AT-rows-static": 2e-7,       # worst 5.1e-8 (24x128-b2-n2)
    "AT-rows-generic": 6e-7,      # worst 1.4e-7 (17x11-b2-n1, single coil)
    "AT-rows-split": 5.5e-6,      # worst 1.4e-6 (2x5851, the rows pass's own limit)
    "ATA-wave": 1.3e-6,           # worst 3.3e-7 (512x320-b1-n2, no maps)
    "ATA-static": 1.3e-6,         # worst 3.1e-7 (16x32x64-b2-n3, no maps)
}

# ------------------------------------------------------------------ dispatch facts of csrc/mri.hip, mri_wave.hpp (restated)
STATIC = (16, 32, 64, 128, 256, 320, 512)          # has_static_plan
STATIC_ROWS = F.STATIC_ROWS                        # DINV_STATIC_SIZES: the rows passes with static kernels
WAVE_SIZES = (256, 320, 512)                       # wave2d_ok: H = R * 64 and W
KMAX_GRID = F.KMAX_GRID
RESIDENT_WAVES = 256 * 4 * 2                       # resident_waves_grid on 256 CUs at DINV_MRIW_MINW = 2
C2C_COLS = {0: "(fft_cols_static_kernel<P, Io, false, L>) x256", 1: "(fft_cols_static_kernel<P, Io, true, L>) x256"}
C2C_COLS_GENERIC = {0: "(fft_cols_kernel<Io, false>) x256", 1: "(fft_cols_kernel<Io, true>) x256"}
C2C_ROWS_GENERIC_INV = "(fft_rows_kernel<Io, true>) x256"
# (the C2CIo passes are instantiated first by csrc/fft.hip, which the emulation builds without instance logging: their log entry
# is the spelling of the launch)


def plan_generic(n):
    """the plan's `generic` flag: a prime factor above 5"""
    m = n
    for p in (2, 3, 5):
        while m % p == 0:
            m //= p
    return m > 1 or n == 1


def combine_lds(n):
    """LDS bytes of mri_rows_combine_kernel: the rows tile of min(lpb, 16) lines + an lpb x LS accumulator"""
    g = plan_generic(n)
    lpb = min(F.rows_lines_per_block(n, g), 16)
    return F.fft_lds_bytes(n, g, lpb) + lpb * (n + 1 if n % 2 == 0 else n) * 8


def rows_lds(n):
    g = plan_generic(n)
    return F.fft_lds_bytes(n, g, F.rows_lines_per_block(n, g))


def width_limits():
    """{(rule, generic): largest admitted width} for the combine tile and the rows pass, and the next width of that kind"""
    out = {}
    for g in (True, False):
        ns = [n for n in range(2, 9000) if plan_generic(n) == g and n not in STATIC_ROWS]
        for rule, f in (("combine", combine_lds), ("rows", rows_lds)):
            top = max(n for n in ns if f(n) <= F.KMAX_LDS)
            out[(rule, g)] = (top, min(n for n in ns if n > top))
    return out


def wave2d_ok(c, op):
    if len(c.vol) != 2:
        return False
    H, W = c.vol
    if H not in WAVE_SIZES or W not in WAVE_SIZES:
        return False
    if op != 0 and c.B * 64 < 1024 and c.hook != 1:
        return False
    return True


def all_static(c):
    return all(n in STATIC for n in c.vol) and c.vol[-1] >= 64


def normal_ok(c):
    return all_static(c) and c.vol[-1] in STATIC_ROWS


def expand_ok(c):
    vol = math.prod(c.vol)
    return (vol // c.vol[0]) % 4 == 0 and c.vol[0] > 16


def combine_cached(c):
    """mri_coil_combine_kernel<8> keeps the maps of a pixel quad in registers: shared maps and at most 8 coils"""
    return c.maps != "none" and c.maps_b <= 1 and c.N <= 8


def _rows_static(n, io, inverse, nlines, R):
    """fft_launch.hpp launch_rows_static_L: wave (N >= 256, io with Raw4, R % LW == 0), else v4, else scalar"""
    if io == "RowsCoilLoadIo":           # no vec4 loads
        return f"fft_rows_static_kernel<{n}, {io}, {'true' if inverse else 'false'}, {F.rows_tile(n)}> x256"
    if n >= 256:
        store = io == "RowsPlanarMaskStoreIo"
        m1 = {256: 32 if store else 64, 320: 40 if store else 64, 512: 64}[n]     # M1 of PlanForS / PlanFor
        lw = 8 if m1 // 4 <= 8 else 4
        if R % lw == 0:
            return f"fft_rows_wave_kernel<{n}, {io}, {'true' if inverse else 'false'}, {lw}, 4, 2, true> x256"
    return f"fft_rows_static_v4_kernel<{n}, {io}, {'true' if inverse else 'false'}, {F.rows_tile(n)}> x256"


def _cols(n, io, inverse):
    if n in STATIC:
        return f"fft_cols_static_kernel<{n}, {io}, {'true' if inverse else 'false'}, {F.cols_tile(n)}> x256"
    return f"fft_cols_kernel<{io}, {'true' if inverse else 'false'}> x256"


def _c2c_cols(n, inverse):
    return C2C_COLS[inverse] if n in STATIC else C2C_COLS_GENERIC[inverse]


def expected_kernels(c, op):
    """the instantiations (as the emulation's launch log prints them) that op 0 = A, 1 = A^T, 2 = A^T A of case c launches"""
    vol = math.prod(c.vol)
    nd, W, N0 = len(c.vol), c.vol[-1], c.vol[0]
    R = vol // W
    if wave2d_ok(c, op):
        Rr = c.vol[0] // 64
        if op == 0:
            return [f"mriw::rows_dif_kernel<{W}, {Rr}, false, 4> x256", f"mriw::cols64_kernel<{Rr}, 0, 4> x256"]
        if op == 1:
            return [f"mriw::rows_dif_kernel<{W}, {Rr}, true, 4> x256",
                    f"mriw::cols64_combine_kernel<{Rr}, 4, {'false' if c.maps == 'none' else 'true'}> x256"]
        return [f"mriw::rows_dif_kernel<{W}, {Rr}, false, 4> x256", f"mriw::cols64_kernel<{Rr}, 2, 4> x256",
                f"mriw::rows_combine_kernel<{W}, {Rr}, 4> x256"]
    mid = [_c2c_cols(c.vol[1], 0)] if nd == 3 else []
    mid_inv = [_c2c_cols(c.vol[1], 1)] if nd == 3 else []
    if op == 2 and not normal_ok(c):
        return []
    if all_static(c) and op in (0, 2):
        first = [f"mri_cols_expand_fwd_kernel<{N0}, 16, 256> x256"] if expand_ok(c) else [_cols(N0, "ColsCoilLoadIo", 0)]
        if op == 0:
            return first + mid + [_rows_static(W, "RowsPlanarMaskStoreIo", 0, c.B * c.N * R, R)]
        last = ([C2C_COLS[1], "mri_coil_combine_kernel<8> x256"] if vol % 4 == 0 and N0 > 16
                else [f"mri_cols_combine_inv_kernel<{N0}, 256, 256> x256"])
        L = {512: 4, 320: 4, 256: 8, 128: 16}.get(W, 32)          # RowsNormalL
        return first + mid + [f"mri_rows_normal_kernel<{W}, {L}> x256"] + mid_inv + last
    if all_static(c):
        last = ([C2C_COLS[1], "mri_coil_combine_kernel<8> x256"] if vol % 4 == 0 and N0 > 16
                else [f"mri_cols_combine_inv_kernel<{N0}, 256, 256> x256"])
        return [_rows_static(W, "RowsPlanarMaskLoadIo", 1, c.B * c.N * R, R)] + mid_inv + last
    if op == 0:
        rows = (_rows_static(W, "RowsCoilLoadIo", 0, c.B * c.N * R, R) if W in STATIC_ROWS
                else "fft_rows_kernel<RowsCoilLoadIo, false> x256")
        return [rows] + mid + [_cols(N0, "ColsPlanarMaskStoreIo", 0)]
    first = [_cols(N0, "ColsPlanarMaskLoadIo", 1)] + mid_inv
    if W in STATIC_ROWS:
        return first + [f"mri_rows_combine_static_kernel<{W}, {F.rows_tile(W)}> x256"]
    if combine_lds(W) <= F.KMAX_LDS:
        return first + ["mri_rows_combine_kernel x256"]
    return first + [C2C_ROWS_GENERIC_INV, "mri_coil_combine_any_kernel x256"]


def family(c, op):
    """key of BOUNDS for op of case c"""
    if wave2d_ok(c, op):
        return ("A", "AT", "ATA")[op] + "-wave"
    if op == 2:
        return "ATA-static"
    if all_static(c):
        return ("A", "AT")[op] + "-static"
    if op == 0:
        return "A-generic"
    W = c.vol[-1]
    if W in STATIC_ROWS:
        return "AT-rows-static"
    return "AT-rows-generic" if combine_lds(W) <= F.KMAX_LDS else "AT-rows-split"


def normalise(entry):
    """a launch-log entry with every StaticPlan<N, r1, r2, r3> written as N"""
    out, i = [], 0
    while True:
        j = entry.find("StaticPlan<", i)
        if j < 0:
            out.append(entry[i:])
            return "".join(out)
        k = entry.index(">", j)
        out.append(entry[i:j] + entry[j + len("StaticPlan<"):k].split(",")[0])
        i = k + 1


# ------------------------------------------------------------------ the case table
@dataclass
class Case:
    id: str
    vol: tuple
    B: int = 1
    N: int = 1
    maps: str = "shared"        # none | shared | per (maps_batch 0 | 1 | B)
    mask: str = "shared"        # none | shared | per
    hook: int = 0               # dinv_mri_desc.reserved = 1: the wave pipelines of A^T / A^T A below B = 16
    coil_dim: int = 1
    emu: bool = True
    kind: str = "op"            # op | reject (both A and A^T must refuse: a width above the rows pass's LDS limit)
    tag: str = ""

    @property
    def maps_b(self):
        return {"none": 0, "shared": 1, "per": self.B}[self.maps]

    @property
    def mask_b(self):
        return {"none": 0, "shared": 1, "per": self.B}[self.mask]


def _case(cases, vol, B=1, N=1, maps="shared", mask="shared", hook=0, emu=True, tag="", **kw):
    cid = "x".join(map(str, vol)) + f"-b{B}-n{N}-maps{maps[:3]}-mask{mask[:3]}" + ("-hook" if hook else "") + tag
    cases.append(Case(cid, tuple(vol), B, N, maps, mask, hook, emu=emu, tag=tag, **kw))


def build_cases():
    cases = []
    # wave pipelines (2-D, H and W in {256, 320, 512}: R = 4, 5, 8), with the test hook for A^T / A^T A
    maps_cycle, mask_cycle = ("shared", "none", "per"), ("per", "shared", "none")
    for i, H in enumerate(WAVE_SIZES):
        for j, W in enumerate(WAVE_SIZES):
            k = i * 3 + j
            B = 2 if maps_cycle[k % 3] == "per" or mask_cycle[k % 3] == "per" else 1
            _case(cases, (H, W), B, 1 + (k % 2), maps_cycle[k % 3], mask_cycle[(k + i) % 3], hook=1)
    # the natural threshold of A^T / A^T A: B * 64 >= 1024 (B = 15: cooperative, B = 16: wave)
    _case(cases, (256, 256), 15, 1, "per", "per")
    _case(cases, (256, 256), 16, 1, "per", "per")
    _case(cases, (256, 320), 16, 1, "none", "shared")
    # static pipeline, fused expand (first axis 32 ... 512), 2-D and 3-D; rows_normal at every W with the expand first pass
    for H, W in ((32, 64), (64, 128), (128, 64), (256, 64), (320, 64), (512, 64), (32, 128), (32, 256), (32, 320), (32, 512),
                 (64, 256)):
        _case(cases, (H, W), 2, 2, "per" if H % 64 else "shared", "per" if W % 128 else "shared")
    for vol in ((32, 16, 64), (64, 32, 64), (32, 32, 128), (128, 16, 64)):
        _case(cases, vol, 1, 2, "shared", "shared")
    # static pipeline with a depth-16 first axis (ColsCoilLoadIo; A^T / A^T A end in mri_cols_combine_inv_kernel<16>); rows_normal
    # at every W with that first / last pass
    for W in STATIC_ROWS:
        _case(cases, (16, W), 2, 2, "per", "per")
    for N, maps in ((1, "none"), (2, "shared"), (3, "per"), (4, "per"), (5, "shared"), (3, "none"), (1, "per"), (5, "per")):
        _case(cases, (16, 32, 64), 2, N, maps, "shared" if N % 2 else "per")
    # mri_coil_combine_kernel<8>: cached maps up to 8 coils, the chunked loop above; batches around CB = 4
    for N, maps, B in ((1, "shared", 1), (7, "per", 4), (8, "shared", 5), (8, "none", 1), (9, "shared", 4), (9, "per", 9),
                       (16, "none", 5), (16, "shared", 9), (17, "per", 5), (17, "shared", 1), (7, "shared", 9)):
        _case(cases, (32, 64), B, N, maps, "per" if B % 2 else "shared")
    # rows_combine_static at every static W behind a non-static first axis (the forward: scalar static rows + generic columns)
    for H, W in ((17, 64), (24, 128), (9, 256), (5, 320), (3, 512)):
        _case(cases, (H, W), 2, 2, "per", "per")
    # generic pipeline: W < 64, odd, prime; a 3-D volume with a non-static middle axis
    for vol, N in (((16, 16), 2), ((8, 32), 3), ((6, 17), 2), ((5, 31), 1), ((7, 45), 2), ((16, 17, 64), 2), ((4, 17, 12), 2)):
        _case(cases, vol, 2, N, "per", "per")
    _case(cases, (17, 11), 2, 1, "none", "per")
    # the width limits of A^T: the combine tile's largest widths (generic / smooth), the next ones (the split route), the rows
    # pass's largest (split route) and the next (both A and A^T refuse)
    lim = width_limits()
    for g in (True, False):
        top, nxt = lim[("combine", g)]
        _case(cases, (2, top), 1, 2, "shared", "shared", tag="-combine-limit")
        _case(cases, (2, nxt), 1, 2, "shared", "shared", tag="-split")
        _case(cases, (2, nxt), 3, 2, "per", "per", tag="-split")      # per-sample maps and masks: the batch offsets of the split route
        top, nxt = lim[("rows", g)]
        _case(cases, (2, top), 1, 1, "none", "none", tag="-rows-limit")
        cases.append(Case(f"2x{nxt}-width-reject", (2, nxt), 1, 1, "none", "none", kind="reject"))
    # single-coil MRI layout (coil_dim = 0)
    _case(cases, (32, 64), 2, 1, "none", "per", coil_dim=0, tag="-single")
    _case(cases, (17, 11), 2, 1, "none", "shared", coil_dim=0, tag="-single")
    # grid edges (device only): past kMaxGrid tiles of the static rows / columns / combine passes, past 4 x kMaxGrid blocks of
    # the expand, combine_inv and rows_normal passes, past the resident grid of the wave passes
    _case(cases, (32, 128, 64), 2, 9, "shared", "per", emu=False, tag="-grid-expand")
    _case(cases, (16, 256, 512), 2, 5, "shared", "shared", emu=False, tag="-grid-rows-normal")
    _case(cases, (16, 64, 64), 520, 1, "shared", "shared", emu=False, tag="-grid-combine-inv")
    _case(cases, (1000, 64), 66, 1, "shared", "per", emu=False, tag="-grid-rows-combine")
    _case(cases, (256, 256), 16, 9, "shared", "shared", emu=False, tag="-grid-wave")
    _case(cases, (320, 320), 48, 2, "per", "shared", emu=False, tag="-grid-wave-combine")
    ids = [c.id for c in cases]
    assert len(ids) == len(set(ids)), "duplicate case ids"
    return cases


CASES = build_cases()


def grid_facts(c):
    """(launcher, blocks or tiles it needs) of the grid-capped launches of case c (A^T and A^T A included)"""
    vol = math.prod(c.vol)
    W, N0, P = c.vol[-1], c.vol[0], c.B * c.N
    R, Q0 = vol // W, vol // N0
    out = {}
    if wave2d_ok(c, 0):
        Rr = N0 // 64
        out["rows_dif waves"] = P * 64
        out["cols64 waves"] = P * Rr * (W // 32)
        out["cols64_combine waves"] = c.B * Rr * (W // 32)
        out["rows_combine waves"] = c.B * 64
        return out
    if all_static(c):
        if expand_ok(c):
            out["expand blocks"] = -(-c.B * -(-Q0 // 16) // 8) * 8 * c.N
        else:
            out["combine_inv tiles"] = c.B * -(-Q0 // F.cols_tile(N0))
        L = {512: 4, 320: 4, 256: 8, 128: 16}.get(W, 32)
        out["rows_normal tiles"] = -(-P * R // L)
        out["rows tiles"] = -(-P * R // F.rows_tile(W))
        out["cols tiles"] = P * -(-Q0 // F.cols_tile(N0))
    elif W in STATIC_ROWS:
        out["combine_static tiles"] = -(-c.B * R // F.rows_tile(W))
    return out


# ------------------------------------------------------------------ inputs
def inputs(c, gen):
    """x [B,2,*vol], maps complex64 [mb,N,*vol] or None, mask [mb,2,*vol] or None (non-binary, exact zeros, distinct channels),
    v [B,2,N,*vol]"""
    x = torch.randn(c.B, 2, *c.vol, generator=gen)
    maps = None
    if c.maps != "none":
        mb = c.maps_b
        maps = (torch.complex(torch.randn(mb, c.N, *c.vol, generator=gen), torch.randn(mb, c.N, *c.vol, generator=gen))
                / math.sqrt(2 * c.N)).to(torch.complex64)
    mask = None
    if c.mask != "none":
        m = torch.rand(c.mask_b, 2, *c.vol, generator=gen)
        mask = torch.where(m < 0.3, torch.zeros_like(m), 0.25 + m)
    v = torch.randn(c.B, 2, c.N, *c.vol, generator=gen)
    return x, maps, mask, v


def _full_maps(c, maps):
    if maps is None:
        return torch.ones(1, c.N, *c.vol, dtype=torch.complex128)
    return maps.to(torch.complex128)


def _full_mask(c, mask):
    return torch.ones(1, 2, *c.vol, dtype=torch.float64) if mask is None else mask.double()


CHUNK_PIXELS = 1 << 23      # the references work on slices of at most this many image-coil pixels (the grid cases)


def _chunks(c):
    step = max(1, CHUNK_PIXELS // (c.N * math.prod(c.vol)))
    for b0 in range(0, c.B, step):
        yield b0, min(c.B, b0 + step)


def _sl(t, b0, b1):
    return t if t.shape[0] == 1 else t[b0:b1]


def err_forward(c, y, x, maps, mask):
    """max over (b, n) of ||y - ref|| / ||S_n x_b||"""
    S, M = _full_maps(c, maps), _full_mask(c, mask)
    worst = 0.0
    dims = tuple(range(2, 2 + len(c.vol)))
    for b0, b1 in _chunks(c):
        xb = x[b0:b1]
        ref = _ref_forward(xb, _sl(S, b0, b1), _sl(M, b0, b1))
        got = y[b0:b1].reshape(ref.shape).double()
        num = (got - ref).pow(2).sum((1,) + tuple(d + 1 for d in dims)).sqrt()                  # [b, n]
        xc = torch.complex(xb[:, 0], xb[:, 1]).to(torch.complex128)
        den = (_sl(S, b0, b1) * xc[:, None]).abs().pow(2).sum(dims).sqrt()
        e = num / den
        if torch.isnan(e).any():
            return float("inf")
        worst = max(worst, float(e.max()))
    return worst


def _adj_measure(c, out, z, S, b0, b1):
    """max over b of ||out_b - ref_b|| / sum_n ||S_bn||_inf ||z_bn||; z [b,2,N,*vol] the (masked) k-space the adjoint reads"""
    nd = len(c.vol)
    dims = tuple(range(-nd, 0))
    u = _cfft(torch.complex(z[:, 0], z[:, 1]), dims, inverse=True)
    Sb = _sl(S, b0, b1)
    ref = (Sb.conj() * u).sum(1)
    ref = torch.stack([ref.real, ref.imag], 1)
    got = out[b0:b1].double()
    num = (got - ref).reshape(b1 - b0, -1).pow(2).sum(1).sqrt()
    sinf = Sb.abs().reshape(Sb.shape[0], c.N, -1).amax(-1)                       # [1|b, N]
    zn = z.pow(2).sum(1).reshape(b1 - b0, c.N, -1).sum(-1).sqrt()              # [b, N]
    den = (sinf * zn).sum(1)
    e = num / den
    if torch.isnan(e).any():
        return float("inf")
    return float(e.max())


def err_adjoint(c, xa, v, maps, mask):
    S, M = _full_maps(c, maps), _full_mask(c, mask)
    worst = 0.0
    for b0, b1 in _chunks(c):
        z = v[b0:b1].double() * _sl(M, b0, b1)[:, :, None]
        worst = max(worst, _adj_measure(c, xa, z, S, b0, b1))
    return worst


def err_normal(c, out, x, maps, mask):
    S, M = _full_maps(c, maps), _full_mask(c, mask)
    worst = 0.0
    for b0, b1 in _chunks(c):
        Mb = _sl(M, b0, b1)
        z = _ref_forward(x[b0:b1], _sl(S, b0, b1), Mb) * Mb[:, :, None]
        worst = max(worst, _adj_measure(c, out, z, S, b0, b1))
    return worst


def err_between(c, a, b, maps, mask, x):
    """A^T A x against A^T(A x) of the library, on the scale of the A^T A measure"""
    S, M = _full_maps(c, maps), _full_mask(c, mask)
    worst = 0.0
    for b0, b1 in _chunks(c):
        Mb, Sb = _sl(M, b0, b1), _sl(S, b0, b1)
        z = _ref_forward(x[b0:b1], Sb, Mb) * Mb[:, :, None]
        num = (a[b0:b1].double() - b[b0:b1].double()).reshape(b1 - b0, -1).pow(2).sum(1).sqrt()
        sinf = Sb.abs().reshape(Sb.shape[0], c.N, -1).amax(-1)
        zn = z.pow(2).sum(1).reshape(b1 - b0, c.N, -1).sum(-1).sqrt()
        worst = max(worst, float((num / (sinf * zn).sum(1)).max()))
    return worst


# ------------------------------------------------------------------ the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip), `device` of its buffers,
    `stream()` -> the stream argument, `fft_plan(n)` -> (plan struct, table tensor on the device), and - on the emulation -
    `reset()` / `launches()`, the instantiations launched since the last reset"""

    def __init__(self, lib, device, stream, fft_plan, reset=None, launches=None):
        self.lib, self.device, self._stream, self.fft_plan = lib, torch.device(device), stream, fft_plan
        self.reset, self.launches = reset, launches
        self.keep = []

    def err(self):
        return self.lib.dinv_last_error().decode()

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def dev(self, t):
        if t is None:
            return None
        d = t.contiguous().to(self.device)
        self.keep.append(d)
        return d

    def desc(self, c):
        d = MriDesc()
        d.batch, d.coils, d.ndim = c.B, c.N, len(c.vol)
        for i, n in enumerate(c.vol):
            d.dims[i] = n
            plan, table = self.fft_plan(n)
            d.plan[i] = plan
            d.table[i] = table.data_ptr()
            self.keep.append(table)
        d.mask_batch, d.maps_batch, d.coil_dim, d.reserved = c.mask_b, c.maps_b, c.coil_dim, c.hook
        return d

    def guarded(self, n):
        return Guarded(n, self.device)

    def ws_bytes(self, d):
        return int(self.lib.dinv_mri_workspace_bytes(ctypes.byref(d)))

    def call(self, fn, d, inp, maps, mask, out, ws, ws_bytes=None, expect=None):
        """fn in forward | adjoint | normal; maps a complex64 device tensor or None; returns the status"""
        if self.reset:
            self.reset()
        p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
        mp = None if maps is None else torch.view_as_real(maps)
        nb = ws.n * 4 if ws_bytes is None else ws_bytes
        rc = getattr(self.lib, f"dinv_mri_{fn}")(ctypes.byref(d), p(inp), p(mp), p(mask), p(out), p(ws.t), ctypes.c_size_t(nb),
                                                  self._stream())
        if expect is not None and self.launches is not None:
            got = [normalise(s) for s in self.launches()]
            assert got == expect, (f"{fn}: launched {got}, the restated dispatch expects {expect}" +
                                   (f" (status {rc}: {self.err()})" if rc else ""))
        return rc

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: error {rc}: {self.err()}")


def _seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id)) % (2 ** 31)


def _zero_pattern_ok(y, mask, c):
    """wherever a mask channel is 0 the output is exactly 0 in that channel"""
    if mask is None:
        return True
    m = mask[:, :, None].expand(c.B, 2, c.N, *c.vol)
    return bool((y.reshape(c.B, 2, c.N, *c.vol)[m == 0] == 0).all())


def _op(r, c, d, fn, inp_dev, maps_d, mask_d, out_words, op):
    """one call on guarded output and workspace; returns the output (host) after the guard / input / determinism checks"""
    wsb = r.ws_bytes(d)
    ws, out = r.guarded(wsb // 4), r.guarded(out_words)
    before = inp_dev.cpu().clone()
    r.check(r.call(fn, d, inp_dev, maps_d, mask_d, out.t, ws, expect=expected_kernels(c, op)), f"{c.id} {fn}")
    r.sync()
    assert out.guards_intact(), f"{c.id} {fn}: write outside the output"
    assert ws.guards_intact(), f"{c.id} {fn}: write outside the workspace of dinv_mri_workspace_bytes"
    res = out.t.cpu().clone()
    assert not torch.isnan(res).any(), f"{c.id} {fn}: output not fully written"
    assert torch.equal(inp_dev.cpu(), before), f"{c.id} {fn}: the call modified its input"
    del out, ws
    ws2, again = r.guarded(wsb // 4), r.guarded(out_words)
    r.check(r.call(fn, d, inp_dev, maps_d, mask_d, again.t, ws2), f"{c.id} {fn} (again)")
    r.sync()
    assert torch.equal(again.t.cpu().view(torch.int32), res.view(torch.int32)), f"{c.id} {fn}: two identical calls differ"
    return res


def run_case(r, c):
    """runs every operator case c reaches on runner r, asserts everything it checks, returns {op: worst error}"""
    r.keep = []
    gen = torch.Generator().manual_seed(_seed(c))
    x, maps, mask, v = inputs(c, gen)
    d = r.desc(c)
    xd, vd, maps_d, mask_d = r.dev(x), r.dev(v), r.dev(maps), r.dev(mask)
    maps_keep = None if maps is None else maps.clone()
    mask_keep = None if mask is None else mask.clone()
    vol = math.prod(c.vol)
    if c.kind == "reject":
        for fn, inp, words in (("forward", xd, c.B * 2 * c.N * vol), ("adjoint", vd, c.B * 2 * vol)):
            ws, out = r.guarded(r.ws_bytes(d) // 4), r.guarded(words)
            rc = r.call(fn, d, inp, maps_d, mask_d, out.t, ws)
            r.sync()
            assert rc != 0 and "LDS" in r.err(), f"{c.id} {fn}: width above the rows pass's LDS limit accepted"
            assert out.untouched() and ws.untouched(), f"{c.id} {fn}: a refused call wrote"
        return {}
    errs = {}
    # A
    y = _op(r, c, d, "forward", xd, maps_d, mask_d, c.B * 2 * c.N * vol, 0)
    e = err_forward(c, y.view(c.B, 2, c.N, *c.vol), x, maps, mask)
    errs["A"] = e
    assert e < BOUNDS[family(c, 0)], f"{c.id} A: worst image error {e:.3g} >= {BOUNDS[family(c, 0)]:.3g} ({family(c, 0)})"
    assert _zero_pattern_ok(y, mask, c), f"{c.id} A: a masked sample is not an exact zero"
    # A^T
    xa = _op(r, c, d, "adjoint", vd, maps_d, mask_d, c.B * 2 * vol, 1).view(c.B, 2, *c.vol)
    e = err_adjoint(c, xa, v, maps, mask)
    errs["AT"] = e
    assert e < BOUNDS[family(c, 1)], f"{c.id} A^T: worst image error {e:.3g} >= {BOUNDS[family(c, 1)]:.3g} ({family(c, 1)})"
    # <A x, v> = <x, A^T v>
    lhs, rhs = float((y.double() * v.reshape(-1).double()).sum()), float((x.reshape(-1).double() * xa.reshape(-1).double()).sum())
    scale = float(y.double().norm() * v.double().norm() + x.double().norm() * xa.double().norm())
    assert abs(lhs - rhs) <= 4e-6 * scale, f"{c.id}: dot test {lhs} vs {rhs}"
    # A^T A
    sup = int(r.lib.dinv_mri_normal_supported(ctypes.byref(d)))
    assert sup == (1 if normal_ok(c) else 0), f"{c.id}: dinv_mri_normal_supported = {sup}"
    if sup:
        xn = _op(r, c, d, "normal", xd, maps_d, mask_d, c.B * 2 * vol, 2).view(c.B, 2, *c.vol)
        e = err_normal(c, xn, x, maps, mask)
        errs["ATA"] = e
        assert e < BOUNDS[family(c, 2)], f"{c.id} A^T A: worst image error {e:.3g} >= {BOUNDS[family(c, 2)]:.3g}"
        # == A^T (A x) of the library, within the A^T A bound (worst emulated: 3.0e-7 wave at 512x320, 1.0e-7 static)
        yd = r.dev(y.view(c.B, 2, c.N, *c.vol))
        ws, xx = r.guarded(r.ws_bytes(d) // 4), r.guarded(c.B * 2 * vol)
        r.check(r.call("adjoint", d, yd, maps_d, mask_d, xx.t, ws), f"{c.id} A^T(A x)")
        r.sync()
        e2 = err_between(c, xn, xx.t.cpu().view(c.B, 2, *c.vol), maps, mask, x)
        errs["chain"] = e2
        assert e2 < BOUNDS[family(c, 2)], f"{c.id}: A^T A x vs A^T(A x): {e2:.3g} >= {BOUNDS[family(c, 2)]:.3g}"
        # symmetric: <A^T A x, u> = <x, A^T A u>
        u = torch.randn(c.B, 2, *c.vol, generator=gen)
        ud = r.dev(u)
        ws, nu = r.guarded(r.ws_bytes(d) // 4), r.guarded(c.B * 2 * vol)
        r.check(r.call("normal", d, ud, maps_d, mask_d, nu.t, ws), f"{c.id} A^T A u")
        r.sync()
        nu = nu.t.cpu()
        a, b = float((xn.reshape(-1).double() * u.reshape(-1).double()).sum()), float((x.reshape(-1).double() * nu.double()).sum())
        assert abs(a - b) <= 4e-6 * float(xn.double().norm() * u.double().norm() + x.double().norm() * nu.double().norm()), \
            f"{c.id}: A^T A not symmetric: {a} vs {b}"
    else:
        ws, out = r.guarded(r.ws_bytes(d) // 4), r.guarded(c.B * 2 * vol)
        rc = r.call("normal", d, xd, maps_d, mask_d, out.t, ws, expect=[])
        r.sync()
        assert rc != 0, f"{c.id}: dinv_mri_normal accepted sizes it does not support"
        assert out.untouched() and ws.untouched(), f"{c.id}: a refused dinv_mri_normal wrote"
    # the constant inputs stayed constant
    assert maps_d is None or torch.equal(maps_d.cpu(), maps_keep), f"{c.id}: coil maps modified"
    assert mask_d is None or torch.equal(mask_d.cpu(), mask_keep), f"{c.id}: mask modified"
    return errs


# ------------------------------------------------------------------ rejections (every entry point, nothing written)
def _rejections(r):
    """(name, desc, which maps / mask / workspace size to pass) of calls validate() or the entry points must refuse"""
    c = Case("reject-base", (32, 64), B=3, N=2, maps="shared", mask="shared")
    out = []

    def mk(name, edit=None, maps=True, mask=True, short=0, ops=("forward", "adjoint", "normal"), base=c):
        d = r.desc(base)
        if edit:
            edit(d)
        out.append((name, base, d, maps, mask, short, ops))

    mk("ndim-1", lambda d: setattr(d, "ndim", 1))
    mk("ndim-4", lambda d: setattr(d, "ndim", 4))
    mk("coils-0", lambda d: setattr(d, "coils", 0))
    mk("coil-dim-0-two-coils", lambda d: setattr(d, "coil_dim", 0))
    mk("plan-dims-mismatch", lambda d: d.plan.__setitem__(1, r.fft_plan(128)[0]))
    mk("null-table", lambda d: d.table.__setitem__(1, None))
    mk("mask-batch-2-of-3", lambda d: setattr(d, "mask_batch", 2))
    mk("maps-batch-without-pointer", maps=False)
    mk("maps-pointer-without-batch", lambda d: setattr(d, "maps_batch", 0))
    mk("mask-pointer-without-batch", lambda d: setattr(d, "mask_batch", 0))
    mk("workspace-one-byte-short", short=1)
    mk("normal-unsupported-size", ops=("normal",), base=Case("reject-normal", (17, 64), B=2, N=2))
    return out


def run_rejections(r):
    r.keep = []
    gen = torch.Generator().manual_seed(5)
    for name, c, d, use_maps, use_mask, short, ops in _rejections(r):
        x, maps, mask, v = inputs(c, gen)
        xd, vd = r.dev(x), r.dev(v)
        maps_d = r.dev(maps) if use_maps else None
        mask_d = r.dev(mask) if use_mask else None
        vol = math.prod(c.vol)
        for fn in ops:
            inp, words = (vd, c.B * 2 * vol) if fn == "adjoint" else (xd, c.B * 2 * (c.N if fn == "forward" else 1) * vol)
            wsb = c.B * c.N * vol * 8
            ws, out = r.guarded(wsb // 4), r.guarded(words)
            rc = r.call(fn, d, inp, maps_d, mask_d, out.t, ws, ws_bytes=wsb - short, expect=[])
            r.sync()
            assert rc != 0, f"{name}: dinv_mri_{fn} accepted the call"
            assert out.untouched(), f"{name}: refused dinv_mri_{fn} wrote to its output"
            assert ws.untouched(), f"{name}: refused dinv_mri_{fn} wrote to its workspace"


def run_empty(r):
    """B = 0: every entry point returns 0 and writes nothing"""
    r.keep = []
    c = Case("empty", (32, 64), B=0, N=2, maps="shared", mask="shared")
    d = r.desc(c)
    d.maps_batch = d.mask_batch = 1
    gen = torch.Generator().manual_seed(1)
    maps = r.dev(torch.randn(1, 2, 32, 64, dtype=torch.complex64, generator=gen))
    mask = r.dev(torch.rand(1, 2, 32, 64, generator=gen))
    assert r.ws_bytes(d) == 0
    for fn in ("forward", "adjoint", "normal"):
        ws, inp, out = r.guarded(0), r.guarded(16), r.guarded(16)
        assert r.call(fn, d, inp.t, maps, mask, out.t, ws, expect=[]) == 0, f"B = 0: dinv_mri_{fn}: {r.err()}"
        r.sync()
        assert out.untouched() and ws.untouched(), f"B = 0: dinv_mri_{fn} wrote"
