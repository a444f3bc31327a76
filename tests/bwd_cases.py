"""Shared by tests/test_bwd_gpu.py (the gfx950 library) and tests/test_emu_bwd.py (the same kernel sources on the host emulation):
one table of cases for the DRUNet / DnCNN TRAINING kernels - the weight gradients, the bias gradient and the ReLU
backward of csrc/drunet_bwd.hip, and the data gradients (the forward kernels on flipped / transposed packs, with their gate and
residual epilogues) as models/drunet_train.py and models/drunet3d.py call them - each meant to reach one path at one of its edges;
the fp64 references; a restatement of the launchers' arithmetic (slice counts, pixels per wave); and one runner.

Every case runs on three kinds of data:

  int     every element of both operands in {-2 .. 2}.  Every product and partial sum is an integer below 2^24 (4 * terms < 2^24),
          so the result must equal the fp64 reference BIT FOR BIT whatever the summation order, slice count or tile shape: a
          dropped, duplicated or misplaced pixel, tap, channel, slice or depth pairing fails, rounding cannot.
  wide    one operand in {-2 .. 2}, the other m / 1024 with |m| <= 4095: 12 significant bits, more than bf16 or tf32 hold.  Exact
          while terms * 8190 < 2^24 (weight gradients: B H W <= 2048; data gradients: 9 cin or 27 cin terms), and only if no
          operand loses mantissa bits on its way to the matrix cores.  In the bf16-split kernels the small-integer operand has a
          zero low part, so the product the split drops (low x low) is zero.  Run both ways round.
  randn   N(0, 1) data against a derived per-element ceiling |out - ref| <= gamma_n * (the same operation on absolute values),
          gamma_n = n u / (1 - n u), u = 2^-24, n = the length of the longest rounding chain read off the code (restated below);
          the bf16-split kernels keep the project's figure for them, relative l2 below 2e-5.

The weight- and bias-gradient calls go through ctypes on guarded buffers (fft_cases.Guarded): the workspace starts as NaN
(production passes torch.empty), dw / db start as NaN (accumulate = 0) or as integers (accumulate = 1: the result must be prefill +
gradient exactly), S's slack is NaN, L's slack is +-1e30 (the kernel's contract: "finite data in the slack, multiplied by S = 0").
"""
import ctypes
import functools
import math
import types
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from fft_cases import Guarded

U = 2.0 ** -24
SPLIT_L2 = 2e-5                   # the bound of test_split2d_conv_matches_fp64 / the bf16s down / up tests on the same kernels


def gamma(n):
    return n * U / (1 - n * U)


# ------------------------------------------------------------------ the launchers of csrc/drunet_bwd.hip, restated
def padded(B, H, W):
    """(hp, wp, plane, np) of dinv_act_geom_init"""
    hp, wp = H + 2, (W + 2 + 3) // 4 * 4
    return hp, wp, hp * wp, B * hp * wp


def part_count(np_, m, n):
    """part_count(): workgroups (pixel slices) per tile"""
    thin = m <= 16 and n <= 16
    tiles = 1 if thin else ((m + 31) // 32) * ((n + 31) // 32)
    return min(max(1, 512 // tiles), max(1, np_ // 512))


def per_wave(np_, nparts):
    """wgrad_launch: pixels per wave, whole iterations of 16"""
    return (-(-np_ // (4 * nparts)) + 15) // 16 * 16


def wgrad_chain(np_, m, n, accumulate):
    """longest rounding chain of one dw element: the per-wave chain, the four-wave sum, the two reduction rounds, the accumulate"""
    nparts = part_count(np_, m, n)
    return per_wave(np_, nparts) + 3 + -(-nparts // 16) + 16 + (1 if accumulate else 0)


def bias_slices(np_):
    """bias_grad_slices()"""
    return min(512, max(1, -(-np_ // 8192)))


def bias_chain(np_):
    ns = bias_slices(np_)
    return -(-(-(-np_ // ns)) // 256) + 8 + ns + 1


# ------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    id: str
    kind: str                     # wgrad3 | wgrad2 | wgrad2x2x2 | wgrad3x3x3 | bias | relu | gate | dgrad3 | dgrad2 | dgrad3d | dstride3d
    B: int = 1
    H: int = 1
    W: int = 1                    # on the S grid (stride-2 layers: the half grid)
    M: int = 0                    # dW's leading shape M x N (bias: M = channels; relu: M = length)
    N: int = 0
    D: int = 0                    # depth of the S grid (3-D kinds)
    up: bool = False              # stride-2 weight gradient of the transposed convolution (S = x) instead of the strided one (S = dL/dy)
    mode: str = "plain"           # data gradients: plain | res | gate
    fp32: bool = False            # data gradients: the fp32 argument of the call
    branch: str = ""              # data gradients: the kernel the call must take (restated dispatch, asserted)
    wname: str = "w"              # data gradients, 2-D: the parameter name Ops2d.weight pads by
    slices: int = 0               # expected slice count (asserted against the restatement: the table says what it reaches)
    gpu_only: bool = False
    gpu_only_classes: tuple = ()  # classes too slow for the host emulation (the fiber emulation of 17 slices x 2 tiles takes ~10 s a run)
    wide: bool = True             # False: terms * 8190 >= 2^24, `int` stands in for `wide` (reason in `note`)
    note: str = ""

    def classes(self):
        if self.kind in ("relu", "gate"):
            return ("special",)
        c = ["int"]
        if self.kind in ("wgrad3", "wgrad2", "wgrad2x2x2", "wgrad3x3x3", "bias"):
            c.append("int+acc")
        if self.wide:
            c += ["wide-s", "wide-l"] if self.kind != "bias" else ["wide-s"]
        return tuple(c + ["randn"])


def _terms_ok(c):
    return c.B * max(c.D, 1) * c.H * c.W <= 2048


CASES = []


def _add(**kw):
    c = Case(**kw)
    if c.kind.startswith("wgrad") or c.kind == "bias":
        if c.wide and not _terms_ok(c):
            c = Case(**{**kw, "wide": False, "note": "B H W > 2048: 8190 * terms reaches 2^24, `int` only"})
    CASES.append(c)


def _w3(B, H, W, M, N, slices=0, **kw):
    _add(id=f"w3-{B}x{H}x{W}-m{M}n{N}", kind="wgrad3", B=B, H=H, W=W, M=M, N=N, slices=slices, **kw)


_SLOW = ("int+acc", "wide-s", "wide-l")
_w3(1, 6, 6, 16, 16, 1)                       # np = 64: one slice shorter than a chunk, waves with nothing to do
_w3(1, 94, 90, 16, 16, 17)                    # np = 8832: 17 slices, per_wave 144, ragged last chunks, the 17th slice EMPTY, 2nd reduction round
_w3(1, 94, 93, 16, 16, 18)                    # np = 9216: 18 slices of 512 pixels, none empty: slices 16 and 17 are real terms of the 2nd round
_w3(1, 94, 90, 64, 3, 17, gpu_only_classes=_SLOW + ("randn",))     # 17 slices on two 32-tiles; L lanes beyond the 8 allocated channels
_w3(2, 30, 29, 24, 40, 4)                     # 4 slices; ragged tiles on both axes
_w3(2, 9, 14, 17, 16)                         # one channel past the thin kernel
_w3(2, 9, 14, 16, 17)
_w3(2, 9, 14, 2, 64)                          # DRUNet tail
_w3(2, 9, 14, 64, 4)                          # DRUNet head
_w3(1, 12, 12, 72, 72, gpu_only_classes=_SLOW)        # 9 tiles, the last row and column 8 wide
_w3(3, 1, 1, 16, 16)                          # smallest images
_w3(1, 2, 330, 32, 32, 2)                     # a chunk inside one long row
_w3(1, 40, 2, 16, 16)                         # wp = 4: one chunk spans 32 rows, the three staged row segments overlap
_w3(70, 4, 6, 16, 64, 6, gpu_only_classes=_SLOW)      # many tiny images; slice boundaries inside frames
_w3(1, 254, 254, 16, 16, 128, gpu_only=True)  # np = 65536: the slice count saturates at np / 512 = 128, 128 pixels per wave


def _w2(B, H, W, M, N, up, slices=0, **kw):
    _add(id=f"w2-{'up' if up else 'down'}-{B}x{H}x{W}-m{M}n{N}", kind="wgrad2", B=B, H=H, W=W, M=M, N=N, up=up, slices=slices, **kw)


for _up in (False, True):
    _w2(1, 1, 1, 16, 16, _up)
    _w2(2, 30, 30, 16, 16, _up, 4)
    _w2(2, 6, 8, 64, 16, _up)
_w2(3, 1, 5, 17, 16, True)
_w2(2, 30, 29, 24, 40, True, 4)
_w2(1, 94, 90, 16, 8, False, 17)              # 17 slices, empty last slice
_w2(1, 5, 4, 32, 128, True)
_w2(1, 94, 90, 64, 64, False, 17, gpu_only=True)
_w2(1, 94, 90, 64, 64, True, 17, gpu_only=True)


def _w222(B, D, H, W, M, N, up, slices=0):
    _add(id=f"w222-{'up' if up else 'down'}-{B}x{D}x{H}x{W}-m{M}n{N}", kind="wgrad2x2x2", B=B, D=D, H=H, W=W, M=M, N=N, up=up,
         slices=slices)


for _up in (False, True):
    _w222(2, 1, 3, 5, 16, 16, _up)            # D = 1 on the half grid: the smallest legal dep_s = 3
    _w222(1, 3, 14, 14, 40, 24, _up)
    _w222(1, 4, 30, 30, 16, 16, _up, 12)      # more than one slice


def _w333(B, D, H, W, M, N, slices=0, **kw):
    _add(id=f"w333-{B}x{D}x{H}x{W}-m{M}n{N}", kind="wgrad3x3x3", B=B, D=D, H=H, W=W, M=M, N=N, slices=slices, **kw)


_w333(2, 1, 5, 7, 16, 3)                      # D = 1: the outer depth taps must be exactly zero
_w333(2, 3, 6, 16, 16, 16)                    # thin
_w333(1, 2, 9, 10, 24, 40, gpu_only_classes=_SLOW)
_w333(1, 3, 14, 12, 16, 16, 2)                # np = 1280: each depth tap reduces several slices


def _bias(B, H, W, c, slices=0, **kw):
    _add(id=f"bias-{B}x{H}x{W}-c{c}", kind="bias", B=B, H=H, W=W, M=c, slices=slices, **kw)


_bias(1, 1, 1, 8, 1)
_bias(2, 9, 13, 5, 1)
_bias(1, 94, 90, 5, 2)
_bias(3, 94, 90, 264, 4, gpu_only_classes=("int+acc",))      # second block of the reduce grid; c not a multiple of 256

_add(id="relu-4", kind="relu", M=4)
_add(id="relu-4004", kind="relu", M=1000 * 4 + 4)
_add(id="relu-8388620", kind="relu", M=8192 * 256 * 4 + 12, gpu_only=True)       # the grid-stride second pass
_add(id="gate-split2d", kind="gate", B=2, H=9, W=14, M=64, N=16)                # conv3x3_split(..., gate=True)
_add(id="gate-thin3d", kind="gate", B=1, D=2, H=5, W=7, M=16, N=16)             # thin conv3x3x3(..., gate=True)


def _d3(B, H, W, wshape, mode, fp32, branch, wname="w"):
    _add(id=f"d3-{branch}-{B}x{H}x{W}-w{wshape[0]}x{wshape[1]}-{mode}", kind="dgrad3", B=B, H=H, W=W, M=wshape[0], N=wshape[1], mode=mode,
         fp32=fp32, branch=branch, wname=wname)


# 2-D 3x3 data gradients: w [Cout, Cin] of the forward layer, non-square so that a missing transpose cannot cancel
_d3(2, 9, 14, (64, 32), "plain", False, "split")
_d3(1, 17, 33, (128, 64), "res", False, "split")
_d3(2, 9, 14, (40, 24), "gate", False, "split")
_d3(1, 5, 36, (128, 64), "gate", False, "split")
_d3(2, 9, 14, (64, 3), "plain", False, "direct", "m_head.weight")
_d3(2, 9, 21, (2, 64), "res", False, "direct", "m_tail.weight")
_d3(1, 7, 5, (2, 64), "gate", False, "direct", "m_tail.weight")
_d3(2, 9, 14, (64, 64), "gate", True, "direct")
_d3(1, 12, 8, (64, 64), "res", True, "direct")


def _d2(B, H, W, wshape, up, fp32, branch):
    _add(id=f"d2-{'up' if up else 'down'}-{branch}-{B}x{H}x{W}-w{wshape[0]}x{wshape[1]}", kind="dgrad2", B=B, H=H, W=W, M=wshape[0],
         N=wshape[1], up=up, fp32=fp32, branch=branch)


# 2-D stride-2 data gradients on the half grid B x H x W: Ops2d.up with a down filter [Cout, Cin, 2, 2], Ops2d.down with an up filter
_d2(2, 5, 6, (64, 128), True, False, "bf16s")
_d2(1, 4, 9, (128, 64), False, False, "bf16s")
_d2(2, 5, 6, (24, 64), True, False, "fp32")           # cin % 16 != 0
_d2(1, 4, 9, (64, 24), False, False, "fp32")
_d2(1, 7, 4, (64, 128), True, True, "fp32")
_d2(1, 7, 4, (128, 64), False, True, "fp32")


def _d3d(level, wshape, mode, fp32, branch):
    _add(id=f"d3d-{branch}-l{level}-w{wshape[0]}x{wshape[1]}-{mode}", kind="dgrad3d", B=2, D=level, M=wshape[0], N=wshape[1], mode=mode,
         fp32=fp32, branch=branch)


# 3-D 3x3x3 data gradients through Ops3d.conv3(flip=True) at level `D` of a [2, c, 8, 8, 16] problem (level 1: 4 x 4 x 8, level 2: 2 x 2 x 4)
_d3d(1, (64, 32), "plain", False, "split")
_d3d(2, (64, 32), "res", False, "split")
_d3d(1, (16, 16), "gate", False, "thin")
_d3d(1, (16, 3), "gate", False, "thin")
_d3d(2, (16, 16), "plain", False, "thin")
_d3d(1, (40, 24), "gate", True, "fp32")               # the wide fp32 kernel, then relu_backward over whole buffers
for _lv, _up in ((2, True), (2, False), (1, True), (1, False)):        # level 2 -> 3: D = 1 on the half grid; level 1 -> 2: D = 2
    _add(id=f"ds3d-{'up' if _up else 'down'}-l{_lv}", kind="dstride3d", B=2, D=_lv, M=32, N=16, up=_up, branch="bf16s")

assert len({c.id for c in CASES}) == len(CASES)
for _c in CASES:
    if _c.slices:
        _np = padded(_c.B * (_c.D + 2 if _c.D else 1), _c.H, _c.W)[3]
        _got = bias_slices(_np) if _c.kind == "bias" else part_count(_np, _c.M, _c.N)
        assert _got == _c.slices, (_c.id, _got)
# what the 17-slice cases are in the table for: the last workgroup's slice starts past the last pixel
assert 16 * 4 * per_wave(8832, 17) >= 8832 and per_wave(8832, 17) == 144


def items(emu):
    """(case, class) pairs of one run of the table"""
    out = []
    for c in CASES:
        if emu and c.gpu_only:
            continue
        out += [(c, k) for k in c.classes() if not (emu and k in c.gpu_only_classes)]
    return out


def item_id(v):
    return v.id if isinstance(v, Case) else str(v)


# ------------------------------------------------------------------ data
def _gen(case, cls):
    return torch.Generator().manual_seed(zlib.crc32(f"{case.id}/{cls}".encode()))


def _small(shape, gen):
    return torch.randint(-2, 3, shape, generator=gen).float()


def _wide(shape, gen):
    return torch.randint(-4095, 4096, shape, generator=gen).float() / 1024


def operands(case, cls, shape_s, shape_l):
    """the two operands of a case in one class: (S-like, L-like); wide-s / wide-l say which one carries the 12-bit values"""
    gen = _gen(case, cls)
    if cls in ("int", "int+acc"):
        return _small(shape_s, gen), _small(shape_l, gen)
    if cls == "wide-s":
        return _wide(shape_s, gen), _small(shape_l, gen)
    if cls == "wide-l":
        return _small(shape_s, gen), _wide(shape_l, gen)
    return torch.randn(shape_s, generator=gen), torch.randn(shape_l, generator=gen)


SPECIALS = [0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -126, -(2.0 ** -126), float("inf"), float("-inf"), float("nan"), 1.0, -1.0]


def special_act(n, gen):
    """activations with every value class a ReLU mask can meet: +-0, +- the smallest denormal, the smallest normal, +-Inf, NaN"""
    a = torch.randn(n, generator=gen)
    sp = torch.tensor(SPECIALS)
    k = min(n, 4 * len(SPECIALS))
    pos = torch.randperm(n, generator=gen)[:k]
    a[pos] = sp.repeat(4)[:k]
    return a


# ------------------------------------------------------------------ activation buffers on the host
def _slack_fill(a, lo, hi, kind):
    """fill pixels [lo, hi) of every channel block of buffer a [C/8, cs, 8]"""
    if hi <= lo or kind is None:
        return
    if kind == "nan":
        a[:, lo:hi] = float("nan")
    else:                                             # +-1e30, alternating
        sign = 1 - 2 * (torch.arange(hi - lo) % 2).float()
        a[:, lo:hi] = (1e30 * sign)[None, :, None]


def to_buf(g, imgs, slack=None, guard=0):
    """[n, C, H, W] images -> activation buffer [ceil(C/8), g.cs, 8] (zero frame, zero padding channels); `slack`: what everything
    outside [sl, sl + np) holds (None: zeros, "nan", "big": +-1e30); guard: pixels in front of the buffer proper (drunet3d.Level:
    one plane, which stays zero like the plane behind)"""
    n, C, H, W = imgs.shape
    cb = (C + 7) // 8
    a = torch.zeros(cb, g.cs, 8)
    _slack_fill(a, guard, guard + g.sl, slack)
    _slack_fill(a, guard + g.sl + g.np, g.cs - guard, slack)
    t = torch.zeros(n, cb * 8, H, W)
    t[:, :C] = imgs
    av = a[:, guard + g.sl:guard + g.sl + g.np].view(cb, n, g.hp, g.wp, 8)
    av[:, :, 1:H + 1, 1:W + 1] = t.view(n, cb, 8, H, W).permute(1, 0, 3, 4, 2)
    return a


def from_buf(g, a, guard=0):
    """interior of an activation buffer -> [n, 8 * blocks, H, W]"""
    cb, n, H, W = a.shape[0], g.batch, g.height, g.width
    av = a[:, guard + g.sl:guard + g.sl + g.np].view(cb, n, g.hp, g.wp, 8)
    return av[:, :, 1:H + 1, 1:W + 1].permute(1, 0, 4, 2, 3).reshape(n, cb * 8, H, W)


def outside_interior_is_zero(g, a, guard=0, depth=0):
    """frame, slack, guard planes (and, for volumes of `depth` slices, the zero end slices) of a result hold exact zeros"""
    a = a.clone()
    cb, n, H, W = a.shape[0], g.batch, g.height, g.width
    av = a[:, guard + g.sl:guard + g.sl + g.np].view(cb, n, g.hp, g.wp, 8)
    if depth:
        av.view(cb, n // (depth + 2), depth + 2, g.hp, g.wp, 8)[:, :, 1:-1, 1:H + 1, 1:W + 1] = 0
    else:
        av[:, :, 1:H + 1, 1:W + 1] = 0
    return int(torch.count_nonzero(a)) == 0 and not bool(torch.isnan(a).any())


def vol_imgs(t):
    """[B, C, D, H, W] -> [B (D + 2), C, H, W] with zero end slices"""
    B, C, D, H, W = t.shape
    return F.pad(t.permute(0, 2, 1, 3, 4), (0, 0, 0, 0, 0, 0, 1, 1)).reshape(B * (D + 2), C, H, W).contiguous()


def imgs_vol(t, B):
    """[B (D + 2), C, H, W] -> [B, C, D, H, W] and the end slices"""
    n, C, H, W = t.shape
    v = t.view(B, n // B, C, H, W)
    return v[:, 1:-1].permute(0, 2, 1, 3, 4), v[:, (0, -1)]


# ------------------------------------------------------------------ the backend
class Backend:
    """the product's ctypes layer (deepinv_amd.hip.drunet) over one library: the gfx950 one with device tensors, or - inside
    emu_backend() - the host emulation with CPU tensors"""

    def __init__(self, device):
        from deepinv_amd import hip
        from deepinv_amd.hip import drunet as K

        self.hip, self.K, self.device = hip, K, torch.device(device)
        self.gpu = self.device.type == "cuda"

    def lib(self):
        return self.K._l()

    def stream(self):
        return self.K.stream_ptr(self.device)

    def dev(self, t):
        return t.contiguous().to(self.device)

    def sync(self):
        if self.gpu:
            torch.cuda.synchronize()

    def guarded(self, n, fill=None):
        g = Guarded(n, self.device)                   # starts as NaN (POISON)
        if fill is not None:
            g.t.copy_(fill.reshape(-1))
        return g


def _p(t, offset_floats=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset_floats)


# ------------------------------------------------------------------ weight gradients
def _wgrad_geometry(be, case):
    """(gs, gl, images of S per batch entry, guard pixels) of a weight-gradient case"""
    K = be.K
    if case.kind == "wgrad3":
        g = K.geom(case.B, case.H, case.W)
        return g, g, 0
    if case.kind == "wgrad2":
        return K.geom(case.B, case.H, case.W), K.geom(case.B, 2 * case.H, 2 * case.W), 0
    from deepinv_amd.models.drunet3d import Level
    if case.kind == "wgrad2x2x2":
        ls, ll = Level(case.B, case.D, case.H, case.W), Level(case.B, 2 * case.D, 2 * case.H, 2 * case.W)
        return ls.g, ll.g, (ls.guard, ll.guard)
    lv = Level(case.B, case.D, case.H, case.W)
    return lv.g, lv.g, (lv.guard, lv.guard)


def _wgrad_shapes(case):
    B, D, H, W, M, N = case.B, case.D, case.H, case.W, case.M, case.N
    if case.kind == "wgrad3":
        return (B, M, H, W), (B, N, H, W)
    if case.kind == "wgrad2":
        return (B, M, H, W), (B, N, 2 * H, 2 * W)
    if case.kind == "wgrad2x2x2":
        return (B, M, D, H, W), (B, N, 2 * D, 2 * H, 2 * W)
    return (B, M, D, H, W), (B, N, D, H, W)


@functools.lru_cache(maxsize=4)
def _wgrad_data(case, cls):
    """(S, L, fp64 reference, the same on absolute values) - computed once per (case, class), shared by the tests that need it"""
    s, l = operands(case, cls, *_wgrad_shapes(case))
    return s, l, wgrad_ref(case, s.double(), l.double()), wgrad_ref(case, s.double().abs(), l.double().abs())


def wgrad_ref(case, s, l):
    """fp64 weight gradient [M, N, *k]: dW[m][n][t] = sum_p S[m][p] L[n][map(p) + off_t]"""
    M, N = case.M, case.N
    if case.kind == "wgrad3":
        return torch.nn.grad.conv2d_weight(l, (M, N, 3, 3), s, padding=1)
    if case.kind == "wgrad3x3x3":
        return torch.nn.grad.conv3d_weight(l, (M, N, 3, 3, 3), s, padding=1)
    k = 2 if case.kind == "wgrad2" else 3
    conv, convT = (F.conv2d, F.conv_transpose2d) if k == 2 else (F.conv3d, F.conv_transpose3d)
    w = torch.zeros((M, N) + (2,) * k, dtype=torch.float64, requires_grad=True)
    if case.up:                   # y = convT(x = S, w [Cin, Cout, 2, 2(, 2)]), dL/dy = L
        (convT(s, w, stride=2) * l).sum().backward()
    else:                         # y = conv(x = L, w [Cout, Cin, 2, 2(, 2)], stride 2), dL/dy = S
        (conv(l, w, stride=2) * s).sum().backward()
    return w.grad


def _wgrad_call(be, case, gs, gl, sa, la, guards, dw, acc, ws, sub=None):
    """one library call on prepared buffers; sub = (dz,) selects the per-tap forms"""
    lib, K = be.lib(), be.K
    M, N = case.M, case.N
    gb = ctypes.byref
    if case.kind in ("wgrad3", "wgrad2"):
        taps = 9 if case.kind == "wgrad3" else 4
        rc = lib.dinv_conv_wgrad(gb(gs), gb(gl), _p(sa), M, _p(la), N, taps, _p(dw.t), acc, _p(ws.t), 4 * ws.n, be.stream())
    elif case.kind == "wgrad2x2x2":
        rc = lib.dinv_conv_wgrad_3d(gb(gs), gb(gl), _p(sa, guards[0] * 8), M, _p(la, guards[1] * 8), N, _p(dw.t), acc, _p(ws.t), 4 * ws.n,
                                    case.D, sub, be.stream())
    elif sub is None:             # the three depth taps in one call; L shifted by -1 slice (guard == plane)
        rc = lib.dinv_conv_wgrad_3x3x3(gb(gs), _p(sa, guards[0] * 8), M, _p(la, (guards[1] - gs.plane) * 8), N, int(gs.plane) * 8, _p(dw.t),
                                       acc, _p(ws.t), 4 * ws.n, be.stream())
    else:                         # one depth tap as a plain 3x3 weight gradient on the slice-shifted view
        rc = lib.dinv_conv_wgrad(gb(gs), gb(gl), _p(sa, guards[0] * 8), M, _p(la, (guards[1] + (sub - 1) * gs.plane) * 8), N, 9, _p(dw.t),
                                 acc, _p(ws.t), 4 * ws.n, be.stream())
    K.check(rc)


def run_wgrad(be, case, cls, beside=None):
    """one weight-gradient case on one data class; returns (worst |out - ref| / (gamma_n * magnitude), bits of dw).
    beside: called right before and right after the library call (the GPU test queues work on another stream there)"""
    K = be.K
    gs, gl, guards = _wgrad_geometry(be, case)
    s, l, ref, mag = _wgrad_data(case, cls)
    vol = case.kind in ("wgrad2x2x2", "wgrad3x3x3")
    sa = be.dev(to_buf(gs, vol_imgs(s) if vol else s, "nan", guards[0] if vol else 0))
    la = be.dev(to_buf(gl, vol_imgs(l) if vol else l, "big", guards[1] if vol else 0))
    M, N = case.M, case.N
    taps = 9 if case.kind in ("wgrad3", "wgrad3x3x3") else 4
    nparts = part_count(gs.np, M, N)
    ndepth = 3 if case.kind == "wgrad3x3x3" else 1
    ws_bytes = be.lib().dinv_conv_wgrad_workspace_bytes(ctypes.byref(gs), M, N, taps)
    assert ws_bytes == nparts * M * N * taps * 4, (ws_bytes, nparts)            # the restatement is the launcher's
    acc = 1 if cls in ("int+acc", "randn") else 0
    prefill = None
    if acc:
        pg = _gen(case, cls + "/prefill")
        prefill = torch.randint(-3, 4, ref.shape, generator=pg).float() if cls == "int+acc" else torch.randn(ref.shape, generator=pg)
    outs = []
    for dz in ((0, 1) if case.kind == "wgrad2x2x2" else (None,)):
        want = ref[:, :, dz] if dz is not None else ref
        pre = None if prefill is None else (prefill[:, :, dz] if dz is not None else prefill).contiguous()
        ws = be.guarded(ndepth * ws_bytes // 4)
        dw = be.guarded(want.numel(), pre)
        if beside:
            beside()
        _wgrad_call(be, case, gs, gl, sa, la, guards, dw, acc, ws, dz)
        if beside:
            beside()
        be.sync()
        assert ws.guards_intact() and dw.guards_intact(), f"{case.id}/{cls}: wrote outside the workspace or dw"
        outs.append(dw.t.cpu().view(want.shape))
    out = torch.stack(outs, 2) if case.kind == "wgrad2x2x2" else outs[0]
    assert bool(torch.isfinite(out).all()), f"{case.id}/{cls}: NaN / Inf in dw (workspace, slack or an unwritten element)"
    want = ref + prefill.double() if acc else ref
    if cls == "randn":
        bound = gamma(wgrad_chain(gs.np, M, N, acc)) * (mag + prefill.double().abs())
        err = (out.double() - want).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        assert bool((err <= bound).all()), f"{case.id}: worst |out - ref| / bound = {ratio:.3g}"
    else:
        bad = int((out.double() != want).sum())
        assert bad == 0, f"{case.id}/{cls}: {bad} of {want.numel()} elements differ from fp64, worst {float((out.double() - want).abs().max())}"
        ratio = 0.0
    bits = out.view(torch.int32).clone()
    if cls == "int":
        if case.kind == "wgrad3x3x3":         # equal to three plain 3x3 weight gradients on slice-shifted views, bit for bit
            for dz in range(3):
                ws, one = be.guarded(ws_bytes // 4), be.guarded(M * N * 9)
                _wgrad_call(be, case, gs, gl, sa, la, guards, one, 0, ws, dz)
                be.sync()
                assert torch.equal(one.t.cpu().view(M, N, 3, 3), out[:, :, dz]), f"{case.id}: depth tap {dz} differs from the per-tap call"
        if be.gpu or gs.np <= 4096:           # the wrappers training calls (torch.empty workspace) return the same bits
            if case.kind in ("wgrad3", "wgrad2"):
                got = K.conv_wgrad(gs, gl, sa, M, la, N, taps)
            elif case.kind == "wgrad2x2x2":
                got = torch.stack([K.conv_wgrad_3d(gs, gl, sa[:, guards[0]:], M, la[:, guards[1]:], N, case.D, dz) for dz in range(2)], 2)
            else:
                got = K.conv_wgrad_3x3x3(gs, sa[:, guards[0]:], M, la[:, guards[1] - gs.plane:], N, int(gs.plane) * 8)
            assert torch.equal(got.cpu(), out), f"{case.id}: the hip.drunet wrapper differs from the direct call"
    return ratio, bits


# ------------------------------------------------------------------ bias gradient
def run_bias(be, case, cls):
    K = be.K
    B, H, W, c = case.B, case.H, case.W, case.M
    g = K.geom(B, H, W)
    gy, _ = operands(case, cls, (B, c, H, W), (1,))
    a = to_buf(g, gy, "nan")
    av = a[:, g.sl:g.sl + g.np].view(a.shape[0], B, g.hp, g.wp, 8)
    inner = av[:, :, 1:H + 1, 1:W + 1].clone()
    av[:] = float("nan")                              # NaN on the whole frame
    av[:, :, 1:H + 1, 1:W + 1] = inner
    a = be.dev(a)
    ref, mag = gy.double().sum((0, 2, 3)), gy.double().abs().sum((0, 2, 3))
    ws_bytes = be.lib().dinv_bias_grad_workspace_bytes(ctypes.byref(g), c)
    ns = bias_slices(g.np)
    assert ws_bytes == ns * ((c + 7) // 8) * 8 * 4
    acc = 1 if cls in ("int+acc", "randn") else 0
    pg = _gen(case, cls + "/prefill")
    prefill = None if not acc else (torch.randint(-3, 4, (c,), generator=pg).float() if cls == "int+acc" else torch.randn(c, generator=pg))
    runs = []
    for _ in range(2):                                # two calls give equal bits
        ws, db = be.guarded(ws_bytes // 4), be.guarded(c, prefill)
        K.check(be.lib().dinv_bias_grad(ctypes.byref(g), _p(a), c, _p(db.t), acc, _p(ws.t), 4 * ws.n, be.stream()))
        be.sync()
        assert ws.guards_intact() and db.guards_intact(), f"{case.id}/{cls}: wrote outside the workspace or db"
        runs.append(db.t.cpu().clone())
    out = runs[0]
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), f"{case.id}: two calls differ"
    assert bool(torch.isfinite(out).all()), f"{case.id}/{cls}: NaN / Inf in db"
    want = ref + prefill.double() if acc else ref
    if cls == "randn":
        bound = gamma(bias_chain(g.np)) * (mag + prefill.double().abs())
        err = (out.double() - want).abs()
        ratio = float((err / bound).max())
        assert bool((err <= bound).all()), f"{case.id}: worst |out - ref| / bound = {ratio:.3g}"
        return ratio
    assert torch.equal(out.double(), want), f"{case.id}/{cls}: differs from fp64, worst {float((out.double() - want).abs().max())}"
    if cls == "int":
        assert torch.equal(K.bias_grad(g, a, c).cpu(), out), f"{case.id}: the hip.drunet wrapper differs from the direct call"
    return 0.0


# ------------------------------------------------------------------ ReLU backward and the gate epilogues
def run_relu(be, case):
    """dinv_relu_backward in place inside a guarded buffer against torch.where(act > 0, grad, 0) on the CPU, bit for bit (a positive
    denormal passes: the forward ReLU keeps it, max(x, 0) with denormals on)"""
    n = case.M
    gen = _gen(case, "special")
    act, grad = special_act(n, gen), torch.randn(n, generator=gen)
    want = torch.where(act > 0, grad, torch.zeros(()))
    gb = be.guarded(n, grad)
    be.K.relu_backward(be.dev(act), gb.t)
    be.sync()
    assert gb.guards_intact()
    got = gb.t.cpu()
    bad = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    assert bad == 0, f"{case.id}: {bad} of {n} elements differ"
    return 0.0


def run_gate(be, case):
    """the gate epilogues give the mask of relu_backward on the same activations: conv(..., gate = act) must equal the same convolution
    followed by relu_backward(act), bit for bit, with every special value in act - and both must equal act > 0 taken on the CPU"""
    K = be.K
    gen = _gen(case, "special")
    cout, cin = case.M, case.N
    if case.D:
        from deepinv_amd.models.drunet3d import Level
        lv = Level(case.B, case.D, case.H, case.W)
        g, guard = lv.g, lv.guard
        x = vol_imgs(_small((case.B, cin, case.D, case.H, case.W), gen))
        act = vol_imgs(special_act(case.B * cout * case.D * case.H * case.W, gen).view(case.B, cout, case.D, case.H, case.W))
        pk, cip, cop = K.pack_conv3x3x3_weight(_small((cout, cin, 3, 3, 3), gen))
        assert int(pk.shape[4]) == 16                 # the thin kernel
    else:
        g, guard = K.geom(case.B, case.H, case.W), 0
        x = _small((case.B, cin, case.H, case.W), gen)
        act = special_act(case.B * cout * case.H * case.W, gen).view(case.B, cout, case.H, case.W)
        pk = K.pack_split2d_weight(_small((cout, cin, 3, 3), gen))
    act_buf = to_buf(g, act, None, guard)
    xa, aa, pkd = be.dev(to_buf(g, x, None, guard)), be.dev(act_buf), be.dev(pk)

    def conv(gate):
        y = torch.zeros((cout // 8, g.cs, 8), device=be.device)
        if case.D:
            K.conv3x3x3(g, xa[:, guard:], pkd, cip, cop, y[:, guard:], case.D, cout_valid=cout, res1=aa[:, guard:] if gate else None, gate=gate)
        else:
            K.conv3x3_split(g, xa, pkd, cin, cout, y, res1=aa if gate else None, gate=gate)
        return y

    gated, plain = conv(True), conv(False)
    masked = K.relu_backward(aa, plain.clone())
    be.sync()
    gated, plain, masked = gated.cpu(), plain.cpu(), masked.cpu()
    assert bool(torch.isfinite(gated).all())
    assert torch.equal(gated, masked), f"{case.id}: the gate epilogue and relu_backward disagree on {int((gated != masked).sum())} elements"
    want = torch.where(from_buf(g, act_buf, guard) > 0, from_buf(g, plain, guard), torch.zeros(()))
    assert torch.equal(from_buf(g, gated, guard), want), f"{case.id}: the mask differs from act > 0 taken on the CPU"
    assert int((want != 0).sum()) > want.numel() // 16    # the comparison is not one of zeros (3-D: half the images are end slices)
    assert outside_interior_is_zero(g, gated, guard, case.D)
    return 0.0


# ------------------------------------------------------------------ data gradients
def _check_dgrad(case, cls, out, ref, mag, chain):
    """exact classes: bit for bit; randn: the bf16-split kernels' l2 figure, or the per-element ceiling gamma_chain * magnitude"""
    assert bool(torch.isfinite(out).all()), f"{case.id}/{cls}: NaN / Inf"
    if cls != "randn":
        bad = int((out.double() != ref).sum())
        assert bad == 0, f"{case.id}/{cls}: {bad} of {ref.numel()} elements differ from fp64, worst {float((out.double() - ref).abs().max())}"
        return 0.0
    if case.branch in ("split", "bf16s"):
        err = float((out.double() - ref).norm() / ref.norm())
        assert err < SPLIT_L2, f"{case.id}: relative l2 {err:.3g}"
        return err / SPLIT_L2
    bound = gamma(chain) * mag
    err = (out.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), f"{case.id}: worst |out - ref| / bound = {ratio:.3g}"
    return ratio


def _dgrad_extras(case, cls, shape, gen):
    """(res, act) in NC.. shape: a residual in the data class of the gradient, ReLU activations (>= 0, about half of them zero)"""
    res = act = None
    if case.mode == "res":
        res = torch.randn(shape, generator=gen) if cls == "randn" else _small(shape, gen)
    if case.mode == "gate":
        act = torch.randn(shape, generator=gen).relu()
    return res, act


def run_dgrad3(be, case, cls):
    """drunet_train._conv3(flip=True): gx = conv_transpose2d(gy, w, padding=1) (+ res) (* (act > 0))"""
    from deepinv_amd.models import drunet_train as T
    K = be.K
    gen = _gen(case, cls)
    B, H, W = case.B, case.H, case.W
    wt, gyt = operands(case, cls, (case.M, case.N, 3, 3), (B, case.M, H, W))          # wide-s: the filter, wide-l: the gradient
    if cls == "randn":
        wt = wt / (3.0 * case.M ** 0.5)
    w = be.dev(T.Ops2d.weight(case.wname, wt))        # padded as training pads it
    cin, cout = w.shape[0], w.shape[1]                # of the data-gradient convolution
    split = cout % 64 == 0 and cin % 16 == 0 and not case.fp32
    assert ("split" if split else "direct") == case.branch, case.id
    g = K.geom(B, H, W)
    gy = torch.zeros(B, cin, H, W)
    gy[:, :case.M] = gyt                              # padded channels carry zero gradients
    res, act = _dgrad_extras(case, cls, (B, cout, H, W), gen)
    ref = F.conv_transpose2d(gy.double(), w.cpu().double(), padding=1)
    mag = F.conv_transpose2d(gy.double().abs(), w.cpu().double().abs(), padding=1)
    if res is not None:
        ref, mag = ref + res.double(), mag + res.double().abs()
    if act is not None:
        ref = ref * (act > 0)
    y = T._conv3(g, w, be.dev(to_buf(g, gy)), res1=None if res is None else be.dev(to_buf(g, res)), fp32=case.fp32, flip=True,
                 gate=None if act is None else be.dev(to_buf(g, act)))
    be.sync()
    K.clear_pack_cache()
    y = y.cpu()
    assert y.shape[0] == (cout + 7) // 8
    assert outside_interior_is_zero(g, y), f"{case.id}/{cls}: the frame or the slack of the result is not zero"
    out = from_buf(g, y)
    assert float(out[:, cout:].abs().max() if out.shape[1] > cout else 0.0) == 0.0
    return _check_dgrad(case, cls, out[:, :cout], ref, mag, 9 * cin + 2)


def run_dgrad2(be, case, cls):
    """Ops2d.up with a down filter [Cout, Cin, 2, 2]: conv_transpose2d(gy, w, stride=2); Ops2d.down with an up filter [Cin, Cout, 2, 2]:
    conv2d(gy, w, stride=2) - each the data gradient of the other layer"""
    from deepinv_amd.models import drunet_train as T
    K = be.K
    B, H, W = case.B, case.H, case.W
    ops = T.Ops2d(types.SimpleNamespace(train_forward_precision="fp32"), torch.empty(B, 1, 2 * H, 2 * W), True)    # levels 0 and 1 are used
    if case.up:
        wt, gyt = operands(case, cls, (case.M, case.N, 2, 2), (B, case.M, H, W))
        cin, cout = case.M, case.N
    else:
        wt, gyt = operands(case, cls, (case.M, case.N, 2, 2), (B, case.N, 2 * H, 2 * W))
        cin, cout = case.N, case.M
    if cls == "randn":
        wt = wt / (2.0 * cin ** 0.5)
    assert ("bf16s" if cin % 16 == 0 and not case.fp32 else "fp32") == case.branch, case.id
    w = be.dev(wt)
    if case.up:
        ref = F.conv_transpose2d(gyt.double(), wt.double(), stride=2)
        mag = F.conv_transpose2d(gyt.double().abs(), wt.double().abs(), stride=2)
        y, go = ops.up(0, w, be.dev(to_buf(ops.g[1], gyt)), fp32=case.fp32), ops.g[0]
    else:
        ref = F.conv2d(gyt.double(), wt.double(), stride=2)
        mag = F.conv2d(gyt.double().abs(), wt.double().abs(), stride=2)
        y, go = ops.down(0, w, be.dev(to_buf(ops.g[0], gyt)), fp32=case.fp32), ops.g[1]
    be.sync()
    K.clear_pack_cache()
    y = y.cpu()
    assert outside_interior_is_zero(go, y), f"{case.id}/{cls}: the frame or the slack of the result is not zero"
    return _check_dgrad(case, cls, from_buf(go, y), ref, mag, 4 * cin + 2)


def _ops3d(be, fp32):
    from deepinv_amd.models import drunet3d as T3
    T3.CHECK_RECYCLED = True
    ops = T3.Ops3d(types.SimpleNamespace(train_forward_precision="fp32" if fp32 else "bf16split", conv_precision="bf16split"),
                   torch.empty(2, 1, 8, 8, 16, device=be.device), True)
    return T3, ops


def _vol(be, T3, lv, t):
    """a Vol of level lv holding [B, C, D, H, W] (zero frames, end slices, guard planes, slack and padded channel blocks)"""
    v = T3.Vol(lv, t.shape[1], be.device)
    full = torch.zeros(v.t.shape)
    buf = to_buf(lv.g, vol_imgs(t), None, lv.guard)
    full[:buf.shape[0]] = buf
    v.t.copy_(full)
    return v


def _vol_out(lv, v, channels):
    """(interior [B, channels, D, H, W] of a result Vol, whether everything else in it is exactly zero)"""
    t = v.t.cpu()
    clean = outside_interior_is_zero(lv.g, t, lv.guard, lv.D)
    vol, _ = imgs_vol(from_buf(lv.g, t, lv.guard), lv.B)
    clean = clean and float(vol[:, channels:].abs().max() if vol.shape[1] > channels else 0.0) == 0.0
    return vol[:, :channels].contiguous(), clean


def run_dgrad3d(be, case, cls):
    """Ops3d.conv3(flip=True) / Ops3d.down / Ops3d.up as training calls them, twice: the second run takes its Vol buffers from the
    free list under CHECK_RECYCLED (frames, end slices, guard planes, slack and padded blocks of every released buffer are zero) and
    must return the same bits"""
    T3, ops = _ops3d(be, case.fp32)
    try:
        gen = _gen(case, cls)
        i = case.D
        if case.kind == "dgrad3d":
            lvi = lvo = ops.lv[i]
            wt, gyt = operands(case, cls, (case.M, case.N, 3, 3, 3), (lvi.B, case.M, lvi.D, lvi.H, lvi.W))
            cin, cout = case.M, case.N
            thin = cin <= 16 and cout <= 16
            branch = "split" if cin >= 16 and cout >= 16 and not case.fp32 and not thin else ("thin" if cout <= 16 else "fp32")
            if cls == "randn":
                wt = wt / (27.0 * cin) ** 0.5
            ref = F.conv_transpose3d(gyt.double(), wt.double(), padding=1)
            mag = F.conv_transpose3d(gyt.double().abs(), wt.double().abs(), padding=1)
            chain = 27 * ((cin + 7) // 8 * 8) + 2
        else:
            lvi, lvo = (ops.lv[i + 1], ops.lv[i]) if case.up else (ops.lv[i], ops.lv[i + 1])
            cin, cout = (case.M, case.N) if case.up else (case.N, case.M)
            wt, gyt = operands(case, cls, (case.M, case.N, 2, 2, 2), (lvi.B, cin, lvi.D, lvi.H, lvi.W))
            branch = "bf16s"
            if cls == "randn":
                wt = wt / (8.0 * cin) ** 0.5
            op = F.conv_transpose3d if case.up else F.conv3d
            ref, mag = op(gyt.double(), wt.double(), stride=2), op(gyt.double().abs(), wt.double().abs(), stride=2)
            chain = 8 * cin + 2
        assert branch == case.branch, (case.id, branch)
        res, act = _dgrad_extras(case, cls, tuple(ref.shape), gen)
        if res is not None:
            ref, mag = ref + res.double(), mag + res.double().abs()
        if act is not None:
            ref = ref * (act > 0)
        w = be.dev(wt)
        runs = []
        for rnd in range(2):
            if rnd:
                assert any(T3._POOL.values()), f"{case.id}: nothing was released to the free list"
            x = _vol(be, T3, lvi, gyt)
            if case.kind == "dgrad3d":
                y = ops.conv3(i, w, x, res=None if res is None else _vol(be, T3, lvo, res), fp32=case.fp32, flip=True,
                              gate=None if act is None else _vol(be, T3, lvo, act))
            else:
                y = ops.up(i, w, x) if case.up else ops.down(i, w, x)
            be.sync()
            out, clean = _vol_out(lvo, y, cout)
            assert clean, f"{case.id}/{cls}: frames, end slices, guard planes, slack or padded channels of the result are not zero"
            runs.append(out)
            del x, y
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), f"{case.id}: the run on recycled buffers differs"
        return _check_dgrad(case, cls, runs[0], ref, mag, chain)
    finally:
        be.K.clear_pack_cache()
        T3.release_buffers()
        T3.CHECK_RECYCLED = False


RUNNERS = {"wgrad3": lambda be, c, k: run_wgrad(be, c, k)[0], "wgrad2": lambda be, c, k: run_wgrad(be, c, k)[0],
           "wgrad2x2x2": lambda be, c, k: run_wgrad(be, c, k)[0], "wgrad3x3x3": lambda be, c, k: run_wgrad(be, c, k)[0],
           "bias": run_bias, "relu": lambda be, c, k: run_relu(be, c), "gate": lambda be, c, k: run_gate(be, c),
           "dgrad3": run_dgrad3, "dgrad2": run_dgrad2, "dgrad3d": run_dgrad3d, "dstride3d": run_dgrad3d}


def run_case(be, case, cls):
    """run one (case, class); returns the measured worst fraction of the randn ceiling (0 for the exact classes) and prints it"""
    ratio = RUNNERS[case.kind](be, case, cls)
    print(f"{case.id}/{cls}: " + (f"worst / bound = {ratio:.3g}" if cls == "randn" else "exact"))
    return ratio
