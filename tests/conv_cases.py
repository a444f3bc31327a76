"""Shared by tests/test_conv_gpu.py (the gfx950 library) and tests/test_emu_conv.py (the same kernel sources on the host emulation):
one table of spatial-convolution cases, each meant to reach one dispatch path of csrc/blur.hip (make_geom, make_tile / launch_tiled,
launch_strided, the generic kernels, make_geom3) at one of its edges, the fp64 references, a restatement of the dispatch rules
(expected_kernel), and the runner that calls the C entry points (dinv_conv2d, dinv_conv2d_transpose, dinv_conv2d_filter_grad and
the three dinv_conv3d*) on guarded buffers (fft_cases.Guarded).

Every case runs the forward, the transpose and the filter gradient and checks, per element, against fp64:
    |y - ref| <= BOUNDS[kernel] * (|k| * |x|)
where (|k| * |x|) is the same operator applied to the absolute values (for the transpose its adjoint applied to |k| and |v|, for
the filter gradient the filter gradient of |x| and |v|).  A dropped tap, a wrong tap or a bad value on one tile edge is an O(1 / taps)
error against that measure, not a 1e-7 one; an output with zero measure (a pixel no tap reaches) must be exactly zero."""
import ctypes
from dataclasses import dataclass

import torch

from fft_cases import POISON, Guarded

from deepinv_amd.hip.conv import Conv3dDesc, ConvDesc

MODES = {"valid": 0, "circular": 1, "reflect": 2, "replicate": 3, "constant": 4}
LDS_MAX = 64 * 1024               # bytes of dynamic LDS a launcher admits
MAX_PLANES = 65535                # kMaxGridZ: planes per launch


# ------------------------------------------------------------------ fp64 references (deepinv's conv2d / conv3d)
def _ref_conv(x, k, mode, stride):
    """true convolution (flipped filter) of the padded image, deepinv's `conv2d` (convolution.py:42-107), then [::s, ::s]"""
    B, C, H, W = x.shape
    fh, fw = k.shape[-2:]
    x, k = x.double(), k.double().expand(-1, C, -1, -1) if k.shape[1] != C else k.double()
    if mode != "valid":
        pad = ((fw - 1) // 2, fw // 2, (fh - 1) // 2, fh // 2)     # deepinv pads (h - 1) // 2 above, h // 2 below
        x = torch.nn.functional.pad(x, pad, mode=mode if mode != "constant" else "constant", value=0)
    out = []
    for b in range(B):
        kb = k[b if k.shape[0] > 1 else 0]
        out.append(torch.nn.functional.conv2d(x[b:b + 1], torch.flip(kb, (-2, -1))[:, None], groups=C))
    y = torch.cat(out, 0)
    return y[:, :, ::stride, ::stride]


def _ref_conv3(x, k, mode):
    """true 3-D convolution of the padded volume, deepinv's conv3d (convolution.py:333-393)"""
    B, C = x.shape[:2]
    fd, fh, fw = k.shape[-3:]
    if mode != "valid":
        pad = ((fw - 1) // 2, fw // 2, (fh - 1) // 2, fh // 2, (fd - 1) // 2, fd // 2)
        x = torch.nn.functional.pad(x, pad, mode=mode if mode != "constant" else "constant", value=0)
    k = k.expand(B, C, fd, fh, fw)
    out = torch.nn.functional.conv3d(x.reshape(1, B * C, *x.shape[2:]), torch.flip(k, (-3, -2, -1)).reshape(B * C, 1, fd, fh, fw), groups=B * C)
    return out.reshape(B, C, *out.shape[2:])


# ------------------------------------------------------------------ error bounds (max over elements of |out - ref| / (|k| * |x|))
# Measured on the host emulation of the kernel sources (`python -m pytest tests/test_emu_conv.py -s` prints every case's worst
# element per operation): the worst of each kernel over its emulated cases, and the bound at about 4x that.
BOUNDS = {
    "conv2d_tiled_kernel": 1.2e-6,                      # worst 2.9e-7 (tiled-fwd-valid-130x70-k31x31-b2c1, forward)
    "conv2d_pad_kernel": 9e-7,                          # worst 2.2e-7 (generic-adj-valid-30x200-k12x128, forward)
    "conv2d_pad_transpose_kernel": 1e-6,                # worst 2.6e-7 (generic-fwd-circular-60x64-k53x53, transpose)
    "conv2d_strided_kernel<true>": 2.6e-7,              # worst 6.4e-8 (strided-fast4-fwd-reflect-67x90-k8x8-s4-b2c1): 4 partial sums
    "conv2d_strided_kernel<false>": 7e-7,               # worst 1.7e-7 (strided-fwd-circular-45x70-k7x9-s3)
    "conv2d_strided_transpose_kernel<true>": 5.2e-7,    # worst 1.3e-7 (strided-fast16-adj-valid-130x75-k16x16-s4-b2c1)
    "conv2d_strided_transpose_kernel<false>": 7e-7,     # worst 1.7e-7 (strided-adj-constant-64x70-k7x7-s2-b2c3-perc)
    "conv2d_filter_grad_kernel": 4e-7,                  # worst 9.5e-8 (strided-generic-adj-reflect-40x70-k3x5-s17)
    "conv3d_pad_kernel": 9e-7,                          # worst 2.3e-7 (vol-reflect-2x2x6x9x11-k3x3x3)
    "conv3d_pad_transpose_kernel": 7e-7,                # worst 1.8e-7 (vol-reflect-1x1x4x9x70-k2x3x4)
    "conv3d_filter_grad_kernel": 4e-7,                  # worst 2.7e-8 (vol-valid-2x1x5x12x9-k3x5x2-perb); the structure and bound of the
                                                        # 2-D kernel: sums of 4 terms on 2 x 2 planes reach 1.4e-7 on the device
}


# ------------------------------------------------------------------ the dispatch rules of csrc/blur.hip, restated
@dataclass(frozen=True)
class Conv2:
    B: int
    C: int
    H: int
    W: int
    fb: int
    fc: int
    fh: int
    fw: int
    mode: str
    stride: int = 1

    def desc(self):
        return ConvDesc(self.B, self.C, self.H, self.W, self.fb, self.fc, self.fh, self.fw, MODES.get(self.mode, self.mode), self.stride)


@dataclass(frozen=True)
class Conv3:
    B: int
    C: int
    D: int
    H: int
    W: int
    fb: int
    fc: int
    fd: int
    fh: int
    fw: int
    mode: str

    def desc(self):
        return Conv3dDesc(self.B, self.C, self.D, self.H, self.W, self.fb, self.fc, self.fd, self.fh, self.fw, MODES.get(self.mode, self.mode), 0)


def out_size(n, f, mode, s=1):
    """output extent of one axis (make_geom): valid n - f + 1, else n; then ceil(. / s)"""
    full = n - f + 1 if mode == "valid" else n
    return -(-full // s)


def rejection(d):
    """the make_geom / make_geom3 check a descriptor fails (None when it is accepted)"""
    is3 = isinstance(d, Conv3)
    sp = (d.D, d.H, d.W) if is3 else (d.H, d.W)
    fs = (d.fd, d.fh, d.fw) if is3 else (d.fh, d.fw)
    if d.B < 0 or d.C < 1 or min(sp) < 1:
        return "geometry"
    if min(fs) < 1 or d.fb not in (1, d.B) or d.fc not in (1, d.C):
        return "filter shape not broadcastable"
    if d.mode not in MODES:
        return "unknown padding mode"
    if not is3 and d.stride < 1:
        return "bad stride"
    if d.mode == "valid" and any(f > n for f, n in zip(fs, sp)):
        return "filter larger than"
    if d.mode == "circular" and any(f // 2 > n for f, n in zip(fs, sp)):
        return "circular padding wider than"
    if d.mode == "reflect" and any(f // 2 >= n for f, n in zip(fs, sp)):
        return "reflect padding must be smaller"
    if not is3 and d.B * d.C > MAX_PLANES:
        return "too many (batch*channel) planes"
    taps = 1
    for f in fs:
        taps *= f
    if taps * 4 > LDS_MAX:
        return "filter too large for LDS"
    return None


def tiled_lds(h, w):
    """make_tile: filter table of h + 6 rows of w4, patch of 64 + h - 1 rows of pitch 64 + w4"""
    w4 = (w + 3) & ~3
    return ((h + 6) * w4 + (64 + h - 1) * (64 + w4)) * 4


def strided_lds(h, w, s, transpose):
    """launch_strided: LDS bytes of the forward (PH x pitch patch) / transposed (PH x (PWs | 1) measurements) tiled kernel"""
    if not transpose:
        ph, pws = 15 * s + h, 15 + (w + s - 1) // s
        pitch = s * pws
        if s == 4 and w % 4 == 0:
            pitch = (pitch + 3) & ~3
        else:
            while pitch % 8 != 4:
                pitch += 1
        return (h * w + ph * pitch) * 4
    ph, pws = 63 // s + (h - 1) // s + 2, 63 // s + (w - 1) // s + 2
    return (h * w + ph * (pws | 1)) * 4


def expected_kernel(d, transpose):
    """the kernel dinv_conv2d (transpose = False) / dinv_conv2d_transpose (True) launches for Conv2 `d`; None: rejected"""
    if rejection(d):
        return None
    s, m = d.stride, d.mode
    if s == 1 and (not transpose or m in ("valid", "circular", "constant")) and tiled_lds(d.fh, d.fw) <= LDS_MAX:
        return "conv2d_tiled_kernel"
    if 2 <= s <= 16:
        if not transpose:
            if strided_lds(d.fh, d.fw, s, False) <= LDS_MAX:
                return "conv2d_strided_kernel<true>" if s == 4 and d.fw % 4 == 0 else "conv2d_strided_kernel<false>"
        elif (m in ("valid", "constant") or (m == "circular" and d.H % s == 0 and d.W % s == 0)) and \
                strided_lds(d.fh, d.fw, s, True) <= LDS_MAX:
            return "conv2d_strided_transpose_kernel<true>" if (s, d.fh, d.fw) == (4, 16, 16) else \
                "conv2d_strided_transpose_kernel<false>"
    return "conv2d_pad_transpose_kernel" if transpose else "conv2d_pad_kernel"


def expected_launches3(d, op):
    """the launches of dinv_conv3d (op "fwd"), dinv_conv3d_transpose ("adj") and dinv_conv3d_filter_grad ("fgrad"): grids are
    cut at 65535 planes of (batch, channel, depth) - of (batch, channel) for the filter gradient"""
    if rejection(d):
        return []
    name = {"fwd": "conv3d_pad_kernel", "adj": "conv3d_pad_transpose_kernel", "fgrad": "conv3d_filter_grad_kernel"}[op]
    planes = d.B * d.C * {"fwd": out_size(d.D, d.fd, d.mode), "adj": d.D, "fgrad": 1}[op]
    return [name] * (-(-planes // MAX_PLANES))


SHORT = {"conv2d_tiled_kernel": "tiled", "conv2d_pad_kernel": "generic", "conv2d_pad_transpose_kernel": "generic",
         "conv2d_strided_kernel<true>": "strided-fast4", "conv2d_strided_kernel<false>": "strided",
         "conv2d_strided_transpose_kernel<true>": "strided-fast16", "conv2d_strided_transpose_kernel<false>": "strided"}


# ------------------------------------------------------------------ the case table
@dataclass
class Case:
    id: str
    conv: object                # Conv2 | Conv3
    emu: bool                   # small enough for the host emulation
    kernels: dict               # op -> the kernel(s) the launcher must reach ("fwd", "adj", "fgrad"); {} for a rejection

    @property
    def rejected(self):
        return not self.kernels


def _c2(cases, op, mode, H, W, fh, fw, s=1, B=1, C=1, fb=1, fc=1, emu=True, tag=""):
    d = Conv2(B, C, H, W, fb, fc, fh, fw, mode, s)
    kf, ka = expected_kernel(d, False), expected_kernel(d, True)
    assert kf and ka, d
    path = SHORT[ka if op == "adj" else kf]
    if path == "generic" and s > 1:
        path = "strided-generic"
    cid = f"{path}-{op}-{mode}-{H}x{W}-k{fh}x{fw}" + (f"-s{s}" if s > 1 else "") + (f"-b{B}c{C}" if (B, C) != (1, 1) else "")
    cid += ("-perb" if fb > 1 else "") + ("-perc" if fc > 1 else "") + tag
    cases.append(Case(cid, d, emu, {"fwd": [kf], "adj": [ka], "fgrad": ["conv2d_filter_grad_kernel"]}))


def _c3(cases, mode, B, C, D, H, W, fb, fc, fd, fh, fw, emu=True, tag=""):
    d = Conv3(B, C, D, H, W, fb, fc, fd, fh, fw, mode)
    assert rejection(d) is None, d
    cid = f"vol-{mode}-{B}x{C}x{D}x{H}x{W}-k{fd}x{fh}x{fw}" + ("-perb" if fb > 1 else "") + ("-perc" if fc > 1 else "") + tag
    cases.append(Case(cid, d, emu, {op: expected_launches3(d, op) for op in ("fwd", "adj", "fgrad")}))


def _reject(cases, d, tag):
    assert rejection(d) is not None, d
    cases.append(Case(f"reject-{'vol-' if isinstance(d, Conv3) else ''}{tag}", d, True, {}))


ALL = ("valid", "circular", "reflect", "replicate", "constant")
GATHER = ("valid", "circular", "constant")          # the modes whose transpose is again a tiled gather


def build_cases():
    cases = []
    # ---- conv2d_tiled_kernel (stride 1)
    # several 64 x 64 tiles in both directions, ragged edges, every padding mode (reflect / replicate transposes: the generic kernel)
    for mode in ALL:
        _c2(cases, "fwd", mode, 130, 70, 31, 31, B=2 if mode == "valid" else 1)
    for mode in GATHER:
        _c2(cases, "adj", mode, 200, 70, 9, 9)
    # filter widths 0..3 (mod 4): every NV and `rem` branch, w = 1 (nfull = 0); heights 1..3 (the short branch) and >= 4; the
    # output is 70 x 66 (2 x 2 tiles, Wo % 4 = 2: the scalar store) in every mode
    hw = [(1, 1), (1, 9), (9, 1), (2, 2), (2, 7), (3, 3), (3, 6), (4, 4), (4, 8), (5, 5), (6, 10), (7, 11), (8, 12), (12, 13)]
    for i, (h, w) in enumerate(hw):
        mode = ALL[i % 5]
        H, W = (70 + h - 1, 66 + w - 1) if mode == "valid" else (70, 66)
        _c2(cases, "fwd" if i % 2 == 0 else "adj", mode, H, W, h, w, B=1 + i % 2)
    # output widths 0 (mod 4) - the 16-byte store - and 1, 2, 3 - the scalar one, at the right edge of a tile
    _c2(cases, "fwd", "circular", 68, 128, 5, 5)
    _c2(cases, "adj", "valid", 68, 131, 7, 4)
    for wo in (1, 2, 3):
        _c2(cases, "fwd", "valid", 10, 10, 3, 11 - wo, tag=f"-wo{wo}")
        _c2(cases, "adj", "constant", 67, 64 + wo, 4, 3, tag=f"-wo{64 + wo}")
    # the largest filters that fit: 52 x 52 square (65424 B of LDS), 41 x 64
    _c2(cases, "fwd", "circular", 60, 70, 52, 52)
    _c2(cases, "adj", "valid", 130, 70, 52, 52)
    _c2(cases, "fwd", "constant", 50, 80, 41, 64)
    # filters larger than the image (circular at ph = H, reflect at ph = H - 1)
    _c2(cases, "fwd", "circular", 9, 11, 15, 17)
    _c2(cases, "adj", "circular", 7, 11, 15, 17, tag="-ph-eq-h")
    _c2(cases, "fwd", "replicate", 5, 6, 13, 9)
    _c2(cases, "adj", "constant", 5, 6, 13, 9)
    _c2(cases, "fwd", "reflect", 8, 9, 15, 17, tag="-ph-eq-h-1")
    # broadcasts: a filter per sample, per channel, per plane
    _c2(cases, "fwd", "reflect", 40, 50, 5, 7, B=3, C=2, fb=3)
    _c2(cases, "adj", "circular", 40, 50, 6, 6, B=3, C=2, fc=2)
    _c2(cases, "adj", "constant", 70, 65, 3, 8, B=2, C=3, fb=2, fc=3)
    # large images (device only): bench.py's Blur shapes (9 x 9 at 256^2), 512^2 and 1024 x 96
    _c2(cases, "adj", "circular", 256, 256, 9, 9, B=4, C=3, emu=False)
    _c2(cases, "fwd", "valid", 256, 256, 9, 9, B=4, C=3, emu=False)
    _c2(cases, "fwd", "circular", 512, 512, 9, 9, B=2, C=3, emu=False)
    _c2(cases, "adj", "valid", 520, 520, 9, 9, B=2, C=3, emu=False)
    _c2(cases, "fwd", "reflect", 1024, 96, 31, 31, emu=False)
    _c2(cases, "adj", "constant", 1024, 96, 31, 31, emu=False)
    # ---- generic stride-1 kernels: past the tiled LDS limit (53 x 53, w = 64 with h = 42, w = 128 with h = 12)
    _c2(cases, "fwd", "circular", 60, 64, 53, 53)
    _c2(cases, "adj", "constant", 70, 90, 53, 53, emu=False)
    _c2(cases, "fwd", "valid", 80, 70, 53, 53, emu=False)
    _c2(cases, "fwd", "replicate", 60, 100, 42, 64)
    _c2(cases, "fwd", "reflect", 20, 140, 12, 128)
    _c2(cases, "adj", "valid", 30, 200, 12, 128)
    # reflect / replicate transposes: several 64-column blocks, H not a multiple of 4
    _c2(cases, "adj", "reflect", 67, 150, 5, 7)
    _c2(cases, "adj", "replicate", 67, 150, 6, 4)
    _c2(cases, "adj", "reflect", 131, 70, 8, 8, B=2)
    _c2(cases, "adj", "reflect", 8, 9, 15, 17, tag="-ph-eq-h-1")
    # ---- strided forward: FAST4 (stride 4, w % 4 = 0), <false> at strides 2, 3, 4, 5 and 8 (4 x 4: 65536 B, exactly the limit)
    _c2(cases, "fwd", "circular", 72, 80, 16, 16, s=4)
    _c2(cases, "fwd", "reflect", 67, 90, 8, 8, s=4, B=2)
    _c2(cases, "fwd", "valid", 70, 75, 5, 12, s=4)
    _c2(cases, "fwd", "replicate", 70, 66, 6, 6, s=2)
    _c2(cases, "fwd", "circular", 45, 70, 7, 9, s=3)
    _c2(cases, "fwd", "valid", 66, 70, 7, 9, s=4)
    _c2(cases, "fwd", "constant", 83, 97, 11, 10, s=5)
    _c2(cases, "fwd", "reflect", 70, 140, 4, 4, s=8)
    # past the strided LDS limit: the generic kernel (stride 8 with 5 x 5; strides 12 and 16 never fit; 17 is above the range)
    _c2(cases, "fwd", "circular", 70, 140, 5, 5, s=8)
    _c2(cases, "fwd", "reflect", 50, 70, 6, 6, s=12)
    _c2(cases, "fwd", "valid", 80, 90, 16, 16, s=16)
    _c2(cases, "fwd", "constant", 40, 70, 3, 5, s=17)
    # ---- strided transpose: FAST16 (16 x 16 at stride 4), <false> at strides 2 .. 16
    _c2(cases, "adj", "circular", 64, 72, 16, 16, s=4)
    _c2(cases, "adj", "valid", 130, 75, 16, 16, s=4, B=2)
    _c2(cases, "adj", "constant", 70, 66, 16, 16, s=4)
    for s in range(2, 17):
        mode = GATHER[s % 3]
        h, w = s + 1 + s % 3, 2 * s - 1
        if mode == "circular":
            H, W = s * -(-70 // s), s * -(-66 // s)
        else:
            H, W = 70 + s % 5, 66 + s
        _c2(cases, "adj", mode, H, W, h, w, s=s)
    # circular with sizes the stride does not divide, reflect / replicate: the generic transpose (smagic division)
    _c2(cases, "adj", "circular", 66, 70, 8, 8, s=4)
    _c2(cases, "adj", "circular", 70, 72, 5, 5, s=3)
    _c2(cases, "adj", "reflect", 45, 70, 7, 9, s=3)
    _c2(cases, "adj", "replicate", 70, 67, 6, 6, s=2)
    _c2(cases, "adj", "reflect", 40, 70, 3, 5, s=17)
    # images smaller than the stride
    _c2(cases, "fwd", "constant", 5, 7, 3, 3, s=8)
    _c2(cases, "adj", "valid", 5, 7, 2, 2, s=8)
    _c2(cases, "adj", "circular", 6, 6, 3, 3, s=8)
    # broadcasts on the strided kernels, and config 5's shape (bicubic x4, circular, 256^2) on the device
    _c2(cases, "fwd", "circular", 64, 64, 16, 16, s=4, B=2, C=2, fb=2)
    _c2(cases, "adj", "constant", 64, 70, 7, 7, s=2, B=2, C=3, fc=3)
    _c2(cases, "adj", "circular", 256, 256, 16, 16, s=4, B=4, C=3, emu=False)
    _c2(cases, "fwd", "circular", 256, 256, 16, 16, s=4, B=4, C=3, emu=False)
    # ---- 3-D: every mode, even and odd filters, several 64-column blocks
    for mode in ALL:
        _c3(cases, mode, 2, 2, 6, 9, 11, 1, 1, 3, 3, 3)
        _c3(cases, mode, 1, 3, 7, 8, 10, 1, 3, 2, 4, 3)
        _c3(cases, mode, 2, 1, 5, 12, 9, 2, 1, 3, 5, 2)
        _c3(cases, mode, 1, 1, 4, 9, 70, 1, 1, 2, 3, 4)
    # plane chunking (device only): more than 65535 (batch, channel) planes - every kernel's z0 - and more than 65535 depth planes
    _c3(cases, "circular", 1, 65600, 1, 2, 2, 1, 1, 1, 3, 3, emu=False, tag="-chunked")
    _c3(cases, "constant", 1, 1, 65600, 2, 2, 1, 1, 3, 2, 2, emu=False, tag="-chunked")
    _c3(cases, "valid", 1, 1, 65602, 2, 2, 1, 1, 3, 2, 2, emu=False, tag="-chunked")
    # ---- rejections: an error, no launch, the output untouched
    _reject(cases, Conv2(1, 1, 8, 20, 1, 1, 17, 3, "reflect"), "reflect-ph-eq-h")
    _reject(cases, Conv2(1, 1, 20, 5, 1, 1, 3, 10, "reflect"), "reflect-pw-eq-w")
    _reject(cases, Conv2(1, 1, 5, 20, 1, 1, 12, 3, "circular"), "circular-ph-gt-h")
    _reject(cases, Conv2(1, 1, 10, 10, 1, 1, 11, 3, "valid"), "valid-filter-taller")
    _reject(cases, Conv2(1, 1, 10, 10, 1, 1, 3, 11, "valid", 2), "valid-filter-wider-s2")
    _reject(cases, Conv2(1, 65536, 1, 1, 1, 1, 1, 1, "constant"), "planes-65536")
    _reject(cases, Conv2(1, 1, 8, 8, 1, 1, 129, 128, "constant"), "filter-66048B")
    _reject(cases, Conv2(1, 2, 8, 8, 1, 1, 3, 3, 5), "mode-5")
    _reject(cases, Conv2(1, 0, 8, 8, 1, 1, 3, 3, "constant"), "channels-0")
    _reject(cases, Conv2(2, 1, 8, 8, 3, 1, 3, 3, "constant"), "filter-batch-3-of-2")
    _reject(cases, Conv2(1, 2, 8, 8, 1, 1, 3, 3, "constant", 0), "stride-0")
    _reject(cases, Conv3(1, 1, 3, 8, 8, 1, 1, 7, 3, 3, "reflect"), "reflect-pd-eq-d")
    _reject(cases, Conv3(1, 1, 3, 8, 8, 1, 1, 3, 3, 19, "circular"), "circular-pw-gt-w")
    _reject(cases, Conv3(1, 1, 8, 8, 8, 1, 1, 3, 9, 3, "valid"), "valid-filter-taller")
    _reject(cases, Conv3(1, 1, 8, 8, 8, 1, 1, 5, 64, 52, "constant"), "filter-66560B")
    _reject(cases, Conv3(1, 2, 8, 8, 8, 1, 3, 3, 3, 3, "constant"), "filter-channels-3-of-2")
    ids = [c.id for c in cases]
    assert len(ids) == len(set(ids)), "duplicate case ids"
    return cases


CASES = build_cases()


# ------------------------------------------------------------------ the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.conv), `device` of its
    buffers, `stream()` -> the stream argument, and - on the emulation - `launches()`, the kernels launched since `reset()`"""

    def __init__(self, lib, device, stream, reset=None, launches=None):
        self.lib, self.device, self._stream = lib, torch.device(device), stream
        self.reset, self.launches = reset, launches

    def dev(self, t):
        return t.contiguous().to(self.device)

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def call(self, name, d, a, b, out, expect=None):
        """one entry point; out is a tensor or a raw address; asserts the launch log against `expect` where there is one"""
        desc = d.desc()
        if self.reset:
            self.reset()
        optr = out if isinstance(out, int) else out.data_ptr()
        rc = getattr(self.lib, name)(ctypes.byref(desc), ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()),
                                     ctypes.c_void_p(optr), self._stream())
        if self.launches is not None and expect is not None:
            got = self.launches()
            assert got == expect, f"{name}: launched {got}, the restated dispatch expects {expect}"
        return rc

    def run(self, name, d, a, b, out, expect):
        rc = self.call(name, d, a, b, out, expect)
        if rc != 0:
            raise RuntimeError(f"{name} error {rc}: {self.lib.dinv_last_error().decode()}")


def _seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id)) % (2 ** 31)


def worst_ratio(out, ref, bound):
    """max over elements of |out - ref| / bound in fp64 (bound == 0: out must equal ref exactly); NaN counts as infinite"""
    o = out.detach().cpu().double().reshape(ref.shape)
    diff = (o - ref.detach()).abs()
    bnd = bound.detach()
    r = torch.where(bnd > 0, diff / bnd.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), diff))
    if torch.isnan(r).any():
        return float("inf")
    return float(r.max()) if r.numel() else 0.0


def _check_buffer(r, what, g, rerun):
    """guard bands intact, no word left with the poison pattern, a second call into the same (re-poisoned) buffer: the same bits"""
    r.sync()
    assert g.guards_intact(), f"{what}: write outside the output"
    bits = g.bits().clone()
    assert not bool((bits == POISON).any()), f"{what}: {int((bits == POISON).sum())} output words never written"
    g.t.view(torch.int32).fill_(POISON)
    rerun()
    r.sync()
    assert torch.equal(g.bits(), bits), f"{what}: two identical calls differ"
    assert g.guards_intact()


def run_case(r, case):
    """runs `case` on runner `r`, asserts everything it checks and returns the worst error ratio of each operation"""
    gen = torch.Generator().manual_seed(_seed(case))
    if case.rejected:
        return _run_reject(r, case)
    if isinstance(case.conv, Conv3):
        return _run3(r, case, gen)
    return _run2(r, case, gen)


def _grad(fn, wrt):
    wrt = wrt.detach().clone().requires_grad_(True)
    fn(wrt).sum().backward()
    return wrt.grad


def _run2(r, case, gen):
    d = case.conv
    B, C, H, W, s = d.B, d.C, d.H, d.W, d.stride
    Ho, Wo = out_size(H, d.fh, d.mode, s), out_size(W, d.fw, d.mode, s)
    x = torch.randn(B, C, H, W, generator=gen)
    k = torch.randn(d.fb, d.fc, d.fh, d.fw, generator=gen)
    v = torch.randn(B, C, Ho, Wo, generator=gen)
    xd, kd, vd = r.dev(x), r.dev(k), r.dev(v)
    xa, ka, va = x.double().abs(), k.double().abs(), v.double().abs()
    errs = {}
    # forward
    y = Guarded(B * C * Ho * Wo, r.device)
    r.run("dinv_conv2d", d, xd, kd, y.t, case.kernels["fwd"])
    r.sync()
    ref = _ref_conv(x.double(), k.double(), d.mode, s)
    assert tuple(ref.shape) == (B, C, Ho, Wo)
    errs["fwd"] = worst_ratio(y.t, ref, _ref_conv(xa, ka, d.mode, s))
    bound = BOUNDS[case.kernels["fwd"][0]]
    assert errs["fwd"] <= bound, f"forward: worst |y - ref| / (|k| * |x|) {errs['fwd']:.3g} > {bound:.3g}"
    _check_buffer(r, "forward", y, lambda: r.run("dinv_conv2d", d, xd, kd, y.t, case.kernels["fwd"]))
    # transpose, against fp64 autograd of the reference
    xt = Guarded(B * C * H * W, r.device)
    r.run("dinv_conv2d_transpose", d, vd, kd, xt.t, case.kernels["adj"])
    r.sync()
    ref_t = _grad(lambda z: _ref_conv(z, k.double(), d.mode, s) * v.double(), x.double())
    bnd_t = _grad(lambda z: _ref_conv(z, ka, d.mode, s) * va, x.double())
    errs["adj"] = worst_ratio(xt.t, ref_t, bnd_t)
    bound = BOUNDS[case.kernels["adj"][0]]
    assert errs["adj"] <= bound, f"transpose: worst |x - ref| / (|k|^T |v|) {errs['adj']:.3g} > {bound:.3g}"
    _check_buffer(r, "transpose", xt, lambda: r.run("dinv_conv2d_transpose", d, vd, kd, xt.t, case.kernels["adj"]))
    # dot test in fp64: |<A x, v> - <x, A^T v>| within what the two measured element errors allow
    lhs = float((y.t.cpu().double().view(B, C, Ho, Wo) * v.double()).sum())
    rhs = float((x.double() * xt.t.cpu().double().view(B, C, H, W)).sum())
    S = float((xa * bnd_t).sum())
    assert abs(lhs - rhs) <= (errs["fwd"] + errs["adj"] + 1e-12) * S, (lhs, rhs, S)
    # filter gradient per (b, c) plane, against fp64 autograd with a per-plane filter
    dk = Guarded(B * C * d.fh * d.fw, r.device)
    r.run("dinv_conv2d_filter_grad", d, xd, vd, dk.t, case.kernels["fgrad"])
    r.sync()
    kp = k.double().expand(B, C, d.fh, d.fw)
    ref_k = _grad(lambda z: _ref_conv(x.double(), z, d.mode, s) * v.double(), kp)
    bnd_k = _grad(lambda z: _ref_conv(xa, z, d.mode, s) * va, kp)
    errs["fgrad"] = worst_ratio(dk.t, ref_k, bnd_k)
    bound = BOUNDS["conv2d_filter_grad_kernel"]
    assert errs["fgrad"] <= bound, f"filter gradient: worst ratio {errs['fgrad']:.3g} > {bound:.3g}"
    _check_buffer(r, "filter gradient", dk, lambda: r.run("dinv_conv2d_filter_grad", d, xd, vd, dk.t, case.kernels["fgrad"]))
    for name, t, t0 in (("x", xd, x), ("filter", kd, k), ("v", vd, v)):
        assert torch.equal(t.cpu(), t0), f"the calls modified their input {name}"
    return errs


def _run3(r, case, gen):
    d = case.conv
    B, C = d.B, d.C
    Do, Ho, Wo = out_size(d.D, d.fd, d.mode), out_size(d.H, d.fh, d.mode), out_size(d.W, d.fw, d.mode)
    x = torch.randn(B, C, d.D, d.H, d.W, generator=gen)
    k = torch.randn(d.fb, d.fc, d.fd, d.fh, d.fw, generator=gen)
    v = torch.randn(B, C, Do, Ho, Wo, generator=gen)
    xd, kd, vd = r.dev(x), r.dev(k), r.dev(v)
    xa, ka, va = x.double().abs(), k.double().abs(), v.double().abs()
    errs = {}
    y = Guarded(B * C * Do * Ho * Wo, r.device)
    r.run("dinv_conv3d", d, xd, kd, y.t, case.kernels["fwd"])
    r.sync()
    ref = _ref_conv3(x.double(), k.double(), d.mode)
    assert tuple(ref.shape) == (B, C, Do, Ho, Wo)
    errs["fwd"] = worst_ratio(y.t, ref, _ref_conv3(xa, ka, d.mode))
    assert errs["fwd"] <= BOUNDS["conv3d_pad_kernel"], f"forward: worst ratio {errs['fwd']:.3g}"
    _check_buffer(r, "forward", y, lambda: r.run("dinv_conv3d", d, xd, kd, y.t, case.kernels["fwd"]))
    xt = Guarded(B * C * d.D * d.H * d.W, r.device)
    r.run("dinv_conv3d_transpose", d, vd, kd, xt.t, case.kernels["adj"])
    r.sync()
    ref_t = _grad(lambda z: _ref_conv3(z, k.double(), d.mode) * v.double(), x.double())
    bnd_t = _grad(lambda z: _ref_conv3(z, ka, d.mode) * va, x.double())
    errs["adj"] = worst_ratio(xt.t, ref_t, bnd_t)
    assert errs["adj"] <= BOUNDS["conv3d_pad_transpose_kernel"], f"transpose: worst ratio {errs['adj']:.3g}"
    _check_buffer(r, "transpose", xt, lambda: r.run("dinv_conv3d_transpose", d, vd, kd, xt.t, case.kernels["adj"]))
    lhs = float((y.t.cpu().double().view(v.shape) * v.double()).sum())
    rhs = float((x.double() * xt.t.cpu().double().view(x.shape)).sum())
    S = float((xa * bnd_t).sum())
    assert abs(lhs - rhs) <= (errs["fwd"] + errs["adj"] + 1e-12) * S, (lhs, rhs, S)
    dk = Guarded(B * C * d.fd * d.fh * d.fw, r.device)
    r.run("dinv_conv3d_filter_grad", d, xd, vd, dk.t, case.kernels["fgrad"])
    r.sync()
    kp = k.double().expand(B, C, d.fd, d.fh, d.fw)
    ref_k = _grad(lambda z: _ref_conv3(x.double(), z, d.mode) * v.double(), kp)
    bnd_k = _grad(lambda z: _ref_conv3(xa, z, d.mode) * va, kp)
    errs["fgrad"] = worst_ratio(dk.t, ref_k, bnd_k)
    assert errs["fgrad"] <= BOUNDS["conv3d_filter_grad_kernel"], f"filter gradient: worst ratio {errs['fgrad']:.3g}"
    _check_buffer(r, "filter gradient", dk, lambda: r.run("dinv_conv3d_filter_grad", d, xd, vd, dk.t, case.kernels["fgrad"]))
    for name, t, t0 in (("x", xd, x), ("filter", kd, k), ("v", vd, v)):
        assert torch.equal(t.cpu(), t0), f"the calls modified their input {name}"
    return errs


def _run_reject(r, case):
    """every entry point returns an error, launches nothing and leaves its (poisoned, accepted-size) output alone"""
    d = case.conv
    is3 = isinstance(d, Conv3)
    sp = (d.D, d.H, d.W) if is3 else (d.H, d.W)
    fs = (d.fd, d.fh, d.fw) if is3 else (d.fh, d.fw)
    s = 1 if is3 else max(d.stride, 1)
    mode = d.mode if d.mode in MODES else "constant"
    osp = [max(out_size(n, f, mode, s), 1) for n, f in zip(sp, fs)]
    nin, nout, nk = d.B * d.C, d.B * d.C, max(d.fb, 1) * max(d.fc, 1)
    for n in sp:
        nin *= n
    for n in osp:
        nout *= n
    for f in fs:
        nk *= f
    x, v = r.dev(torch.randn(max(nin, 1))), r.dev(torch.randn(max(nout, 1)))
    k = r.dev(torch.randn(max(nk, 1)))
    pre = "dinv_conv3d" if is3 else "dinv_conv2d"
    taps = 1
    for f in fs:
        taps *= f
    for name, a, b, n in ((pre, x, k, nout), (pre + "_transpose", v, k, nin), (pre + "_filter_grad", x, v, d.B * d.C * taps)):
        out = Guarded(max(n, 1), r.device)
        rc = r.call(name, d, a, b, out.t, expect=[])
        assert rc != 0, f"{name} accepted a descriptor make_geom must reject ({rejection(d)})"
        msg = r.lib.dinv_last_error().decode()
        assert rejection(d) in msg, f"rejected for '{msg}', the restated checks expect '{rejection(d)}'"
        r.sync()
        assert out.untouched(), f"{name}: a rejected call wrote to its output"
    return {}
