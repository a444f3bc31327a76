"""Shared by tests/test_drunet_kernels_gpu.py (the gfx950 library) and tests/test_emu_drunet_cases.py (the same kernel sources on the
host emulation): one table of cases for the DRUNet / DnCNN INFERENCE kernels - dinv_act_pack / dinv_act_unpack,
dinv_conv3x3 (+ _bias), dinv_conv3x3_winograd, dinv_conv3x3_winograd4 (+ _bf16x3, _bias), dinv_conv3x3_split, dinv_conv3x3_wsplit,
dinv_conv_down2x2 (+ _bf16s, _bf16x3), dinv_conv_up2x2 (+ _bf16s), dinv_conv3x3_tail (+ _bias) - each meant to reach one kernel
instance at one of its edges; a restatement of every launcher's arithmetic (the table asserts what it reaches); the fp64 references;
and one runner.  Every call goes through ctypes with the product's prototypes (deepinv_amd.hip.drunet._declare) on guarded buffers
(fft_cases.Guarded).

The 3-D forms of these kernels (dinv_conv3x3x3, dinv_conv3x3x3_split, dinv_conv_down2x2_bf16s_3d, dinv_conv_up2x2_bf16s_3d) have a
table of their own, tests/drunet3d_cases.py, built on the helpers of this module (the buffer helpers below take the guard plane and
the depth of a drunet3d.Level for it).

Data classes (per case; `Case.classes()`):

  int      both operands in {-2 .. 2} (x2, residuals and the bias as well): every product and partial sum is an integer (F(2x2): a
           multiple of 1/4, U = G g G^T of an integer filter; the bf16-split kernels: a small integer has a zero low part), so the
           result must equal fp64 BIT FOR BIT whatever the summation order.  Asserted per case: (terms) x (largest product) x
           (1 / quantum) < 2^24; for the Winograd forms the magnitude sum of the actual data stands in for terms x product.
           F(4x4) (G holds 1/6 and 1/24): filters a b^T with a, b from the lattice L = {v in Z^3: v1 = 0, v0 + v2 = 0 (mod 3)} and
           x in {-1, 0, 1}: U is a multiple of 1/64 with |U| <= 4, every quantity the kernel forms is a multiple of 1/64 bounded by
           winograd4_magnitude, exact while mag.max() * 64 < 2^24.  pack_winograd4_weight forms U in fp64 and rounds once, so that
           class asserts |out - ref| <= r * (|A^T| sum_ci (|B^T||d||B|) |A|) with r = max |v - round(64 v) / 64| over the values v of
           the pack that is uploaded (pack_u_values; bf16x3: the three parts summed; printed with -s, with the ceiling's size in
           fp32 roundings of the largest output).  A U formed by matrix
           products leaves ~3.5e-18 where zeros belong (a ceiling near 1e-12); hip/drunet.py: filter_transform skips zero
           coefficients and gives r = 0 on these lattice vectors, i.e. the class is then bit-exact like the others.
  wide-x   one operand in {-2 .. 2}, the other m / 1024 with |m| <= 4095 (12 significant bits: more than bf16 or tf32 hold), both
  wide-w   ways round; bit-exact while terms x 8190 < 2^24, and only if no operand loses mantissa bits on its way to the matrix
           cores.  F(4x4): wide = False (12-bit data times the transform gain exceeds 2^24 quanta; its mantissa check stays with
           the *_worst_case tests of tests/test_emu_drunet.py / test_drunet_gpu.py).
  randn    N(0, 1) inputs, He-scaled weights, per-element ceiling gamma_n x (the same operation on absolute values; the Winograd
           forms: the Winograd magnitude), n = the longest rounding chain read off the code (`chain()` below); the bf16-split
           kernels keep the project's figures: relative l2 < SPLIT_L2 and 3 * 2^-16 x magnitude per element (bf16x3: 2^-22 x
           magnitude), plus one rounding u x |value| for each x2, bias or residual add the case has and 2^-18 x |value| for a
           pre-split output; down_bf16x3 also l2 < 1e-6, and per element 2^-22 + gamma(1.5 cin) for its 1.5 cin accumulator roundings.
  special  pack / unpack: pure copies, bit-equal on +-0, denormals, +-Inf, NaN.  ReLU epilogues (direct, thin, 2-D tiles - the kernels
           in which a NaN input pixel reaches exactly the outputs of the fp64 convolution; a Winograd form spreads it over the tile):
           NaN pre-activations under two input pixels; the reference is fmaxf(v, 0) = +0 there (NOT torch.relu's NaN).  A -0.0
           pre-activation cannot be set up through these kernels: every accumulator starts from +0 and (-0) + (+0) = +0, so it would
           take a summation order in which no +0 term (a zero padding pixel, a padded channel) follows; fmaxf(-0.0, 0) may return a
           zero of either sign (IEEE-754 maxNum leaves it open), which the value comparison of the other classes already allows.

Buffer contracts (read off the kernels; CONTRACT below): what everything outside the interior of an INPUT may hold
and what a launch may write in its OUTPUT.  No forward kernel multiplies slack by an exact zero, so there is no +-1e30 contract here
(the weight gradients of bwd_cases have one); every input slack is NaN, and so is every frame whose outputs are replaced by a
select or never computed."""
import ctypes
import functools
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from bwd_cases import SPECIALS, SPLIT_L2, U, Backend, _p, from_buf, gamma, padded, to_buf
from winograd_ref import winograd4_magnitude

CUS = {"emu": 2, "gpu": 32}           # cus_per_xcd(): the emulated device, the MI355X


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the launchers, restated
def geom_py(B, H, W):
    """dinv_act_geom_init: (hp, wp, plane, np, sl, cs)"""
    hp, wp, plane, np_ = padded(B, H, W)
    sl = wp + 4
    cs = sl + max(cdiv(np_, 512) * 512 + wp + 4, np_ + 34 * wp + 64)
    return hp, wp, plane, np_, sl, (cs + 3) // 4 * 4


def direct_launch(np_, cout_p, tile):
    """conv3_launch (drunet.hip:482): 256-pixel tiles on 8 XCD slots; `idle` = blocks that return early (tile >= ntiles)"""
    ntiles = cdiv(np_, 256)
    tpx = cdiv(ntiles, 8)
    ytiles = cout_p // tile
    return dict(ntiles=ntiles, tpx=tpx, ytiles=ytiles, grid=8 * tpx * ytiles, idle=(8 * tpx - ntiles) * ytiles)


def picks32(np_, cout_p):
    """ConvPacks.pick (hip/drunet.py): the 32-wide pack where the 64-wide grid has fewer than 1536 workgroups"""
    return cout_p % 64 == 0 and cdiv(np_, 256) * (cout_p // 64) < 1536


def _least_waste(tyn, txn, shapes):
    """launch_any of drunet_wino.hip / drunet_wino4.hip: the rectangle with the least padded-tile waste, ties to the first"""
    best, bw = 0, 1e30
    for i, (th, tw) in enumerate(shapes):
        w = float(cdiv(tyn, th) * th * cdiv(txn, tw) * tw)
        if w < bw * 0.999:
            bw, best = w, i
    return shapes[best]


def wino2_launch(B, H, W, cout, cus):
    """drunet_wino.hip:479-518"""
    tyn, txn = (H + 1) // 2, (W + 1) // 2
    th, tw = _least_waste(tyn, txn, ((4, 16), (8, 8), (4, 4)))
    nty, ntx = cdiv(tyn, th), cdiv(txn, tw)
    nsub = 64 // (th * tw)
    nsr = B * nty * ntx
    nwg = cdiv(nsr, nsub) * (cout // 64)
    per_xcd = cdiv(nwg, 8)
    slots = min(per_xcd, cus)
    return dict(rect=(th, tw), filled=tyn % th == 0 and txn % tw == 0, nsub=nsub, nsr=nsr, nwg=nwg, per_xcd=per_xcd, slots=slots,
                tiles_per_wg=cdiv(per_xcd, slots), straddles=nsub > nty * ntx and B > 1)


UBLK = 8 * 9 * 64 * 4


def wino4_launch(B, H, W, cin, cout, cus, workspace):
    """drunet_wino4.hip:722-783"""
    tyn, txn = H // 4, W // 4
    th, tw = _least_waste(tyn, txn, ((4, 8), (4, 4), (2, 2)))
    nty, ntx = cdiv(tyn, th), cdiv(txn, tw)
    nsub = 32 // (th * tw)
    nsr = B * nty * ntx
    ncb, nct = cin // 8, cout // 64
    npw = cdiv(nsr, nsub)
    nwg = npw * nct
    per_xcd = cdiv(nwg, 8)
    ntail = per_xcd % cus
    split_f = 1
    if workspace and ntail > 0:
        for f in (8, 4, 2):
            if ntail * f <= cus and ncb % f == 0 and (ncb // f) % 2 == 0:
                split_f = f
                break
    ntail = ntail if split_f > 1 else 0
    return dict(rect=(th, tw), filled=tyn % th == 0 and txn % tw == 0, nsub=nsub, nsr=nsr, nwg=nwg, per_xcd=per_xcd,
                ct_major=nct * ncb * UBLK * 4 > (3 << 20), split_f=split_f, ntail=ntail, full_x=per_xcd - ntail,
                straddles=nsub > nty * ntx and B > 1)


def split_launch(B, H, W, cout, force):
    """split_launch / launch_s2 (drunet_split2d.hip:291-365); force = bits 8-9 of flags"""
    tc = 32 if W % 32 == 0 else (16 if W % 16 == 0 else 8)
    rows = B * (H + 2)
    n256 = cdiv(rows, 256 // tc) * cdiv(W, tc) * (cout // 64)
    nrep = force if force else (2 if n256 >= 384 else 1)
    tr = 128 * nrep // tc
    return dict(tc=tc, n256=n256, nrep=nrep, tr=tr, ntr=cdiv(rows, tr), ntc=cdiv(W, tc), partial_col=W % tc != 0,
                ragged_row=rows % tr != 0)


def wsplit_launch(B, H, W):
    """dinv_conv3x3_wsplit / launch_ws (drunet_wsplit.hip:345-394)"""
    tc = 32 if W % 32 == 0 else (16 if W % 16 == 0 else 8)
    rows, tr = B * (H + 2), 256 // tc
    return dict(tc=tc, tr=tr, ntr=cdiv(rows, tr), ntc=cdiv(W, tc), partial_col=W % tc != 0, ragged_row=rows % tr != 0,
                image_ends_inside=B > 1 and (H + 2) % tr != 0)


def tail_launch(B, H, W):
    """tail_launch (drunet_tail.hip:157-183): the lane-shift kernel unless the batch exceeds grid.z"""
    if B > 65535:
        return dict(flat=True, nstrip=0, sw=0, rb=0, ragged=False)
    nstrip = cdiv(W, 62)
    sw = cdiv(W, nstrip)
    rb = 8
    while rb > 2 and nstrip * cdiv(H, rb) * B < 2048:
        rb >>= 1
    return dict(flat=False, nstrip=nstrip, sw=sw, rb=rb, ragged=H % rb != 0)


# ------------------------------------------------------------------ contracts
# in_frame: what the frame of x (and x2) holds.  "zero": required - it is the convolution's padding, and the pixel `sl` (top-left frame
#           pixel of image 0) is what F(2x2) / F(4x4) read in place of every out-of-frame pixel (drunet_wino.hip:148,
#           drunet_wino4.hip:257-260: "the (always zero) top-left border pixel").  "nan": never read by a stored output
#           (the stride-2 kernels: interior outputs read interior inputs only; border lanes read pixel `sl` and are not stored /
#           replaced by a select).
# Every input's slack is NaN, every residual's frame and slack are NaN (read only at pixels whose value a select replaces, or not
# at all); padding channels are zero as production leaves them.
# writes:   the pixels of [sl, sl + np) a launch stores to, in the channel blocks it owns.  "all": every pixel below np, frame
#           pixels as exact zeros (select) - frame prefill NaN.  "interior": interior pixels only ("the zero frame is never
#           written") - frame prefill zero, and it must keep those bits.  "rows": columns 1 .. W of EVERY row, frame rows as
#           zeros, frame columns untouched (the 2-D tiles of drunet_split2d.hip / drunet_wsplit.hip).
# Nothing is ever stored into the slack or past np.
CONTRACT = {
    "direct": ("zero", "all"), "wino2": ("zero", "interior"), "wino4": ("zero", "interior"), "wino4x3": ("zero", "interior"),
    "split": ("zero", "rows"), "wsplit": ("zero", "rows"), "tail": ("zero", "interior"),
    "down": ("nan", "all"), "down_bf16s": ("nan", "all"), "down_bf16x3": ("nan", "all"),
    "up": ("nan", "interior"), "up_bf16s": ("nan", "interior"),
}
BF16_KINDS = ("split", "wsplit", "down_bf16s", "up_bf16s")
C3_KINDS = ("direct", "wino2", "wino4", "wino4x3", "split", "wsplit", "tail")


# ------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    id: str
    kind: str                     # pack | unpack | direct | wino2 | wino4 | wino4x3 | split | wsplit | tail | down* | up*
    B: int = 1
    H: int = 1
    W: int = 1                    # the image grid; stride-2 kinds: the HALF grid (down: output, up: input)
    cin: int = 8                  # real channels (the head: 4 of cin_p = 8)
    cout: int = 64                # real channels (cout_valid; the direct kernel pads to 32 / 16)
    mode: str = "plain"           # '+'-joined: relu, res (res1), res2, x2, bias
    tile: int = 0                 # direct: cout tile 16 / 32 / 64, 0 = ConvPacks.pick;  split: bits 8-9 of flags (0 = automatic)
    fmt: str = "f32"              # split: f32 | in_split | out_split;  pack: the sigma form (py | dev | batch | map)
    ws: bool = False              # wino4: with a workspace
    expect: tuple = ()            # what the case must reach (asserted from the restated arithmetic in _check_table)
    split_emu: tuple = ()         # wino4 with a workspace: expected (split_f, ntail) per backend
    split_gpu: tuple = ()
    gpu_only: bool = False
    gpu_only_classes: tuple = ()
    wide: bool = True
    special: bool = False         # run the `special` class (ReLU epilogues)
    note: str = ""

    def has(self, tok):
        return tok in self.mode.split("+")

    def classes(self):
        if self.kind in ("pack", "unpack"):
            return ("special",)
        c = ["int"] + (["wide-x", "wide-w"] if self.wide else []) + ["randn"]
        return tuple(c + (["special"] if self.special else []))


CASES = []


def _add(**kw):
    CASES.append(Case(**kw))


# ---- 1. pack / unpack (64-column blocks)
for _W, _c, _f in ((1, 1, "py"), (63, 3, "dev"), (64, 7, "batch"), (65, 3, "map"), (130, 1, "map"), (130, 7, "batch"), (65, 7, "py")):
    _add(id=f"pack-w{_W}-c{_c}-{_f}", kind="pack", B=2, H=3, W=_W, cin=_c, fmt=_f)
for _W, _c in ((1, 1), (63, 3), (64, 8), (65, 3), (130, 8), (130, 1)):
    _add(id=f"unpack-w{_W}-c{_c}", kind="unpack", B=2, H=3, W=_W, cout=_c)


# ---- 2. dinv_conv3x3 / dinv_conv3x3_bias: conv3x3_kernel<MREP, RELU, NRES, BIAS>, conv3_thin_kernel<RELU, NRES, BIAS>
def _d(B, H, W, cin, cout, mode, tile, expect=(), **kw):
    _add(id=f"direct-{B}x{H}x{W}-c{cin}o{cout}-t{tile}-{mode}", kind="direct", B=B, H=H, W=W, cin=cin, cout=cout, mode=mode, tile=tile,
         expect=expect, **kw)


_d(1, 6, 6, 64, 64, "plain", 64, ("np<256",))                 # both packs of one 64-multiple layer: MREP 2 ...
_d(1, 6, 6, 64, 64, "plain", 32)                              # ... and MREP 1
_d(1, 14, 14, 16, 64, "relu", 64, ("np=256",), special=True)
_d(1, 14, 14, 16, 64, "relu+res", 32)
_d(1, 14, 18, 8, 64, "res", 64, ("ragged",))
_d(1, 14, 18, 8, 64, "res+res2", 32)
_d(1, 46, 42, 8, 64, "x2", 64, ("9tiles",))                   # tiles_per_xcd = 2: 7 of the 16 tile slots return early
_d(1, 46, 42, 8, 128, "res+res2", 64, ("9tiles",))            # two cout tiles
_d(1, 46, 42, 8, 64, "relu+res+res2", 32, ("9tiles",))
_d(3, 1, 1, 16, 64, "plain", 32)                              # B = 3 of 1 x 1
_d(1, 14, 18, 16, 96, "relu", 32)                             # cout = 96: 32-wide only
_d(1, 6, 6, 8, 128, "plain", 32)                              # four 32-wide cout tiles
_d(2, 9, 14, 64, 3, "x2", 32, ("tail-layer",))                # the tail layer: x2 + cout_valid = 3 of 32, ONE output block
_d(1, 6, 6, 8, 8, "plain", 32)                                # cout_valid = 8 of 32: a whole block, and not one more (cblocks_valid)
_d(1, 6, 6, 8, 8, "plain", 16)                                # ... the thin kernel's `cb >= cblocks_valid` at cout_valid = 8 of 16
_d(2, 9, 14, 4, 64, "plain", 64, ("head",))                   # the head: cin_p = 8 with 4 valid channels
_d(2, 9, 14, 4, 64, "plain", 0, ("head", "pick32"))           # ... as production launches it: the pack ConvPacks.pick returns
_d(2, 9, 14, 16, 2, "plain", 16)                              # thin (tile 16): cout_valid = 2 ...
_d(2, 9, 14, 16, 16, "relu", 16, special=True)                # ... and 16
_d(1, 14, 18, 64, 2, "res", 16)
_d(1, 46, 42, 8, 16, "relu", 16, ("9tiles",))
for _t, _co in ((16, 16), (32, 32), (64, 64)):                # dinv_conv3x3_bias: relu, res, plain on each of thin, 32, 64
    _d(1, 14, 18, 8, _co, "bias", _t)
    _d(1, 14, 18, 8, _co, "bias+relu", _t)
    _d(2, 5, 6, 16, _co, "bias+res", _t)


# ---- 3. dinv_conv3x3_winograd (F(2x2); not part of the emulation build: its LDS barrier is inline assembly)
def _w2(B, H, W, cin, cout, mode, rect, filled, expect=(), **kw):
    _add(id=f"wino2-{B}x{H}x{W}-c{cin}o{cout}-{mode}", kind="wino2", B=B, H=H, W=W, cin=cin, cout=cout, mode=mode, gpu_only=True,
         expect=(rect, filled) + expect, **kw)


_w2(1, 8, 32, 32, 64, "plain", (4, 16), True)
_w2(1, 6, 60, 32, 64, "relu", (4, 16), False)
_w2(1, 16, 16, 64, 64, "res", (8, 8), True, wide=False,
    note="wide = False: at cin = 64 the magnitude sum of 12-bit data reaches 1.26 x 2^24 quanta of 1/4096; cin = 32 and 48 carry the class")
_w2(1, 14, 14, 48, 64, "plain", (8, 8), False)                # cin = 48: six blocks, the pair pipeline with the peeled last four
_w2(1, 8, 8, 32, 128, "relu", (4, 4), True)                   # cout = 128
_w2(1, 37, 51, 32, 64, "res", (4, 4), False)                  # odd H and odd W
_w2(1, 1, 1, 32, 64, "plain", (4, 4), False)
_w2(1, 2, 330, 32, 64, "relu", (4, 4), False)
_w2(3, 8, 8, 48, 64, "res", (4, 4), True, ("straddles",))     # four rectangles per workgroup: one workgroup holds three images
_w2(1028, 1, 1, 32, 64, "plain", (4, 4), False, ("walks",))   # 257 workgroups > 8 x 32: a workgroup walks a second tile on the device


# ---- 4. dinv_conv3x3_winograd4 / _bf16x3 / _bias
def _w4(B, H, W, cin, cout, mode, rect, filled, ws=False, emu=(), gpu=(), expect=(), kinds=("wino4", "wino4x3"), **kw):
    for k in kinds:
        _add(id=f"{k}-{B}x{H}x{W}-c{cin}o{cout}-{mode}{'-ws' if ws else ''}", kind=k, B=B, H=H, W=W, cin=cin, cout=cout, mode=mode,
             ws=ws, expect=(rect, filled) + expect, split_emu=emu, split_gpu=gpu, wide=False,
             note="wide = False: 12-bit data times the F(4x4) transform gain exceeds 2^24 quanta", **kw)


_w4(1, 16, 32, 16, 64, "plain", (4, 8), True)                               # without a workspace
_w4(1, 12, 60, 16, 64, "relu", (4, 8), False)
_w4(1, 16, 16, 32, 128, "res", (4, 4), True, ws=True, emu=(2, 1), gpu=(2, 1), expect=("all-tail",))
_w4(3, 16, 12, 16, 64, "res", (4, 4), False, ws=True, emu=(1, 0), gpu=(1, 0))           # cin 16: (ncb / f) % 2 fails for every f
_w4(1, 8, 8, 32, 64, "plain", (2, 2), True, ws=True, emu=(2, 1), gpu=(2, 1), expect=("all-tail",))      # full_x == 0
_w4(1, 20, 36, 16, 64, "relu", (2, 2), False)
_w4(1, 4, 332, 16, 64, "plain", (2, 2), False)
_w4(1, 4, 4, 16, 64, "plain", (2, 2), False)
_w4(5, 8, 8, 64, 64, "relu", (2, 2), True, ws=True, emu=(2, 1), gpu=(4, 1), expect=("all-tail", "straddles"))
_w4(2, 8, 8, 128, 64, "res", (2, 2), True, ws=True, emu=(2, 1), gpu=(8, 1), expect=("all-tail",))
_w4(1, 8, 8, 48, 64, "plain", (2, 2), True, ws=True, emu=(1, 0), gpu=(1, 0), expect=("unsplit-48",))    # stays unsplit
_w4(72, 8, 8, 32, 64, "plain", (2, 2), True, ws=True, emu=(1, 0), gpu=(2, 2), expect=("ntail0-emu",))   # emulation: per_xcd = 2 = cpx
_w4(2000, 4, 4, 16, 64, "plain", (2, 2), False, ws=True, emu=(), gpu=(1, 0), expect=("ntail0-gpu",), gpu_only=True)   # per_xcd = 32
_w4(1, 8, 8, 176, 128, "plain", (2, 2), True, expect=("ct-major",))                    # nct ncb UBLK 4 > 3 MiB: cout tile outermost
_w4(136, 8, 8, 32, 64, "res", (2, 2), True, ws=True, emu=(2, 1), gpu=(2, 3), expect=("full+tail-emu",),
    gpu_only_classes=("randn",))                                                       # emulation: per_xcd = 3 = cpx + 1
_w4(136, 8, 8, 32, 64, "relu", (2, 2), True, ws=True, emu=(2, 1), gpu=(2, 3), expect=("full+tail-emu",), gpu_only_classes=("randn",))
_w4(2112, 8, 8, 32, 64, "res", (2, 2), True, ws=True, emu=(), gpu=(2, 1), expect=("full+tail-gpu",), gpu_only=True)    # per_xcd = 33
_w4(2112, 8, 8, 32, 64, "relu", (2, 2), True, ws=True, emu=(), gpu=(2, 1), expect=("full+tail-gpu",), gpu_only=True)
_w4(1, 16, 32, 16, 64, "bias", (4, 8), True, kinds=("wino4",))                         # dinv_conv3x3_winograd4_bias: plain ...
_w4(5, 8, 8, 64, 64, "bias+relu", (2, 2), True, ws=True, emu=(2, 1), gpu=(4, 1), kinds=("wino4",))      # ... relu, bias by the combiner


# ---- 5. dinv_conv3x3_split (flag bits 8-9 through ctypes)
def _s(B, H, W, cin, cout, mode, fmt, tile, expect=(), **kw):
    _add(id=f"split-{B}x{H}x{W}-c{cin}o{cout}-{mode}-{fmt}-n{tile}", kind="split", B=B, H=H, W=W, cin=cin, cout=cout, mode=mode, fmt=fmt,
         tile=tile, expect=expect, **kw)


_s(1, 8, 32, 16, 64, "plain", "f32", 1, ("tc32",))
_s(1, 8, 32, 16, 64, "relu", "out_split", 2, ("tc32",))
_s(3, 16, 16, 32, 64, "res", "in_split", 1, ("tc16",))
_s(3, 16, 16, 32, 64, "plain", "f32", 2, ("tc16",))
_s(2, 9, 8, 16, 64, "relu", "in_split", 2, ("tc8",), special=True)
_s(1, 17, 33, 32, 128, "res", "f32", 1, ("tc8", "partial-col"))              # 33 columns: a partial column tile
_s(1, 17, 33, 16, 64, "plain", "out_split", 2, ("tc8", "partial-col"))
_s(2, 9, 14, 16, 64, "plain", "in_split", 0, ("auto1",))                     # automatic: n256 far below 384
_s(376, 2, 8, 16, 512, "res", "f32", 0, ("auto1", "n256=376"), gpu_only=True)   # one automatic case on each side of n256 = 384
_s(377, 2, 8, 16, 512, "res", "f32", 0, ("auto2", "n256=384"), gpu_only=True)


# ---- 6. dinv_conv3x3_wsplit
def _ws(B, H, W, cin, cout, mode, expect=(), **kw):
    _add(id=f"wsplit-{B}x{H}x{W}-c{cin}o{cout}-{mode}", kind="wsplit", B=B, H=H, W=W, cin=cin, cout=cout, mode=mode, expect=expect, **kw)


_ws(1, 5, 2, 16, 64, "plain", ("tc8", "partial-col"))
_ws(1, 12, 34, 32, 64, "relu", ("tc8", "partial-col", "ragged-row"))
_ws(3, 9, 32, 16, 128, "res", ("tc32", "ragged-row", "ends-inside"))         # hp = 11 rows per image against 8-row tiles
_ws(3, 9, 16, 32, 64, "plain", ("tc16", "ragged-row", "ends-inside"))
_ws(2, 14, 8, 16, 64, "res", ("tc8",))                                       # rows = 32: exactly one row tile


# ---- 7. stride 2 (B x H x W = the half grid); non-square filters: a missing transpose cannot cancel
def _st(kind, B, H, W, cin, cout, mode="plain", expect=(), **kw):
    _add(id=f"{kind}-{B}x{H}x{W}-c{cin}o{cout}-{mode}", kind=kind, B=B, H=H, W=W, cin=cin, cout=cout, mode=mode, expect=expect, **kw)


_st("down", 2, 1, 1, 8, 64)
_st("down", 2, 5, 6, 24, 128)
_st("down", 1, 46, 42, 8, 128, expect=("9tiles",))                           # ceil(np_out / 256) = 9 > 8
_st("down", 1, 46, 42, 24, 64, expect=("9tiles",))
for _k in ("down_bf16s", "down_bf16x3"):                                     # NPL = 2 / 3
    _st(_k, 2, 1, 1, 16, 64)
    _st(_k, 2, 5, 6, 32, 128)
    _st(_k, 1, 46, 42, 16, 128, expect=("9tiles",))
_st("up", 2, 1, 1, 24, 64, "x2", ("np<128",))
_st("up", 1, 5, 6, 64, 128, "plain", ("np<128",))
_st("up", 1, 6, 14, 24, 128, "plain", ("np=128",))
_st("up", 1, 6, 14, 64, 64, "x2", ("np=128",))
_st("up", 1, 46, 42, 24, 64, "x2", ("np>128",))
_st("up_bf16s", 2, 1, 1, 64, 64, "plain", ("np<128",))
_st("up_bf16s", 1, 5, 6, 64, 128, "x2", ("np<128",))
_st("up_bf16s", 1, 6, 14, 64, 128, "x2", ("np=128",))
_st("up_bf16s", 1, 46, 42, 64, 64, "plain", ("np>128",))


# ---- 8. dinv_conv3x3_tail / _tail_bias
def _t(B, H, W, cin, cout, mode, expect=(), **kw):
    _add(id=f"tail-{B}x{H}x{W}-c{cin}o{cout}-{mode}", kind="tail", B=B, H=H, W=W, cin=cin, cout=cout, mode=mode, expect=expect, **kw)


_t(2, 5, 62, 16, 1, "plain", ("strips1", "rb2", "ragged"))
_t(1, 4, 63, 8, 2, "x2", ("strips2", "rb2"))
_t(1, 3, 124, 16, 3, "bias", ("strips2", "rb2", "ragged"))
_t(1, 5, 125, 8, 4, "bias+res", ("strips3", "rb2", "ragged"))
_t(2, 9, 21, 64, 3, "x2", ("strips1", "rb2", "ragged"))                      # DRUNet's last layer
_t(700, 9, 2, 8, 3, "x2", ("rb4", "ragged"), gpu_only=True)                  # (the emulation takes 15 s for these two: 700 / 1024 images)
_t(1024, 9, 2, 8, 1, "bias+res", ("rb8", "ragged"), gpu_only=True)
_t(65536, 1, 1, 8, 2, "x2", ("flat",), gpu_only=True)                        # batch > 65535: the flat tail3x3_kernel
_t(65536, 1, 1, 8, 4, "bias+res", ("flat",), gpu_only=True)

assert len({c.id for c in CASES}) == len(CASES)
BY_ID = {c.id: c for c in CASES}


def reached(c, backend):
    """what case c reaches on `backend` ("emu" | "gpu"), from the restated launcher arithmetic: a set of regime names"""
    cus = CUS[backend]
    hp, wp, plane, np_, sl, cs = geom_py(c.B, c.H, c.W)
    r = set()
    if c.kind == "direct":
        cout_p = 16 if c.tile == 16 else cdiv(c.cout, 32) * 32
        tile = c.tile or (32 if picks32(np_, cout_p) else 64)
        if c.tile == 0 and tile == 32:
            r.add("pick32")
        d = direct_launch(np_, cout_p, tile)
        r |= {"np<256"} if np_ < 256 else ({"np=256"} if np_ == 256 else set())
        if np_ % 256 and np_ > 256:
            r.add("ragged")
        if d["ntiles"] == 9 and d["tpx"] == 2 and d["idle"] > 0:
            r.add("9tiles")
        if c.cin % 8:
            r.add("head")
        if c.has("x2") and cdiv(c.cout, 8) == 1 and cout_p == 32:
            r.add("tail-layer")
    elif c.kind == "wino2":
        d = wino2_launch(c.B, c.H, c.W, c.cout, cus)
        r |= {d["rect"], d["filled"]}
        if d["straddles"]:
            r.add("straddles")
        if d["nwg"] > 8 * cus and d["tiles_per_wg"] > 1:
            r.add("walks")
    elif c.kind in ("wino4", "wino4x3"):
        d = wino4_launch(c.B, c.H, c.W, c.cin, c.cout, cus, c.ws)
        r |= {d["rect"], d["filled"]}
        if d["straddles"]:
            r.add("straddles")
        if d["ct_major"]:
            r.add("ct-major")
        if c.ws and d["split_f"] > 1 and d["full_x"] == 0:
            r |= {"all-tail", "all-tail-" + backend}
        if c.ws and d["split_f"] > 1 and d["full_x"] > 0:
            r.add("full+tail-" + backend)
        if c.ws and d["per_xcd"] % cus == 0:
            r.add("ntail0-" + backend)
        if c.ws and c.cin == 48 and d["per_xcd"] % cus and d["split_f"] == 1:
            r.add("unsplit-48")
        r.add(("split", d["split_f"], d["ntail"]))
    elif c.kind == "split":
        d = split_launch(c.B, c.H, c.W, c.cout, c.tile)
        r |= {f"tc{d['tc']}", f"n256={d['n256']}"}
        if d["partial_col"]:
            r.add("partial-col")
        if not c.tile:
            r.add(f"auto{d['nrep']}")
    elif c.kind == "wsplit":
        d = wsplit_launch(c.B, c.H, c.W)
        r.add(f"tc{d['tc']}")
        r |= {n for n, k in (("partial-col", "partial_col"), ("ragged-row", "ragged_row"), ("ends-inside", "image_ends_inside")) if d[k]}
    elif c.kind.startswith("down"):
        if cdiv(np_, 256) > 8:
            r.add("9tiles")
    elif c.kind.startswith("up"):
        r.add("np<128" if np_ < 128 else ("np=128" if np_ == 128 else "np>128"))
    elif c.kind == "tail":
        d = tail_launch(c.B, c.H, c.W)
        if d["flat"]:
            r.add("flat")
        else:
            r |= {f"strips{d['nstrip']}", f"rb{d['rb']}"} | ({"ragged"} if d["ragged"] else set())
    return r


def _check_table():
    """every case reaches what its `expect` says, on every backend that runs it (names ending in -emu / -gpu: on that backend)"""
    for c in CASES:
        for backend in ("emu", "gpu"):
            if backend == "emu" and c.gpu_only:
                continue
            got = reached(c, backend)
            for e in c.expect:
                if isinstance(e, str) and e[-4:] in ("-emu", "-gpu") and e[-3:] != backend:
                    continue
                assert e in got, (c.id, backend, e, got)
            want = c.split_emu if backend == "emu" else c.split_gpu
            if c.kind in ("wino4", "wino4x3"):
                assert (("split",) + want in got) if c.ws else (("split", 1, 0) in got and not want), (c.id, backend, want, got)


_check_table()


def items(emu):
    out = []
    for c in CASES:
        if emu and c.gpu_only:
            continue
        out += [(c, k) for k in c.classes() if not (emu and k in c.gpu_only_classes)]
    return out


def item_id(v):
    return v.id if isinstance(v, Case) else str(v)


# ------------------------------------------------------------------ rounding chains (randn ceilings), read off the code
def chain(c, backend):
    """the longest chain of fp32 roundings behind one output element (F(4x4): of the launch `backend` makes).
    direct / thin / tail / stride 2 (fp32): one fused multiply-add per term of the 9 cin_p (4 cin) sum - the tail kernel: a product
      and an add per term, 2 x 9 cin -, plus one for each of the x2 add, the bias and each residual.
    F(2x2): B^T d B is one add per pass (2), U is rounded once (1), cin accumulations, A^T M A two adds per pass (4), + residual / bias.
    F(4x4): B^T d B at most three roundings per pass (6: 4 xa - 5 xb + xc, p + be qq with p, qq one fma each), U rounded once (1), cin
      accumulations - cin / split_f in a part of a tail tile -, A^T M A at most six roundings per pass (12: five additions and the
      scaled terms 2 s, 4 s, 8 s are exact), the tail-split combine where it runs (split_f - 1 additions: wino4_launch), bias / residual."""
    extra = sum(c.has(t) for t in ("x2", "bias", "res", "res2"))
    if c.kind == "direct":
        return 9 * cdiv(c.cin, 8) * 8 + extra
    if c.kind == "tail":
        return 2 * 9 * c.cin + extra
    if c.kind in ("down", "up"):
        return 4 * c.cin + extra
    if c.kind == "wino2":
        return 2 + 1 + c.cin + 4 + extra
    if c.kind in ("wino4", "wino4x3"):
        f = wino4_launch(c.B, c.H, c.W, c.cin, c.cout, CUS[backend], c.ws)["split_f"]
        whole = 6 + 1 + c.cin + 12                    # a whole tile (full_x > 0, or nothing split)
        part = 6 + 1 + c.cin // f + 12 + (f - 1)      # a tail tile: the longer of the two holds for every output
        return max(whole, part) + extra
    raise ValueError(c.kind)


# ------------------------------------------------------------------ data
def _gen(case, cls):
    return torch.Generator().manual_seed(zlib.crc32(f"{case.id}/{cls}".encode()))


def _small(shape, gen, lim=2):
    return torch.randint(-lim, lim + 1, shape, generator=gen).float()


def _wide(shape, gen):
    return torch.randint(-4095, 4096, shape, generator=gen).float() / 1024


LATTICE = torch.tensor([[1., 0., -1.], [1., 0., 2.], [0., 3., 0.], [2., 0., 1.], [1., 3., -1.], [-1., 0., 1.], [0., 0., 0.]])


def lattice_filters(cout, cin, gen):
    """filters a b^T with a, b drawn from L = {v in Z^3: v1 = 0, v0 + v2 = 0 (mod 3)}: G a is a multiple of 1/8 with |G a| <= 2 for
    these vectors, so U = (G a)(G b)^T is a multiple of 1/64 with |U| <= 4"""
    a = LATTICE[torch.randint(0, len(LATTICE), (cout, cin), generator=gen)]
    b = LATTICE[torch.randint(0, len(LATTICE), (cout, cin), generator=gen)]
    return a[..., :, None] * b[..., None, :]


def winograd2_magnitude(x, w):
    """|A^T| [ sum_ci |G g G^T| . (|B^T| |d| |B|) ] |A| of Winograd F(2x2, 3x3) in fp64 (winograd_ref.winograd4_magnitude's sibling);
    odd heights / widths: the tiles that stick out are computed on zero padding and cut"""
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
    bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64).abs()
    at = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64).abs()
    B, cin, H, W = x.shape
    He, We = (H + 1) // 2 * 2, (W + 1) // 2 * 2
    Um = (G @ w.double() @ G.t()).abs()
    xp = F.pad(x.double().abs(), (1, 1 + We - W, 1, 1 + He - H))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)
    V = bt @ d @ bt.t()
    M = torch.einsum("ocij,bcyxij->boyxij", Um, V)
    Y = at @ M @ at.t()
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(B, w.shape[0], He, We)[:, :, :H, :W]


def winograd4_input_magnitude(x):
    """|A^T| [ sum_ci |B^T| |d| |B| ] |A| of Winograd F(4x4, 3x3) in fp64, [B, H, W]: winograd4_magnitude with every |U| = 1 - what an
    error of U is multiplied by"""
    from deepinv_amd.hip.drunet import winograd4_matrices
    bt, _, at = (m.abs() for m in winograd4_matrices())
    B, cin, H, W = x.shape
    d = F.pad(x.double().abs(), (1, 1, 1, 1)).unfold(2, 6, 4).unfold(3, 6, 4)
    Y = at @ (bt @ d @ bt.t()).sum(1) @ at.t()                                             # [B, ty, tx, 4, 4]
    return Y.permute(0, 1, 3, 2, 4).reshape(B, H, W)


def wsplit_magnitude(x, w):
    """sum over the Winograd F(2,3) points of an output pixel of |U_k| conv |V_k| (fp64): what the operand-split error of
    csrc/drunet_wsplit.hip is relative to (even columns: points 0, 1, 2; odd columns: 1, 2, 3)"""
    B, C, H, W = x.shape
    g = w.double()
    Um = torch.stack((g[..., 0], (g[..., 0] + g[..., 1] + g[..., 2]) / 2, (g[..., 0] - g[..., 1] + g[..., 2]) / 2, g[..., 2])).abs()
    xp = F.pad(x.double(), (1, 1, 1, 1))
    d0, d1, d2, d3 = xp[..., 0:W:2], xp[..., 1:W + 1:2], xp[..., 2:W + 2:2], xp[..., 3:W + 3:2]
    V = [(d0 - d2).abs(), (d1 + d2).abs(), (d2 - d1).abs(), (d1 - d3).abs()]
    M = [F.conv2d(V[k], Um[k].unsqueeze(-1)) for k in range(4)]
    return torch.stack((M[0] + M[1] + M[2], M[1] + M[2] + M[3]), -1).reshape(B, -1, H, W)


def bf16_split(t, parts=2):
    """what the kernels' split8 / split3 make of fp32 values: the sum of the `parts` bf16 parts (round to nearest even each)"""
    from deepinv_amd.hip.drunet import _bf16_parts
    return sum(p.float() for p in _bf16_parts(t, parts))


def _conv(c, x, w):
    if c.kind in C3_KINDS:
        return F.conv2d(x, w, padding=1)
    if c.kind.startswith("down"):
        return F.conv2d(x, w, stride=2)
    return F.conv_transpose2d(x, w, stride=2)


def _shapes(c):
    """(x, w, out) shapes"""
    B, H, W = c.B, c.H, c.W
    if c.kind in C3_KINDS:
        return (B, c.cin, H, W), (c.cout, c.cin, 3, 3), (B, c.cout, H, W)
    if c.kind.startswith("down"):
        return (B, c.cin, 2 * H, 2 * W), (c.cout, c.cin, 2, 2), (B, c.cout, H, W)
    return (B, c.cin, H, W), (c.cin, c.cout, 2, 2), (B, c.cout, 2 * H, 2 * W)


@functools.lru_cache(maxsize=2)
def data(c, cls):
    """operands, the fp64 reference, the magnitude sum and the asserted exactness precondition of one (case, class) - computed once,
    shared by the tests that need it, never modified"""
    gen = _gen(c, cls)
    xs, wsh, osh = _shapes(c)
    w4 = c.kind in ("wino4", "wino4x3")
    taps = 9 if c.kind in C3_KINDS else 4
    he = 1.0 / (taps * c.cin) ** 0.5
    if cls in ("int", "special"):
        x = _small(xs, gen, 1 if w4 else 2)
        w = lattice_filters(c.cout, c.cin, gen) if w4 else _small(wsh, gen)
    elif cls == "wide-x":
        x, w = _wide(xs, gen), _small(wsh, gen)
    elif cls == "wide-w":
        x, w = _small(xs, gen), _wide(wsh, gen)
    else:
        x, w = torch.randn(xs, generator=gen), torch.randn(wsh, generator=gen) * he
    exact = cls != "randn"
    draw = (lambda s: _small(s, gen)) if exact else (lambda s: torch.randn(s, generator=gen))
    drawx = (lambda s: _wide(s, gen)) if cls == "wide-x" else draw
    x2 = drawx(xs) if c.has("x2") else None
    res1 = draw(osh) if c.has("res") else None
    res2 = draw(osh) if c.has("res2") else None
    bias = draw((c.cout,)) if c.has("bias") else None
    if c.fmt == "in_split" and not exact:
        x = bf16_split(x)                             # the operand the kernel really sees (exact classes: 12 bits fit two parts)
    if cls == "special":                              # NaN pre-activations under two input pixels (all channels of one, one of another)
        x[0, :, 0, 0] = float("nan")
        x[-1, 0, -1, -1] = float("nan")
    xe = x if x2 is None else x + x2                  # exact classes: the sum is exact (13 bits); randn: ONE rounding, counted in chain()
    xe64 = xe.double() if exact else (x.double() + x2.double() if x2 is not None else x.double())
    w64 = w.double()
    ref = _conv(c, xe64, w64)
    pre_mag = _conv(c, xe64.abs() if x2 is None else x.double().abs() + x2.double().abs(), w64.abs())
    # the magnitude every rounding is relative to
    if c.kind == "wino2":
        mag = winograd2_magnitude(xe64, w)
    elif w4:
        mag = winograd4_magnitude(xe64, w)
    elif c.kind == "wsplit":
        mag = wsplit_magnitude(xe64, w)
    else:
        mag = pre_mag
    if cls == "special":
        mag = torch.nan_to_num(mag, nan=0.0)
    conv_mag = mag
    if bias is not None:
        ref, mag = ref + bias.double()[None, :, None, None], mag + bias.double().abs()[None, :, None, None]
    if c.has("relu"):
        ref = ref.relu() if cls != "special" else torch.where(torch.isnan(ref), torch.zeros_like(ref), ref.relu())
    for r_ in (res1, res2):
        if r_ is not None:
            ref, mag = ref + r_.double(), mag + r_.double().abs()
    d = dict(x=x, x2=x2, w=w, bias=bias, res1=res1, res2=res2, ref=ref, mag=mag)
    # ---- exactness preconditions: asserted, not assumed
    if exact and cls != "special":
        if w4:                                        # quanta of 1/64; the cap of the issue: mag.max() * 64 < 2^24
            assert float(mag.max()) * 64 < 2 ** 24, (c.id, float(mag.max()) * 64 / 2 ** 24)
            from deepinv_amd.hip.drunet import filter_transform, winograd4_matrices
            u64 = filter_transform(winograd4_matrices()[1].tolist(), w.double())
            assert float(((u64 * 64).round() / 64 - u64).abs().max()) < 1e-15 and float(u64.abs().max()) <= 4      # the lattice holds
            d["in_mag"] = winograd4_input_magnitude(xe64)[:, None].expand_as(ref)      # |A^T| sum_ci (|B^T||d||B|) |A|; r: run_conv
        else:
            quantum = 1 if cls == "int" else 1024
            if c.kind == "wino2":
                quantum *= 4
            if c.kind == "wsplit":
                quantum *= 2
            assert float(mag.max()) * quantum < 2 ** 24, (c.id, cls, float(mag.max()) * quantum / 2 ** 24)
            terms = taps * c.cin if c.kind in C3_KINDS or c.kind.startswith("down") else c.cin
            prod = (4 if cls == "int" else 8190 / 1024) * (2 if x2 is not None else 1)
            if c.kind not in ("wino2", "wsplit"):     # the sufficient condition of the issue, in its own words
                assert (terms * prod + 2 * sum(c.has(t) for t in ("bias", "res", "res2"))) * quantum < 2 ** 24, c.id
    d["conv_mag"] = conv_mag
    return d


# ------------------------------------------------------------------ buffers
def _nan_frame(g, a, guard=0, depth=0):
    """NaN on the whole frame of an activation buffer (interior kept); guard: pixels in front of the buffer proper (drunet3d.Level);
    depth: the images are volumes of depth + 2 slices, and the two end slices of each are NaN as well"""
    cb, n, H, W = a.shape[0], g.batch, g.height, g.width
    av = a[:, guard + g.sl:guard + g.sl + g.np].view(cb, n, g.hp, g.wp, 8)
    inner = av[:, :, 1:H + 1, 1:W + 1].clone()
    av[:] = float("nan")
    if depth:
        av.view(cb, n // (depth + 2), depth + 2, g.hp, g.wp, 8)[:, :, 1:-1, 1:H + 1, 1:W + 1] = \
            inner.view(cb, n // (depth + 2), depth + 2, H, W, 8)[:, :, 1:-1]
    else:
        av[:, :, 1:H + 1, 1:W + 1] = inner
    return a


def in_buf(be, g, imgs, frame="zero", split=False, guard=0, depth=0):
    """a Guarded input buffer [C/8, cs, 8]: zero padding channels, `frame` on the frame (depth: and on the end slices of every volume),
    NaN on everything outside [sl, sl + np) - the guard planes of a drunet3d.Level (guard pixels at each end) included"""
    a = to_buf(g, imgs, "nan", guard)
    if guard:
        a[:, :guard] = float("nan")
        a[:, g.cs - guard:] = float("nan")
    if frame == "nan":
        _nan_frame(g, a, guard, depth)
    if split:                                         # pre-split: 8 bf16 high parts then 8 bf16 low parts in the same 32 bytes
        hi = a.bfloat16()
        lo = (a - hi.float()).bfloat16()
        a = torch.cat((hi, lo), dim=-1).view(torch.float32).contiguous()
    gb = be.guarded(a.numel(), be.dev(a))
    return gb


def masks(g, guard=0, depth=0):
    """(interior, in-range) boolean masks over the cs pixels of a channel-block row; guard: pixels in front of the buffer proper;
    depth: volumes of depth + 2 slices, whose end slices are no interior"""
    lo = guard + g.sl
    inside = torch.zeros(g.cs, dtype=torch.bool)
    inside[lo:lo + g.np] = True
    inner = torch.zeros(g.cs, dtype=torch.bool)
    iv = inner[lo:lo + g.np].view(g.batch, g.hp, g.wp)
    if depth:
        iv.view(g.batch // (depth + 2), depth + 2, g.hp, g.wp)[:, 1:-1, 1:g.height + 1, 1:g.width + 1] = True
    else:
        iv[:, 1:g.height + 1, 1:g.width + 1] = True
    return inner, inside


def write_mask(g, writes, guard=0, depth=0):
    """the pixels a launch stores to: "all" | "interior" | "rows", or the mask itself"""
    if isinstance(writes, torch.Tensor):
        return writes
    inner, inside = masks(g, guard, depth)
    if writes == "all":
        return inside
    if writes == "interior":
        return inner
    m = torch.zeros(g.cs, dtype=torch.bool)
    m[guard + g.sl:guard + g.sl + g.np].view(g.batch, g.hp, g.wp)[:, :, 1:g.width + 1] = True       # "rows"
    return m


PO2 = 0x7FD1C0DE                  # the prefill of words a launch must not write (a NaN no kernel produces; the guards hold POISON)


def out_buf(be, g, blocks, owned, writes, lanes=8, guard=0, depth=0, hold=0):
    """a Guarded output buffer of `blocks` channel blocks of which the launch owns the first `owned` (channels < lanes of them):
    interior NaN, frame NaN where the launch writes zeros and `hold` (bits; zero unless told) where it never writes, everything else
    PO2.  Returns (Guarded, the prefill bits, the mask of words the launch may write)"""
    inner, inside = masks(g, guard, depth)
    wm = write_mask(g, writes, guard, depth)
    pre = torch.full((blocks, g.cs, 8), PO2, dtype=torch.int32)
    may = torch.zeros((blocks, g.cs, 8), dtype=torch.bool)
    nanbits = torch.tensor(float("nan")).view(torch.int32)
    for b in range(owned):
        fz = pre[b, inside & ~inner]
        fz[:, :lanes] = hold                          # frame the launch leaves alone: zero, and it keeps those bits (lanes it does
        pre[b, inside & ~inner] = fz                  # not own - channels 4 .. 7 of the tail - stay PO2 on the frame as well)
        fw = pre[b, wm & ~inner]
        fw[:, :lanes] = nanbits                       # frame the launch writes: NaN, must come back as exact zeros
        pre[b, wm & ~inner] = fw
        pre[b, inner, :lanes] = nanbits
        may[b, wm, :lanes] = True
    gb = be.guarded(pre.numel(), be.dev(pre.view(torch.float32)))
    return gb, pre, may


def check_out(c, cls, g, gb, pre, may, owned, lanes=8, frame_poison=False, guard=0, depth=0, writes=None):
    """guards intact; every word the launch may not write keeps its prefill bits; the frame of the owned blocks is exactly zero (or,
    frame_poison, untouched; with `writes`: the part of it the launch stores to); returns the buffer as [blocks, cs, 8] on the host"""
    assert gb.guards_intact(), f"{c.id}/{cls}: wrote outside the output allocation"
    bits = gb.bits().view(pre.shape)
    bad = (bits != pre) & ~may
    assert not bool(bad.any()), f"{c.id}/{cls}: {int(bad.sum())} words the launch must not write changed (first at {bad.nonzero()[0].tolist()})"
    inner, inside = masks(g, guard, depth)
    if not frame_poison:
        fr = bits[:owned][:, (inside if writes is None else write_mask(g, writes, guard, depth)) & ~inner][..., :lanes]
        assert not bool(fr.any()), f"{c.id}/{cls}: {int((fr != 0).sum())} frame words are not exact zeros"
    return bits.view(torch.float32)


# ------------------------------------------------------------------ pack / unpack
def _special_imgs(shape, gen):
    t = torch.randn(shape, generator=gen)
    sp = torch.tensor(SPECIALS)
    flat = t.view(-1)
    k = min(flat.numel(), 4 * len(sp))
    flat[torch.randperm(flat.numel(), generator=gen)[:k]] = sp.repeat(4)[:k]
    return t


def run_pack(be, c):
    K = be.K
    gen = _gen(c, "special")
    g = K.geom(c.B, c.H, c.W)
    x = _special_imgs((c.B, c.cin, c.H, c.W), gen)
    if c.fmt in ("py", "dev"):
        sig = torch.tensor(0.0625) if c.fmt == "dev" else 0.0625
        smap = torch.full((c.B, 1, c.H, c.W), 0.0625)
        sig = be.dev(sig) if c.fmt == "dev" else sig
    elif c.fmt == "batch":
        sv = _special_imgs((c.B,), gen)
        sig, smap = be.dev(sv), sv.view(c.B, 1, 1, 1).expand(c.B, 1, c.H, c.W)
    else:
        smap = _special_imgs((c.B, 1, c.H, c.W), gen)
        sig = be.dev(smap)
    # contract: the launch writes all 8 channels of the first block at interior pixels (channels cin + 1 .. 7 as zeros) and nothing
    # else: the frame is UNTOUCHED (prefill PO2 on it), a second block is not its
    inner, inside = masks(g)
    pre = torch.full((2, g.cs, 8), PO2, dtype=torch.int32)
    may = torch.zeros((2, g.cs, 8), dtype=torch.bool)
    may[0, inner] = True
    gb = be.guarded(pre.numel(), be.dev(pre.view(torch.float32)))
    xg = be.guarded(x.numel(), be.dev(x))
    K.pack_input(g, xg.t.view(x.shape), sig, gb.t.view(2, g.cs, 8))
    be.sync()
    assert xg.guards_intact()
    out = check_out(c, "special", g, gb, pre, may, 1, frame_poison=True)
    want = torch.zeros(c.B, 8, c.H, c.W)
    want[:, :c.cin] = x
    want[:, c.cin:c.cin + 1] = smap
    got = from_buf(g, out[:1].contiguous())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{c.id}: {int((got.view(torch.int32) != want.view(torch.int32)).sum())} words differ"
    return 0.0


def run_unpack(be, c):
    K = be.K
    gen = _gen(c, "special")
    g = K.geom(c.B, c.H, c.W)
    x = _special_imgs((c.B, 8, c.H, c.W), gen)
    a = _nan_frame(g, to_buf(g, x, "nan"))            # contract: only interior pixels of the first block are read
    ag = be.guarded(a.numel(), be.dev(a))
    yg = be.guarded(c.B * c.cout * c.H * c.W)         # starts as POISON: every element must be written
    K.unpack_output(g, ag.t.view(a.shape), c.cout, yg.t.view(c.B, c.cout, c.H, c.W))
    be.sync()
    assert yg.guards_intact() and ag.guards_intact()
    got = yg.bits().view(c.B, c.cout, c.H, c.W)
    want = x[:, :c.cout].contiguous().view(torch.int32)
    assert torch.equal(got, want), f"{c.id}: {int((got != want).sum())} words differ"
    return 0.0


# ------------------------------------------------------------------ the convolutions
def _packs(be, c, w, bias):
    """(packed weight on the device, cin_p, cout_p, tile, packed bias)"""
    K = be.K
    k = c.kind
    pb = None
    if k == "direct":
        if c.tile == 16:
            pk, cin_p = K.pack_thin_weight(w)
            cout_p, tile = 16, 16
        elif c.tile == 0:                             # as production: conv_packs(...).pick(g)
            packs = K.conv_packs(w)
            pk = packs.pick(K.geom(c.B, c.H, c.W))
            cin_p, cout_p, tile = packs.cin_p, packs.cout_p, int(pk.shape[3])
        else:
            pk, cin_p, cout_p = K.pack_conv3x3_weight(w, mt=c.tile)
            tile = c.tile
        if bias is not None:
            pb = K.pack_bias(bias, cout_p)
        return be.dev(pk), cin_p, cout_p, tile, None if pb is None else be.dev(pb)
    fn = {"wino2": K.pack_winograd_weight, "wino4": K.pack_winograd4_weight, "wino4x3": K.pack_winograd4_bf16x3_weight,
          "split": K.pack_split2d_weight, "wsplit": K.pack_wsplit_weight, "tail": K.pack_tail_weight, "down": K.pack_down_weight,
          "down_bf16s": K.pack_down_bf16s_weight, "down_bf16x3": K.pack_down_bf16x3_weight, "up": K.pack_up_weight,
          "up_bf16s": K.pack_up_bf16s_weight}[k]
    if bias is not None:
        pb = be.dev(bias.float().contiguous() if k == "tail" else K.pack_bias(bias, c.cout))
    return be.dev(fn(w)), c.cin, c.cout, 0, pb


def _emu_log(be):
    """the launch log of the emulation since the last reset: [(spelling, instance x block)]"""
    if be.gpu:
        return None
    import emu_lib
    L = emu_lib.lib()
    log = [(L.dinv_emu_launch_log_name(i).decode(), L.dinv_emu_launch_log_instance(i).decode()) for i in range(L.dinv_emu_launch_log_count())]
    L.dinv_emu_launch_log_reset()
    return log


def pack_u_values(kind, pk):
    """the fp32 values of U that an uploaded F(4x4) pack holds, in fp64 (bf16x3: the sum of the three parts of every value, laid out
    [lane 64][um 4 | uh 4] then [lane 64][ul 4] per (wave, point))"""
    pk = pk.cpu()
    if kind == "wino4":
        return pk.double().reshape(-1)
    lead = pk.shape[:4]
    mh = pk[..., :512].reshape(*lead, 64, 2, 4).double()
    return (mh[..., 0, :] + mh[..., 1, :] + pk[..., 512:].reshape(*lead, 64, 4).double()).reshape(-1)


def _expected_launches(c, backend, tile):
    """the kernel instances a case's ONE library call must launch on the emulation, as the launch log names them (template
    arguments resolved where the launcher picks them at run time: rectangle, tile width, pixels per workgroup)"""
    relu, nres = c.has("relu"), int(c.has("res")) + int(c.has("res2"))
    t, f = "true", "false"
    if c.kind == "direct":
        b = ", true" if c.has("bias") else ""
        if tile == 16:
            return [f"(conv3_thin_kernel<{t if relu else f}, {nres}{b}>) x256"]
        return [f"(conv3x3_kernel<{tile // 32}, {t if relu else f}, {nres}{b}>) x256"]
    if c.kind in ("wino4", "wino4x3"):
        d = wino4_launch(c.B, c.H, c.W, c.cin, c.cout, CUS[backend], c.ws)
        one = "conv3x3_wino4_kernel<%d, %d, %s, %d, %%s, %s, %s> x512" % (d["rect"] + (t if relu else f, nres, t if c.kind == "wino4x3" else f,
                                                                                   t if c.has("bias") else f))
        return [one % f] * (d["full_x"] > 0) + [one % t] * (d["split_f"] > 1)
    if c.kind == "split":
        d = split_launch(c.B, c.H, c.W, c.cout, c.tile)
        return ["conv3x3_split2d_kernel<%s, %s, %s, %d, %d, %d> x256" % (t if c.fmt == "in_split" else f, t if c.fmt == "out_split" else f,
                                                                        t if relu else f, nres, d["tc"], d["nrep"])]
    if c.kind == "wsplit":
        return ["conv3x3_wsplit_kernel<%s, %d, %d> x256" % (t if relu else f, nres, wsplit_launch(c.B, c.H, c.W)["tc"])]
    if c.kind == "tail":
        d = tail_launch(c.B, c.H, c.W)
        return [f"(tail3x3_shift_kernel<{c.cout}, {d['rb']}, BR>) x256"]
    if c.kind == "down":
        return ["down2x2_kernel x256"]
    if c.kind == "down_bf16s":
        return ["(down2x2_bf16s_kernel<false, 2>) x256"]
    if c.kind == "down_bf16x3":
        return ["(down2x2_bf16s_kernel<false, 3>) x256"]
    if c.kind == "up":
        return ["up2x2_kernel x256"]
    return [f"up2x2_bf16s_kernel<{t if c.has('x2') else f}> x256"]


def run_conv(be, c, cls, beside=None):
    """one convolution case on one data class; returns (worst fraction of the ceiling, the bits of the interior)"""
    K, lib = be.K, be.lib()
    backend = "gpu" if be.gpu else "emu"
    d = data(c, cls)
    k = c.kind
    in_frame, writes = CONTRACT[k]
    B, H, W = c.B, c.H, c.W
    if k.startswith("down"):
        gi, go = K.geom(B, 2 * H, 2 * W), K.geom(B, H, W)
    elif k.startswith("up"):
        gi, go = K.geom(B, H, W), K.geom(B, 2 * H, 2 * W)
    else:
        gi = go = K.geom(B, H, W)
    hp, wp, plane, np_, sl, cs = geom_py(gi.batch, gi.height, gi.width)
    assert (gi.hp, gi.wp, gi.plane, gi.np, gi.sl, gi.cs) == (hp, wp, plane, np_, sl, cs), "the restated geometry is not the library's"
    pk, cin_p, cout_p, tile, pb = _packs(be, c, d["w"], d["bias"])
    xg = in_buf(be, gi, d["x"], in_frame, split=c.fmt == "in_split")
    x2g = in_buf(be, gi, d["x2"], in_frame) if d["x2"] is not None else None
    if k == "tail":
        owned, blocks, lanes = 1, 2, 4                # channels 4 .. 7 of the block and a second block are not the launch's
    else:
        owned = cdiv(c.cout, 8)                       # the direct kernel: cblocks_valid = ceil(cout_valid / 8) <= cout_p / 8
        blocks, lanes = owned + 1, 8
    # residuals: one buffer of `owned` blocks (tail_bias: the packed input image's first block), NaN frame and slack
    rg = [None if r_ is None else in_buf(be, go, r_, "nan") for r_ in (d["res1"], d["res2"])]
    yg, pre, may = out_buf(be, go, blocks, owned, writes, lanes)
    wsb = None
    if c.ws:
        wsb = be.guarded(lib.dinv_conv3x3_winograd4_workspace_bytes() // 4, torch.zeros(lib.dinv_conv3x3_winograd4_workspace_bytes() // 4))
    gb = ctypes.byref
    st = be.stream()
    P = lambda t_: None if t_ is None else _p(t_.t)   # noqa: E731
    relu = int(c.has("relu"))

    def call():
        if k == "direct" and c.has("bias"):
            return lib.dinv_conv3x3_bias(gb(gi), P(xg), _p(pk), _p(pb), cin_p, cout_p, c.cout, tile, P(yg), P(rg[0]), relu, st)
        if k == "direct":
            return lib.dinv_conv3x3(gb(gi), P(xg), P(x2g), _p(pk), cin_p, cout_p, c.cout, tile, P(yg), P(rg[0]), P(rg[1]), relu, st)
        if k == "wino2":
            return lib.dinv_conv3x3_winograd(gb(gi), P(xg), _p(pk), c.cin, c.cout, P(yg), P(rg[0]), relu, st)
        if k in ("wino4", "wino4x3"):
            wsz = ctypes.c_size_t(0 if wsb is None else 4 * wsb.n)
            if c.has("bias"):
                return lib.dinv_conv3x3_winograd4_bias(gb(gi), P(xg), _p(pk), _p(pb), c.cin, c.cout, P(yg), relu, P(wsb), wsz, st)
            fn = lib.dinv_conv3x3_winograd4 if k == "wino4" else lib.dinv_conv3x3_winograd4_bf16x3
            return fn(gb(gi), P(xg), _p(pk), c.cin, c.cout, P(yg), P(rg[0]), relu, P(wsb), wsz, st)
        if k == "split":
            flags = (1 if c.fmt == "in_split" else 0) | (2 if c.fmt == "out_split" else 0) | (4 if relu else 0) | (c.tile << 8)
            return lib.dinv_conv3x3_split(gb(gi), P(xg), _p(pk), c.cin, c.cout, P(yg), P(rg[0]), flags, st)
        if k == "wsplit":
            return lib.dinv_conv3x3_wsplit(gb(gi), P(xg), _p(pk), c.cin, c.cout, P(yg), P(rg[0]), 4 if relu else 0, st)
        if k == "tail" and c.has("bias"):
            return lib.dinv_conv3x3_tail_bias(gb(gi), P(xg), _p(pk), _p(pb), c.cin, c.cout, P(yg), P(rg[0]), st)
        if k == "tail":
            return lib.dinv_conv3x3_tail(gb(gi), P(xg), P(x2g), _p(pk), c.cin, c.cout, P(yg), st)
        if k == "down":
            return lib.dinv_conv_down2x2(gb(gi), gb(go), P(xg), _p(pk), c.cin, c.cout, P(yg), st)
        if k == "down_bf16s":
            return lib.dinv_conv_down2x2_bf16s(gb(gi), gb(go), P(xg), _p(pk), c.cin, c.cout, P(yg), st)
        if k == "down_bf16x3":
            return lib.dinv_conv_down2x2_bf16x3(gb(gi), gb(go), P(xg), _p(pk), c.cin, c.cout, P(yg), st)
        if k == "up":
            return lib.dinv_conv_up2x2(gb(gi), gb(go), P(xg), P(x2g), _p(pk), c.cin, c.cout, P(yg), st)
        return lib.dinv_conv_up2x2_bf16s(gb(gi), gb(go), P(xg), P(x2g), _p(pk), c.cin, c.cout, P(yg), st)

    _emu_log(be)
    if beside:
        beside()
    K.check(call())
    if beside:
        beside()
    be.sync()
    log = _emu_log(be)
    if log is not None:
        want = _expected_launches(c, backend, tile)
        assert [i for _, i in log] == want, f"{c.id}: launched {log}, the restated launcher says {want}"
    out_full = check_out(c, cls, go, yg, pre, may, owned, lanes)
    for gbuf in (xg, x2g, rg[0], rg[1], wsb):
        assert gbuf is None or gbuf.guards_intact()
    if k in ("wino4", "wino4x3"):
        f_, nt = K.winograd4_last_split()
        d4 = wino4_launch(B, H, W, c.cin, c.cout, CUS[backend], c.ws)
        assert (f_, nt) == (d4["split_f"], d4["ntail"]), f"{c.id}: the library split ({f_}, {nt}), the restatement says {d4}"
        if c.ws:                                      # the expected split of the table, per backend
            assert (f_, nt) == (c.split_gpu if be.gpu else c.split_emu), (c.id, f_, nt)
            first = out_full.clone()
            assert int(wsb.bits()[:8 * 64].abs().max()) == 0, f"{c.id}: ticket words are not zero after the launch"
            yg.t.copy_(be.dev(pre.view(torch.float32)).reshape(-1))     # launch again on the workspace the first launch left
            K.check(call())
            be.sync()
            out_full = check_out(c, cls, go, yg, pre, may, owned, lanes)
            assert int(wsb.bits()[:8 * 64].abs().max()) == 0, f"{c.id}: ticket words are not zero after the second launch"
            assert wsb.guards_intact()
            assert torch.equal(out_full.view(torch.int32), first.view(torch.int32)), f"{c.id}: the second launch gives other bits"
    got = out_full[:owned].contiguous()
    if c.fmt == "out_split":
        h = got.view(torch.bfloat16).view(owned, go.cs, 16)
        got = (h[..., :8].float() + h[..., 8:].float()).contiguous()
    out = from_buf(go, got)[:, :max(c.cout, lanes if k == "tail" else c.cout)]
    bits = out.contiguous().view(torch.int32).clone()
    if k == "tail":
        assert not bool(out[:, c.cout:4].view(torch.int32).any()), f"{c.id}: channels cout .. 3 are not exact zeros"
    elif c.cout % 8:                                  # padded couts of the last owned block: zero weights, exact zeros (+ residual pad 0)
        padv = from_buf(go, got)[:, c.cout:]
        assert not bool(padv.view(torch.int32).any()) or cls == "special", f"{c.id}: padded output channels are not exact zeros"
    out = out[:, :c.cout]
    ref, mag = d["ref"], d["mag"]
    assert not bool(torch.isnan(out).any()), f"{c.id}/{cls}: NaN in the interior (slack, frame or an unwritten element)"
    if c.fmt == "out_split":                          # the epilogue's split8 keeps 16 significant bits of the fp32 result
        ref_cmp = bf16_split(ref.float()).double() if cls != "randn" else ref
    else:
        ref_cmp = ref
    if cls == "special":
        assert bool((out.double() == ref_cmp).all()), f"{c.id}: fmaxf(NaN, 0) = 0 expected where the fp64 convolution is NaN; " \
            f"{int((out.double() != ref_cmp).sum())} elements differ"
        assert int(torch.isnan(_conv(c, d["x"].double(), d["w"].double())).sum()) > 0
        return 0.0, bits
    if cls != "randn":
        if k in ("wino4", "wino4x3"):
            uv = pack_u_values(k, pk)                 # r: measured on the pack that was uploaded
            r = float((uv - (uv * 64).round() / 64).abs().max())
            ceil = r * d["in_mag"]
            big = ref.abs() >= 1
            factor = 2.0 ** 24 * float(ceil[big].max()) / float(ref.abs().max()) if bool(big.any()) else 0.0
            err = (out.double() - ref_cmp).abs()
            worst = float((err / ceil.clamp_min(1e-300)).max())
            print(f"{c.id}/{cls}: r = {r:.3g}, largest ceiling {float(ceil.max()):.3g}, "
                  f"ceiling / one fp32 rounding = {factor:.3g}, worst / ceiling = {worst:.3g}")
            assert factor < 2.0 ** -10
            assert bool((err <= ceil).all()), f"{c.id}/{cls}: {int((err > ceil).sum())} elements off the lattice value, worst {float(err.max())}"
            return worst, bits
        bad = int((out.double() != ref_cmp).sum())
        assert bad == 0, f"{c.id}/{cls}: {bad} of {ref.numel()} elements differ from fp64, worst {float((out.double() - ref_cmp).abs().max())}"
        return 0.0, bits
    err = (out.double() - ref_cmp).abs()
    if k in BF16_KINDS or k in ("wino4x3", "down_bf16x3"):
        l2 = float((out.double() - ref_cmp).norm() / ref_cmp.norm())
        # the project's figures, relative to the convolution's magnitude sum: 3 * 2^-16 for the two-part split, 2^-22 for the
        # three-part one (2^-23 for the three dropped cross terms + 2 * 2^-24 for the two splits).  Then ONE rounding u x |value| for
        # each fp32 operation the case really has outside the products: the x + x2 add (carried through the products: u x conv_mag),
        # the bias add, each residual add - and 2^-18 x |value| for a pre-split output (hi = 8 bits, lo = 8 bits of the rest, round
        # to nearest each)
        cm = d["conv_mag"]
        bound = (2.0 ** -22 if k in ("wino4x3", "down_bf16x3") else 3 * 2.0 ** -16) * cm
        if k == "down_bf16x3":
            # no project figure per element: the kernel issues 6 products x 4 taps x cin / 16 MFMAs into one accumulator, which
            # is rounded once per instruction ("the accumulator is rounded once per 16-term MFMA and product", test_emu_drunet)
            bound = bound + gamma(6 * 4 * c.cin // 16) * cm
            assert l2 < 1e-6, f"{c.id}: relative l2 {l2:.3g}"
        after = cm
        if d["x2"] is not None:
            bound = bound + U * cm
        for t_ in (None if d["bias"] is None else d["bias"].double().abs()[None, :, None, None], d["res1"], d["res2"]):
            if t_ is not None:
                after = after + t_.double().abs()
                bound = bound + U * after
        if c.fmt == "out_split":
            bound = bound + 2.0 ** -18 * after
        assert l2 < SPLIT_L2, f"{c.id}: relative l2 {l2:.3g}"
    else:
        bound = gamma(chain(c, backend)) * mag
    ratio = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), f"{c.id}: worst |out - ref| / bound = {ratio:.3g}"
    return ratio, bits


def run_case(be, case, cls):
    """run one (case, class); prints and returns the worst fraction of the class's ceiling (0 for the bit-exact classes)"""
    if case.kind == "pack":
        ratio = run_pack(be, case)
    elif case.kind == "unpack":
        ratio = run_unpack(be, case)
    else:
        ratio = run_conv(be, case, cls)[0]
    print(f"{case.id}/{cls}: " + (f"worst / bound = {ratio:.3g}" if cls == "randn" else "exact"))
    return ratio
