"""Shared by tests/test_drunet3d_kernels_gpu.py (the gfx950 library) and tests/test_emu_drunet3d_cases.py (the same kernel sources on
the host emulation): one table of cases for the 3-D forms of the DRUNet kernels (models/drunet3d.py: a volume of D
slices is D + 2 images of the padded layout, a zero slice at each end, inside a buffer with one guard plane in front and behind) -
dinv_conv3x3x3, dinv_conv3x3x3_split, dinv_conv_down2x2_bf16s_3d, dinv_conv_up2x2_bf16s_3d - each case meant to reach one kernel
instance at one of its edges; the launchers' arithmetic restated (the table asserts what it reaches); the fp64 references
(F.conv3d / F.conv_transpose3d on the CPU); and one runner through the C entry points with the product's ctypes prototypes on guarded
buffers (fft_cases.Guarded).  The helpers are those of tests/bwd_cases.py and tests/drunet_fwd_cases.py, imported.

What the table reaches, per entry point, and what it knowingly does not:

  dinv_conv3x3x3        conv3x3_kernel<2, RELU, NRES> and <1, RELU, NRES> for RELU in {false, true}, NRES in {0, 1} with ndz = 3;
                        conv3_thin_kernel<RELU, NRES> for (false, 0), (true, 0), (false, 1), (true, 1) and the gate form (false, 2).
                        Launcher: one tile (np < 256), a ragged last tile, tiles_per_xcd = 1 with an idle slot, tiles_per_xcd = 2 with
                        7 of 16 slots idle, one to four cout tiles, cblocks_valid below the tile (5 of 8, 1 of 2), cin_p = 8 with 3
                        valid channels.  Slices: D = 1 (both depth neighbours are padding slices), volume boundaries inside a tile,
                        tiles across slices, plane > 256 (the tap shift exceeds the tile).
                        NOT reached: NRES = 2 of the wide kernel and x2 (the 3-D entry point passes neither), the BIAS instantiations
                        (2-D only: dinv_conv3x3_bias), a 32-wide pack of a 64-multiple layer (pack_conv3x3x3_weight never makes one).
  dinv_conv3x3x3_split  conv3x3_split2d_kernel<IN_SPLIT, OUT_SPLIT, RELU, NRES, TC, NREP> with ndz = 3: TC in {8, 16, 32} x NREP in
                        {1, 2}; (IN, OUT, RELU, NRES) = (f, f, f, 0), (f, f, t, 0), (f, f, f, 1), (f, f, f, 2: gate), (f, t, t, 0) and
                        (t, f, f, 1) - the last two chained as the inference ResBlock chains them.  Launcher: forced and automatic
                        pixels per workgroup (the automatic rule on both sides of n256 = 384: device only), a partial column tile, a
                        ragged last row tile, a row tile that holds the end of one volume, the whole leading padding slice of the
                        next and interior rows; nk = 3 (the prologue is the whole pipeline), 6 and 24.
                        NOT reached: (t, f, t, 0), (t, f, f, 0) and (f, t, f, 0) - no 3-D caller makes them (Ops3d pre-splits only the
                        ReLU temporary, and only the residual convolution reads it); they are reached in 2-D by drunet_fwd_cases.
  dinv_conv_down2x2_bf16s_3d   down2x2_bf16s_kernel<false, 2> (dz = 0, accumulate = 0) and <true, 2> (dz = 1, accumulate = 1, onto the
                        first tap's result and onto integers): depth_pair at D = 1, 2, 3, a 256-pixel tile across a slice, a padding
                        slice and a volume boundary.  NOT reached: the XCD walk beyond 8 workgroups per cout tile and NPL = 3 (both are
                        the 2-D table's: `9tiles`, down_bf16x3; the 3-D entry point has no three-part form).
  dinv_conv_up2x2_bf16s_3d     up2x2_bf16s_kernel<false> and <true> (x2, which Ops3d.up never passes), each depth tap alone and both;
                        np below and above one 128-pixel tile, a tile across a slice, a padding slice and a volume boundary.
  models/drunet3d.py    Ops3d.conv3 / down / up on every layer shape of the 16 / 32 / 64 / 128 network in three settings (PRODUCTION
                        below): which kernel runs, and whether the ReLU temporary travels pre-split.

Data classes (`Case.classes()`), as in drunet_fwd_cases: `int` (both operands, residuals and x2 in {-2 .. 2}: bit for bit, asserted
terms x 4 < 2^24 with terms = 27 cin or 8 cin), `wide-x` / `wide-w` (one operand m / 1024, |m| <= 4095: bit for bit while terms x 8190
< 2^24, i.e. cin <= 64 for the 3x3x3 kernels; the cin = 128 cases carry wide = False, asserted), `randn` (fp32 kernels: |out - ref| <=
gamma(27 cin_p + 2 + one per residual add) x the same operation on absolute values; bf16-split kernels: relative l2 < SPLIT_L2 and per
element 3 * 2^-16 x magnitude + u |value| per residual, accumulate or x2 add + 2^-18 |value| for a pre-split output) and `special` (ReLU
epilogues: NaN pre-activations under an input voxel of the first and of the last interior slice; fmaxf(NaN, 0) = +0 exactly at the
outputs of the fp64 convolution, and the footprint stops at the padding slice, which is written as zeros).  Gate epilogues draw their
activation from bwd_cases.special_act (+-0, denormals, +-Inf, NaN among N(0, 1) values).

Worst fraction of the randn ceiling per family on the MI355X (`-s` prints every run's): see BOUND_NOTES below.

Buffer contracts: CONTRACT below (read off the kernels).  Every call runs twice on fresh outputs and must give the same bits; operands
and guard bands are compared with their state before the call."""
import ctypes
import functools
import types
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from bwd_cases import (SPLIT_L2, U, Backend, _p, _vol, _vol_out, from_buf, gamma, imgs_vol,  # noqa: F401 (Backend: re-exported)
                       outside_interior_is_zero, special_act, to_buf, vol_imgs)
from drunet_fwd_cases import (_emu_log, _gen, _small, _wide, bf16_split, cdiv, check_out, direct_launch, geom_py, in_buf, masks,
                              out_buf, split_launch)

HOLD = 0x4B1D3D00                 # 10304768.0: the prefill of words inside [sl, sl + np) that a launch must leave alone (finite, recognisable)

# worst |out - ref| / ceiling of the randn class per family, from the MI355X run of tests/test_drunet3d_kernels_gpu.py (-s)
BOUND_NOTES = {
    "direct-wide": "gamma(27 cin_p + 2 + nres) x magnitude",                        # worst 0.0213 (direct-1x3x14x18-c8o128-plain)
    "direct-thin": "gamma(27 cin_p + 2 + nres) x magnitude",                        # worst 0.0147 (direct-1x3x14x18-c3o16-relu)
    "split": "3 * 2^-16 x magnitude (+ u per residual add, + 2^-18 pre-split)",     # worst 0.108 (split-127x1x2x32-c16o128-res-f32-n0)
    "down": "3 * 2^-16 x magnitude (+ u for the accumulate)",                       # worst 0.0969 (down-2x2x7x9-c16o128-plain)
    "up": "3 * 2^-16 x magnitude (+ u for x2)",                                     # worst 0.222 (up-2x2x7x5-c16o64-plain)
}


def r16(c):
    return cdiv(c, 16) * 16


def r64(c):
    return cdiv(c, 64) * 64


# ------------------------------------------------------------------ the geometry and the launchers, restated
def level_py(V, D, H, W):
    """models/drunet3d.py Level: V (D + 2) images, one guard plane in front, cs enlarged by two planes"""
    images = V * (D + 2)
    hp, wp, plane, np_, sl, cs = geom_py(images, H, W)
    return dict(images=images, hp=hp, wp=wp, plane=plane, np=np_, sl=sl, cs=(cs + 2 * plane + 3) // 4 * 4, guard=plane)


def direct_pack(cout):
    """pack_conv3x3x3_weight: (cout_p, cout tile) - the thin pack up to 16 outputs, 64-wide tiles where cout_p is a multiple of 64"""
    if cout <= 16:
        return 16, 16
    cout_p = cdiv(cout, 32) * 32
    return cout_p, 64 if cout_p % 64 == 0 else 32


def tile_straddles(V, D, plane, tile):
    """some `tile`-pixel tile of the flattened V (D + 2) plane pixels holds pixels of an interior slice, pixels of a padding slice and
    the first pixel of a later volume with its predecessor"""
    np_ = V * (D + 2) * plane
    for t in range(cdiv(np_, tile)):
        lo, hi = t * tile, min((t + 1) * tile, np_)
        z = {i % (D + 2) for i in range(lo // plane, (hi - 1) // plane + 1)}
        if any(1 <= s <= D for s in z) and (0 in z or D + 1 in z) and any(lo < v * (D + 2) * plane < hi for v in range(1, V)):
            return True
    return False


def pad_slice_in_row_tile(V, D, H, tr):
    """some row tile of the 2-D tiles holds the last frame row of a volume's trailing padding slice, the whole leading padding slice
    of the next volume and interior rows of that volume's first slice"""
    hp = H + 2
    rows = V * (D + 2) * hp
    for t in range(cdiv(rows, tr)):
        lo, hi = t * tr, min((t + 1) * tr, rows)
        for v in range(1, V):
            b = v * (D + 2) * hp                       # first row of the leading padding slice of volume v
            if lo <= b - 1 and hi >= b + hp + 2:        # ... row b + hp is the frame row of its first slice, b + hp + 1 is interior
                return True
    return False


# ------------------------------------------------------------------ contracts (read off the kernels)
# in_frame: what the frame and BOTH PADDING SLICES of x (and x2) hold.
#   "zero"  required: they are the convolution's padding.  conv3x3_kernel / conv3_thin_kernel (drunet.hip) and conv3x3_split2d_kernel
#           read them as the operands of the taps that leave the volume.
#   "nan"   never read by a stored output: the stride-2 kernels pair interior pixels of interior slices with interior pixels of
#           interior slices (depth_pair returns -1 for a padding slice; such lanes, border lanes and lanes past np read pixel `sl` and
#           are not stored / replaced by a select).
# Guard planes, slack and everything else outside [sl, sl + np) are NaN in EVERY input, residuals and gates included, and so are the
# frames and padding slices of residuals and gates: an MFMA column is one output pixel, so a NaN operand reaches only outputs whose
# footprint holds it, and every output at a frame pixel or in a padding slice - the only ones whose footprint reaches a guard plane
# (depth tap dz = 0 of slice 0, dz = 2 of slice D + 1) or whose residual is NaN - is replaced by a SELECT (`if (!in) v = 0`,
# writes_value()), not multiplied by zero.  No 3-D kernel needs zeros in a guard plane; the launchers only need the planes to be
# readable memory (the cs checks of dinv_conv3x3x3 and split_launch).
# writes:   "all"      every pixel below np of the blocks the launch owns, frames and padding slices as exact zeros (select);
#           "rows"     columns 1 .. W of every row, frame rows and padding slices as zeros, frame columns untouched (2-D tiles);
#           "interior" up: tap dz stores the interior pixels of the slices 2 z + dz + 1 (z = 0 .. D - 1) and nothing else - frames,
#                      padding slices and the slices of the other tap keep their bits.
# Nothing is stored outside [sl, sl + np), into a guard plane or into a channel block past the owned ones (direct: past
# cblocks_valid = ceil(cout_valid / 8); split / down / up: past cout_p / 8).
CONTRACT = {"direct": ("zero", "all"), "split": ("zero", "rows"), "down": ("nan", "all"), "up": ("nan", "interior")}
C3_KINDS = ("direct", "split")


# ------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    id: str
    kind: str                     # direct | split | pair | down | up
    V: int = 1                    # volumes
    D: int = 1                    # slices per volume; stride-2 kinds: of the HALF grid (down: output, up: input), as H and W
    H: int = 1
    W: int = 1
    cin: int = 16                 # real channels (direct pads to 8 / 32 or 16, the bf16-split kernels to 16 / 64 as Ops3d does)
    cout: int = 64
    mode: str = "plain"           # '+'-joined: relu, res, gate, x2
    tile: int = 0                 # split / pair: bits 8-9 of flags (0 = automatic)
    fmt: str = "f32"              # split: f32 | in_split | out_split;  pair: presplit | direct (which kernels, how the temporary travels)
    expect: tuple = ()            # what the case must reach (asserted from the restated arithmetic in _check_table)
    gpu_only: bool = False
    gpu_only_classes: tuple = ()
    wide: bool = True
    special: bool = False
    note: str = ""

    def has(self, tok):
        return tok in self.mode.split("+")

    def classes(self):
        c = ["int"] + (["wide-x", "wide-w"] if self.wide else []) + ["randn"]
        return tuple(c + (["special"] if self.special else []))


CASES = []
NO_WIDE_128 = "wide = False: 27 x 128 terms x 8190 = 1.69 x 2^24 quanta of 1/1024; cin = 16, 32 and 64 carry the class"


def _add(**kw):
    CASES.append(Case(**kw))


# ---- 1. dinv_conv3x3x3: conv3x3_kernel<MREP, RELU, NRES> with ndz = 3, conv3_thin_kernel<RELU, NRES>
G1 = (1, 1, 2, 2)                 # np = 48: one tile; both depth neighbours of the only slice are padding slices
G2 = (3, 1, 2, 2)                 # np = 144: slices 0, 1, 2, 0, 1, 2, ... inside one tile
G3 = (2, 2, 4, 8)                 # plane = 72, np = 576: tiles across slices and across the volume boundary
G4 = (1, 3, 14, 18)               # plane = 320 > 256, np = 1600: 7 tiles, the last ragged, tiles_per_xcd = 1, one idle slot
G5 = (1, 5, 14, 18)               # np = 2240: 9 tiles, tiles_per_xcd = 2, 7 of 16 slots return early
GEXP = {G1: ("np<256", "D1"), G2: ("np<256", "D1", "volumes-in-tile"), G3: ("straddles",), G4: ("plane>256", "ragged", "tpx1-idle"),
        G5: ("plane>256", "9tiles")}


_SLOW = ("wide-x", "wide-w")       # the wide kernel on 7 and 9 tiles takes the fiber emulation 6 - 9 s a run: `int` and `randn` there


def _d(geo, cin, cout, mode, expect=(), **kw):
    V, D, H, W = geo
    if geo in (G4, G5) and cout > 16:
        kw.setdefault("gpu_only_classes", _SLOW)
    _add(id=f"direct-{V}x{D}x{H}x{W}-c{cin}o{cout}-{mode}", kind="direct", V=V, D=D, H=H, W=W, cin=cin, cout=cout, mode=mode,
         expect=GEXP[geo] + expect, **kw)


_d(G1, 16, 64, "plain", ("mrep2",))
_d(G2, 16, 64, "relu", ("mrep2",))
_d(G3, 16, 64, "res", ("mrep2",))
_d(G3, 8, 128, "relu+res", ("mrep2", "ytiles2"))
_d(G4, 8, 128, "plain", ("mrep2", "ytiles2"))
_d(G4, 16, 64, "relu+res", ("mrep2",))
_d(G5, 8, 128, "res", ("mrep2", "ytiles2"))
_d(G5, 16, 64, "relu", ("mrep2",), special=True)
_d(G3, 24, 40, "relu", ("mrep2", "cbv5of8"))                # cout_valid = 40 of 64: blocks 5 .. 7 are never written
_d(G4, 24, 40, "res", ("mrep2", "cbv5of8"))
_d(G1, 16, 32, "relu", ("mrep1",))                          # the 32-wide tile: cout_p = 32 and 96
_d(G2, 16, 32, "res", ("mrep1",))
_d(G3, 16, 96, "relu+res", ("mrep1", "ytiles3"))
_d(G4, 16, 32, "plain", ("mrep1",))
_d(G5, 16, 96, "plain", ("mrep1", "ytiles3"))
_d(G3, 16, 16, "relu", ("thin",), special=True)
_d(G5, 16, 16, "relu", ("thin",))
_d(G2, 16, 16, "relu+res", ("thin",))
_d(G4, 16, 16, "relu+res", ("thin",))
_d(G3, 3, 16, "relu", ("thin", "head"))                     # the head: 3 valid channels of cin_p = 8
_d(G4, 3, 16, "relu", ("thin", "head"))
_d(G1, 16, 2, "plain", ("thin", "cbv1of2"))                 # the tail: cout_valid = 2
_d(G4, 16, 2, "plain", ("thin", "cbv1of2"))
_d(G3, 16, 2, "res", ("thin", "cbv1of2"))
_d(G5, 16, 2, "res", ("thin", "cbv1of2"))
_d(G1, 8, 8, "plain", ("thin", "cbv1of2"))                  # a whole block and not one more
_d(G3, 8, 8, "plain", ("thin", "cbv1of2"))
_d(G4, 16, 16, "gate", ("thin",))


# ---- 2. dinv_conv3x3x3_split: the 2-D tiles with ndz = 3 (flag bits 8-9 through ctypes)
def _s(geo, cin, cout, mode, fmt, tile, expect=(), **kw):
    V, D, H, W = geo
    _add(id=f"split-{V}x{D}x{H}x{W}-c{cin}o{cout}-{mode}-{fmt}-n{tile}", kind="split", V=V, D=D, H=H, W=W, cin=cin, cout=cout, mode=mode,
         fmt=fmt, tile=tile, expect=expect, **kw)


_s((1, 1, 4, 8), 16, 64, "plain", "f32", 1, ("tc8", "tr16", "ragged-row", "nk3", "D1"))       # V = 1, D = 1: 18 rows against 16
_s((2, 1, 4, 8), 16, 64, "relu", "f32", 1, ("tc8", "tr16", "pad-slice-in-tile", "nk3"), special=True)
_s((2, 1, 4, 8), 32, 64, "res", "f32", 2, ("tc8", "tr32", "pad-slice-in-tile", "nk6"))
_s((2, 1, 4, 16), 32, 128, "gate", "f32", 2, ("tc16", "tr16", "pad-slice-in-tile", "ytiles2"))
_s((2, 1, 4, 16), 16, 64, "plain", "f32", 1, ("tc16", "tr8", "ragged-row"))
_s((1, 2, 4, 32), 16, 64, "relu", "f32", 1, ("tc32", "tr4"))
_s((1, 2, 4, 32), 128, 64, "res", "f32", 2, ("tc32", "tr8", "nk24"), wide=False, note=NO_WIDE_128)
_s((1, 2, 3, 12), 32, 128, "plain", "f32", 1, ("tc8", "partial-col", "ragged-row"))
_s((1, 2, 3, 12), 16, 64, "gate", "f32", 2, ("tc8", "tr32", "partial-col", "ragged-row"))
_s((1, 3, 5, 8), 128, 128, "relu", "f32", 0, ("tc8", "auto1", "nk24", "ytiles2"), wide=False, note=NO_WIDE_128)
_s((2, 2, 4, 8), 16, 64, "relu", "out_split", 1, ("tc8",))                       # the two halves of the ResBlock pair on their own
_s((2, 2, 4, 8), 32, 64, "res", "in_split", 2, ("tc8",))
# one automatic case on each side of n256 = 384 (W = 32: 8 rows per 256 pixels; 381 / 384 images of 4 rows, two cout tiles)
_s((127, 1, 2, 32), 16, 128, "res", "f32", 0, ("tc32", "auto1", "n256=382"), gpu_only=True)
_s((128, 1, 2, 32), 16, 128, "res", "f32", 0, ("tc32", "auto2", "n256=384"), gpu_only=True)
# the inference ResBlock as production chains it: relu + y_presplit into a temporary, the temporary as x_presplit into res
PAIR_NOTE = "wide = False: the temporary of 12-bit data needs more than the 16 bits a pre-split value holds"
_add(id="pair-2x2x4x8-c64-presplit-n1", kind="pair", V=2, D=2, H=4, W=8, cin=64, cout=64, fmt="presplit", tile=1, expect=("tc8",),
     wide=False, note=PAIR_NOTE)
_add(id="pair-1x2x4x16-c64-presplit-n0", kind="pair", V=1, D=2, H=4, W=16, cin=64, cout=64, fmt="presplit", tile=0, expect=("tc16", "auto1"),
     wide=False, note=PAIR_NOTE)


# ---- 3. dinv_conv_down2x2_bf16s_3d / dinv_conv_up2x2_bf16s_3d on the HALF grid V x D x H x W
def _st(kind, geo, cin, cout, mode="plain", expect=(), **kw):
    V, D, H, W = geo
    _add(id=f"{kind}-{V}x{D}x{H}x{W}-c{cin}o{cout}-{mode}", kind=kind, V=V, D=D, H=H, W=W, cin=cin, cout=cout, mode=mode, expect=expect, **kw)


_st("down", (2, 1, 2, 4), 16, 64, expect=("D1", "one-tile"))
_st("down", (1, 3, 5, 6), 64, 128)
_st("down", (2, 2, 7, 9), 16, 128, expect=("straddles",))
_st("down", (2, 2, 7, 9), 64, 64, expect=("straddles",))
_st("up", (2, 1, 2, 4), 64, 64, "x2", ("D1",))
_st("up", (1, 3, 5, 6), 16, 128)
# (7 x 9 has plane = 108: no 128-pixel tile of two volumes holds a whole padding slice, the boundary and a slice; 7 x 5 - plane 72 - does)
_st("up", (2, 2, 7, 5), 64, 128, "x2", ("straddles",))
_st("up", (2, 2, 7, 5), 16, 64, "plain", ("straddles",))
_st("up", (2, 2, 7, 9), 16, 64, "x2")

assert len({c.id for c in CASES}) == len(CASES)
BY_ID = {c.id: c for c in CASES}


def reached(c):
    """what case c reaches, from the restated launcher arithmetic: a set of regime names"""
    lp = level_py(c.V, c.D, c.H, c.W)
    r = {"D1"} if c.D == 1 else set()
    if c.kind == "direct":
        cout_p, tile = direct_pack(c.cout)
        d = direct_launch(lp["np"], cout_p, tile)
        r |= {"thin" if tile == 16 else f"mrep{tile // 32}", f"ytiles{d['ytiles']}"}
        if lp["np"] < 256:
            r.add("np<256")
            if c.V >= 2:
                r.add("volumes-in-tile")
        if lp["np"] > 256 and lp["np"] % 256:
            r.add("ragged")
        if lp["plane"] > 256:
            r.add("plane>256")
        if lp["plane"] < 256 and tile_straddles(c.V, c.D, lp["plane"], 256):
            r.add("straddles")
        if d["tpx"] == 1 and d["idle"] == d["ytiles"]:
            r.add("tpx1-idle")
        if d["ntiles"] == 9 and d["tpx"] == 2 and d["idle"] == 7 * d["ytiles"]:
            r.add("9tiles")
        if c.cin % 8:
            r.add("head")
        if cdiv(c.cout, 8) < cout_p // 8:
            r.add(f"cbv{cdiv(c.cout, 8)}of{cout_p // 8}")
    elif c.kind in ("split", "pair"):
        d = split_launch(lp["images"], c.H, c.W, r64(c.cout), c.tile)
        r |= {f"tc{d['tc']}", f"tr{d['tr']}", f"n256={d['n256']}", f"nk{3 * r16(c.cin) // 16}", f"ytiles{r64(c.cout) // 64}"}
        if d["partial_col"]:
            r.add("partial-col")
        if d["ragged_row"]:
            r.add("ragged-row")
        if not c.tile:
            r.add(f"auto{d['nrep']}")
        if pad_slice_in_row_tile(c.V, c.D, c.H, d["tr"]):
            r.add("pad-slice-in-tile")
    else:
        tile = 256 if c.kind == "down" else 128       # down: 256 output pixels, up: 128 input pixels - both of the half grid
        if lp["np"] <= tile:
            r.add("one-tile")
        if tile_straddles(c.V, c.D, lp["plane"], tile):
            r.add("straddles")
    return r


def terms(c):
    return (27 if c.kind in C3_KINDS + ("pair",) else 8) * c.cin


def _check_table():
    """every case reaches what its `expect` says; the exactness conditions of the classes a case runs hold; wide = False exactly where
    the condition fails (and the case says why)"""
    for c in CASES:
        got = reached(c)
        for e in c.expect:
            assert e in got, (c.id, e, got)
        extra = 2 * (c.has("res") + c.has("x2")) + (3 if c.kind == "down" else 0)       # residual / prefill of the accumulate
        assert (terms(c) * 4 * (2 if c.has("x2") else 1) + extra) < 2 ** 24, c.id
        fits = (terms(c) * 8190 * (2 if c.has("x2") else 1) + extra * 1024) < 2 ** 24
        if c.kind == "pair":
            assert not c.wide and c.note
        else:
            assert c.wide == fits and (c.wide or c.note), (c.id, fits)
        assert lp_pixels(c) <= (4096 if not c.gpu_only else 65536) and max(c.cin, c.cout) <= 128, c.id


def lp_pixels(c):
    return level_py(c.V, c.D, c.H, c.W)["np"] * (4 if c.kind in ("down", "up") else 1)


_check_table()
# the two geometry facts of section 3 that the shapes were chosen for, spelled out
assert tile_straddles(2, 2, 9 * 12, 256) and not tile_straddles(2, 2, 9 * 12, 128) and tile_straddles(2, 2, 9 * 8, 128)


def items(emu):
    out = []
    for c in CASES:
        if emu and c.gpu_only:
            continue
        out += [(c, k) for k in c.classes() if not (emu and k in c.gpu_only_classes)]
    return out


def item_id(v):
    return v.id if isinstance(v, Case) else str(v)


# ------------------------------------------------------------------ data and references
def _shapes(c):
    """(x, w, out) shapes"""
    V, D, H, W = c.V, c.D, c.H, c.W
    if c.kind in C3_KINDS:
        return (V, c.cin, D, H, W), (c.cout, c.cin, 3, 3, 3), (V, c.cout, D, H, W)
    if c.kind == "down":
        return (V, c.cin, 2 * D, 2 * H, 2 * W), (c.cout, c.cin, 2, 2, 2), (V, c.cout, D, H, W)
    return (V, c.cin, D, H, W), (c.cin, c.cout, 2, 2, 2), (V, c.cout, 2 * D, 2 * H, 2 * W)


def _conv(c, x, w):
    if c.kind in C3_KINDS:
        return F.conv3d(x, w, padding=1)
    if c.kind == "down":
        return F.conv3d(x, w, stride=2)
    return F.conv_transpose3d(x, w, stride=2)


def _one_tap(w, dz):
    """the filter with the other depth tap zeroed"""
    w = w.clone()
    w[:, :, 1 - dz] = 0
    return w


def make(c, cls, x=None, res=None):
    """operands, the fp64 reference, the magnitude sums and the asserted exactness preconditions of one (case, class).  x / res: given
    instead of drawn (the second half of a pair reads the first half's output and adds the block's input)"""
    gen = _gen(c, cls)
    xs, wsh, osh = _shapes(c)
    fed = x is not None
    exact = cls != "randn"
    if cls in ("int", "special"):
        x0, w = _small(xs, gen), _small(wsh, gen)
    elif cls == "wide-x":
        x0, w = _wide(xs, gen), _small(wsh, gen)
    elif cls == "wide-w":
        x0, w = _small(xs, gen), _wide(wsh, gen)
    else:
        x0, w = torch.randn(xs, generator=gen), torch.randn(wsh, generator=gen) / terms(c) ** 0.5
    x = x0 if x is None else x
    draw = (lambda s: _small(s, gen)) if exact else (lambda s: torch.randn(s, generator=gen))
    x2 = (_wide(xs, gen) if cls == "wide-x" else draw(xs)) if c.has("x2") else None
    if res is None and c.has("res"):
        res = draw(osh)
    act = special_act(int(torch.tensor(osh).prod()), gen).view(osh) if c.has("gate") else None
    prefill = None
    if c.kind == "down":
        prefill = torch.randint(-3, 4, osh, generator=gen).float() if exact else torch.randn(osh, generator=gen)
    if c.fmt == "in_split" and not exact and not fed:
        x = bf16_split(x)                             # the operand the kernel really sees (exact classes: 12 bits fit two parts)
    if cls == "special":                              # a NaN under an input voxel of the first and of the last interior slice
        x = x.clone()
        x[0, :, 0, 0, 0] = float("nan")
        x[-1, 0, -1, -1, -1] = float("nan")
    x64 = x.double() if x2 is None else x.double() + x2.double()
    xa = x.double().abs() if x2 is None else x.double().abs() + x2.double().abs()
    w64 = w.double()
    ref, cm = _conv(c, x64, w64), _conv(c, xa, w64.abs())
    d = dict(x=x, x2=x2, w=w, res=res, act=act, prefill=prefill)
    if c.kind == "down":
        d["ref_tap"] = [_conv(c, x64, _one_tap(w64, dz)) for dz in range(2)]
        d["mag_tap"] = [_conv(c, xa, _one_tap(w64, dz).abs()) for dz in range(2)]
    if cls == "special":
        assert int(torch.isnan(ref).sum()) > 0 and not bool(torch.isnan(ref).all())
        cm = torch.nan_to_num(cm, nan=0.0)
    mag = cm
    if c.has("relu"):
        ref = ref.relu() if cls != "special" else torch.where(torch.isnan(ref), torch.zeros_like(ref), ref.relu())
    if res is not None:
        ref, mag = ref + res.double(), mag + res.double().abs()
    if act is not None:
        ref = torch.where(act > 0, ref, torch.zeros_like(ref))
    d.update(ref=ref, mag=mag, conv_mag=cm)
    # ---- exactness preconditions: asserted, not assumed
    if exact and cls != "special":
        quantum = 1 if cls == "int" else 1024
        big = mag if prefill is None else mag + 3
        assert float(big.max()) * quantum < 2 ** 24, (c.id, cls, float(big.max()) * quantum / 2 ** 24)
        if not fed:                                   # the sufficient condition of the table, in its own words
            prod = (4 if cls == "int" else 8190 / 1024) * (2 if x2 is not None else 1)
            assert (terms(c) * prod + 2 * (res is not None) + (3 if prefill is not None else 0)) * quantum < 2 ** 24, c.id
    return d


@functools.lru_cache(maxsize=2)
def data(c, cls):
    """make(c, cls), computed once, shared by the tests that need it, never modified"""
    return make(c, cls)


# ------------------------------------------------------------------ comparing
def _bits(t):
    return t.contiguous().view(torch.int32)


def compare(tag, cls, out, ref, bound=None, l2=False):
    """exact classes: out equals the fp64 reference bit for bit (as values: a zero of either sign is a zero); randn: |out - ref| <=
    bound per element (and, l2, relative l2 < SPLIT_L2).  Returns the worst fraction of the bound"""
    assert out.shape == ref.shape, (tag, out.shape, ref.shape)
    assert not bool(torch.isnan(out).any()), f"{tag}/{cls}: NaN in the interior (slack, guard plane, frame or an unwritten element)"
    if cls != "randn":
        bad = int((out.double() != ref).sum())
        assert bad == 0, f"{tag}/{cls}: {bad} of {ref.numel()} elements differ from fp64, worst {float((out.double() - ref).abs().max())}"
        return 0.0
    if l2:
        rel = float((out.double() - ref).norm() / ref.norm())
        assert rel < SPLIT_L2, f"{tag}: relative l2 {rel:.3g}"
    err = (out.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), f"{tag}: worst |out - ref| / bound = {ratio:.3g}"
    return ratio


def split_bound(cm, adds=(), x2=False, presplit=False):
    """the project's per-element figure of the bf16-split kernels: 3 * 2^-16 x the convolution's magnitude sum, one rounding u x
    |value| for the x + x2 add (carried through the products) and for each add behind the products, 2^-18 x |value| for a pre-split
    output"""
    bound, after = 3 * 2.0 ** -16 * cm, cm
    if x2:
        bound = bound + U * cm
    for t in adds:
        after = after + t.double().abs()
        bound = bound + U * after
    if presplit:
        bound = bound + 2.0 ** -18 * after
    return bound


def _padc(t, channels):
    """zero channels behind dim 1 up to `channels`"""
    return t if t.shape[1] == channels else F.pad(t, (0, 0) * (t.ndim - 2) + (0, channels - t.shape[1]))


def _padw(w, a, b):
    """zero filters / channels up to [a, b, ...] (what Ops3d hands the bf16-split kernels)"""
    out = torch.zeros((a, b) + tuple(w.shape[2:]))
    out[:w.shape[0], :w.shape[1]] = w
    return out


def level(c_or_geo, scale=1):
    from deepinv_amd.models.drunet3d import Level
    V, D, H, W = (c_or_geo.V, c_or_geo.D, c_or_geo.H, c_or_geo.W) if isinstance(c_or_geo, Case) else c_or_geo
    lv = Level(V, scale * D, scale * H, scale * W)
    lp = level_py(V, scale * D, scale * H, scale * W)
    g = lv.g
    assert (g.batch, g.hp, g.wp, g.plane, g.np, g.sl, g.cs, lv.guard) == tuple(lp[k] for k in ("images", "hp", "wp", "plane", "np", "sl", "cs", "guard")), \
        "the restated geometry is not the library's"
    return lv


def decode(buf, presplit):
    """[blocks, cs, 8] fp32 words -> values (pre-split: high part + low part)"""
    if not presplit:
        return buf
    h = buf.contiguous().view(torch.bfloat16).view(buf.shape[0], buf.shape[1], 16)
    return (h[..., :8].float() + h[..., 8:].float()).contiguous()


def _weights(be, pk):
    """a packed weight (fp32, or bf16 pairs) inside a Guarded buffer on the backend's device"""
    words = pk if pk.dtype == torch.float32 else pk.contiguous().view(torch.int16).view(torch.float32)
    return be.guarded(words.numel(), be.dev(words))


def _snapshot(bufs):
    return [None if b is None else b.full.clone() for b in bufs]


def _unchanged(tag, bufs, snap):
    for b, s in zip(bufs, snap):
        assert b is None or torch.equal(b.full, s), f"{tag}: an operand (or its guard band) changed"


def _volume(lv, buf, V, channels, cls, tag):
    """interior [V, channels, D, H, W] of the owned blocks `buf`; the padded channels behind `channels` are exact zeros"""
    vol, _ = imgs_vol(from_buf(lv.g, buf, lv.guard), V)
    if vol.shape[1] > channels and cls != "special":
        assert not bool(_bits(vol[:, channels:]).any()), f"{tag}: padded output channels are not exact zeros"
    return vol[:, :channels].contiguous()


# ------------------------------------------------------------------ what a call must launch (the emulation's launch log)
def expected_launches(c):
    t, f = "true", "false"
    b = lambda v: t if v else f                       # noqa: E731
    if c.kind == "direct":
        nres = 2 if c.has("gate") else int(c.has("res"))
        _, tile = direct_pack(c.cout)
        if tile == 16:
            return [f"(conv3_thin_kernel<{b(c.has('relu'))}, {nres}>) x256"]
        return [f"(conv3x3_kernel<{tile // 32}, {b(c.has('relu'))}, {nres}>) x256"]
    if c.kind == "split":
        d = split_launch(level_py(c.V, c.D, c.H, c.W)["images"], c.H, c.W, r64(c.cout), c.tile)
        nres = 2 if c.has("gate") else int(c.has("res"))
        return ["conv3x3_split2d_kernel<%s, %s, %s, %d, %d, %d> x256" % (b(c.fmt == "in_split"), b(c.fmt == "out_split"), b(c.has("relu")),
                                                                        nres, d["tc"], d["nrep"])]
    if c.kind == "pair":
        return [i for h in pair_halves(c) for i in expected_launches(h)]
    if c.kind == "down":
        return ["(down2x2_bf16s_kernel<false, 2>) x256", "(down2x2_bf16s_kernel<true, 2>) x256"]
    return [f"up2x2_bf16s_kernel<{b(c.has('x2'))}> x256"] * 2


def _check_log(be, tag, want):
    log = _emu_log(be)
    if log is not None:
        assert [i for _, i in log] == want, f"{tag}: launched {log}, the restated launcher says {want}"


# ------------------------------------------------------------------ 3x3x3: dinv_conv3x3x3 / dinv_conv3x3x3_split
def run_c3(be, c, cls, feed=None, hold=HOLD):
    """one 3x3x3 case on one data class, twice on fresh outputs.  feed = (Guarded input buffer, its values [V, cin, D, H, W], the
    residual): the second half of a pair.  Returns (worst fraction of the ceiling, bits of the interior [V, cout, D, H, W], the output
    buffer of the second run, the data)"""
    K, lib = be.K, be.lib()
    lv = level(c)
    g, guard = lv.g, lv.guard
    d = data(c, cls) if feed is None else make(c, cls, x=feed[1], res=feed[2])
    writes = CONTRACT[c.kind][1]
    if c.kind == "direct":
        pk, cin_p, cout_p = K.pack_conv3x3x3_weight(d["w"])
        tile = int(pk.shape[4])
        assert (cout_p, tile) == direct_pack(c.cout)
        owned = cdiv(c.cout, 8)                       # cblocks_valid
        nblk, rch = max(owned, cout_p // 8) + 1, owned * 8
    else:
        cin_p, cout_p, tile = r16(c.cin), r64(c.cout), 0
        pk = K.pack_split3d_weight(_padw(d["w"], cout_p, cin_p))
        owned = cout_p // 8
        nblk, rch = owned + 1, cout_p
    xg = feed[0] if feed else in_buf(be, g, _padc(vol_imgs(d["x"]), cin_p), "zero", split=c.fmt == "in_split", guard=guard, depth=c.D)
    r_ = d["act"] if c.has("gate") else d["res"]
    rg = None if r_ is None else in_buf(be, g, _padc(vol_imgs(r_), rch), "nan", guard=guard, depth=c.D)
    wg = _weights(be, pk)
    relu, gate = int(c.has("relu")), int(c.has("gate"))
    st = be.stream()
    P = lambda t_: None if t_ is None else _p(t_.t, guard * 8)      # noqa: E731  (views whose first plane is the leading padding slice)
    ops = (xg, rg, wg)
    runs = []
    for _ in range(2):
        yg, pre, may = out_buf(be, g, nblk, owned, writes, 8, guard, c.D, hold)
        snap = _snapshot(ops)
        _emu_log(be)
        if c.kind == "direct":
            rc = lib.dinv_conv3x3x3(ctypes.byref(g), P(xg), _p(wg.t), cin_p, cout_p, c.cout, tile, P(yg), P(rg), relu | 2 * gate, c.D, st)
        else:
            flags = (1 if c.fmt == "in_split" else 0) | (2 if c.fmt == "out_split" else 0) | 4 * relu | 8 * gate | (c.tile << 8)
            rc = lib.dinv_conv3x3x3_split(ctypes.byref(g), P(xg), _p(wg.t), cin_p, cout_p, P(yg), P(rg), flags, c.D, st)
        K.check(rc)
        be.sync()
        _check_log(be, c.id, expected_launches(c))
        full = check_out(c, cls, g, yg, pre, may, owned, 8, guard=guard, depth=c.D, writes=writes)
        _unchanged(c.id, ops, snap)
        runs.append(full)
    assert torch.equal(_bits(runs[0]), _bits(runs[1])), f"{c.id}/{cls}: the second call gives other bits"
    out = _volume(lv, decode(runs[0][:owned].contiguous(), c.fmt == "out_split"), c.V, c.cout, cls, c.id)
    ref = d["ref"]
    if c.fmt == "out_split" and cls != "randn":       # the epilogue's split8 keeps 16 significant bits of the fp32 result
        ref = bf16_split(ref.float()).double()
    if cls == "special":
        assert bool((out.double() == ref).all()), f"{c.id}: fmaxf(NaN, 0) = 0 expected where the fp64 convolution is NaN; " \
            f"{int((out.double() != ref).sum())} elements differ"
        return 0.0, _bits(out).clone(), yg, d
    adds = () if d["res"] is None else (d["res"],)
    if c.kind == "direct":
        bound = gamma(27 * cin_p + 2 + len(adds)) * d["mag"]
    else:
        bound = split_bound(d["conv_mag"], adds, presplit=c.fmt == "out_split")
    ratio = compare(c.id, cls, out, ref, bound, l2=c.kind == "split")
    return ratio, _bits(out).clone(), yg, d


def pair_halves(c):
    """the two launches of a ResBlock: t = relu(conv(x, w1)), y = conv(t, w2) + x"""
    kind = "split" if c.fmt == "presplit" else "direct"
    f1, f2 = ("out_split", "in_split") if c.fmt == "presplit" else ("f32", "f32")
    base = dict(kind=kind, V=c.V, D=c.D, H=c.H, W=c.W, cin=c.cin, cout=c.cout, tile=c.tile, wide=c.wide)
    return Case(id=c.id + "/relu", mode="relu", fmt=f1, **base), Case(id=c.id + "/res", mode="res", fmt=f2, **base)


def run_pair(be, c, cls):
    """the ResBlock as production chains it: the buffer the first launch wrote IS the second launch's input.  Each half is checked
    against fp64 on the operands it really read; the exact classes also end to end.  Returns (ratio, bits of y, bits of t, data 1, 2)"""
    assert c.cin == c.cout
    h1, h2 = pair_halves(c)
    r1, tbits, tg, d1 = run_c3(be, h1, cls, hold=0)   # hold = 0: the frame columns the 2-D tiles leave alone are the next launch's padding
    t = tbits.view(torch.float32)
    if cls != "randn" and c.fmt == "presplit":
        assert torch.equal(bf16_split(t), t)          # 16 bits hold the temporary
    r2, ybits, _, d2 = run_c3(be, h2, cls, feed=(tg, t, d1["x"]))
    if cls != "randn":
        want = F.conv3d(F.conv3d(d1["x"].double(), d1["w"].double(), padding=1).relu(), d2["w"].double(), padding=1) + d1["x"].double()
        assert torch.equal(ybits.view(torch.float32).double(), want), f"{c.id}/{cls}: the chained result differs from fp64"
    return max(r1, r2), ybits, tbits, d1, d2


# ------------------------------------------------------------------ stride 2
def _stride_setup(be, c, cls):
    K = be.K
    d = data(c, cls)
    half, full = level(c), level(c, 2)
    cin_p, cout_p = r16(c.cin), r64(c.cout)
    return K, d, half, full, cin_p, cout_p


def run_down(be, c, cls):
    """dinv_conv_down2x2_bf16s_3d: tap dz = 0 alone (accumulate = 0), then dz = 1 accumulated onto it (both taps = F.conv3d(stride=2)),
    and dz = 1 accumulated onto integers / N(0, 1) values; twice on fresh outputs.  Returns (ratio, bits of the two-tap result)"""
    K, d, lo, li, cin_p, cout_p = _stride_setup(be, c, cls)
    lib, st, gb = be.lib(), be.stream(), ctypes.byref
    owned = cout_p // 8
    xg = in_buf(be, li.g, _padc(vol_imgs(d["x"]), cin_p), "nan", guard=li.guard, depth=2 * c.D)
    wgs = [_weights(be, K.pack_down_bf16s_weight(_padw(d["w"][:, :, dz], cout_p, cin_p))) for dz in range(2)]
    ops = (xg, wgs[0], wgs[1])
    inner, _ = masks(lo.g, lo.guard, c.D)

    def call(yg, dz, acc, want):
        snap = _snapshot(ops)
        _emu_log(be)
        K.check(lib.dinv_conv_down2x2_bf16s_3d(gb(li.g), gb(lo.g), _p(xg.t, li.guard * 8), _p(wgs[dz].t), cin_p, cout_p, _p(yg.t, lo.guard * 8),
                                               c.D, dz, acc, st))
        be.sync()
        _check_log(be, c.id, [want])
        _unchanged(c.id, ops, snap)

    two, t0 = expected_launches(c)[1], expected_launches(c)[0]
    runs = []
    for _ in range(2):
        yg, pre, may = out_buf(be, lo.g, owned + 1, owned, "all", 8, lo.guard, c.D, HOLD)
        call(yg, 0, 0, t0)
        a0 = check_out(c, cls, lo.g, yg, pre, may, owned, 8, guard=lo.guard, depth=c.D).clone()     # (on the host, bits() is no copy)
        call(yg, 1, 1, two)
        a1 = check_out(c, cls, lo.g, yg, pre, may, owned, 8, guard=lo.guard, depth=c.D)
        # accumulate onto non-zero contents: the interior holds `prefill`, frames and padding slices NaN (they come back as zeros)
        yb, preb, mayb = out_buf(be, lo.g, owned + 1, owned, "all", 8, lo.guard, c.D, HOLD)
        fill = preb.clone().view(torch.float32)
        pf = to_buf(lo.g, _padc(vol_imgs(d["prefill"]), cout_p), None, lo.guard)
        fill[:owned][:, inner] = pf[:, inner]
        yb.t.copy_(be.dev(fill).reshape(-1))
        call(yb, 1, 1, two)
        b1 = check_out(c, cls, lo.g, yb, fill.view(torch.int32), mayb, owned, 8, guard=lo.guard, depth=c.D)
        runs.append((a0, a1, b1))
    for k in range(3):
        assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), f"{c.id}/{cls}: the second round gives other bits"
    a0, a1, b1 = (_volume(lo, t[:owned].contiguous(), c.V, c.cout, cls, c.id) for t in runs[0])
    mt, pf = d["mag_tap"], d["prefill"]
    ratio = compare(c.id + "/dz0", cls, a0, d["ref_tap"][0], split_bound(mt[0]), l2=True)
    ratio = max(ratio, compare(c.id + "/dz0+dz1", cls, a1, d["ref"], split_bound(mt[1], (mt[0],)) + 3 * 2.0 ** -16 * mt[0], l2=True))
    ratio = max(ratio, compare(c.id + "/prefill+dz1", cls, b1, d["ref_tap"][1] + pf.double(), split_bound(mt[1], (pf,))))
    return ratio, _bits(a1).clone()


def run_up(be, c, cls):
    """dinv_conv_up2x2_bf16s_3d: tap dz = 0 writes the interior of the slices 2 z + 1 and nothing else, dz = 1 then the slices 2 z + 2
    and nothing else; together F.conv_transpose3d(stride=2); twice on fresh outputs.  Returns (ratio, bits of the result)"""
    K, d, li, lo, cin_p, cout_p = _stride_setup(be, c, cls)
    lib, st, gb = be.lib(), be.stream(), ctypes.byref
    owned = cout_p // 8
    xg = in_buf(be, li.g, _padc(vol_imgs(d["x"]), cin_p), "nan", guard=li.guard, depth=c.D)
    x2g = None if d["x2"] is None else in_buf(be, li.g, _padc(vol_imgs(d["x2"]), cin_p), "nan", guard=li.guard, depth=c.D)
    wgs = [_weights(be, K.pack_up_bf16s_weight(_padw(d["w"][:, :, dz], cin_p, cout_p))) for dz in range(2)]
    ops = (xg, x2g, wgs[0], wgs[1])
    inner, _ = masks(lo.g, lo.guard, 2 * c.D)
    taps = []
    for dz in range(2):                               # the interior pixels of the slices 2 z + dz + 1
        m = torch.zeros(lo.g.cs, dtype=torch.bool)
        m[lo.guard + lo.g.sl:lo.guard + lo.g.sl + lo.g.np].view(c.V, 2 * c.D + 2, lo.g.plane)[:, 1 + dz:2 * c.D + 1:2] = True
        taps.append(m & inner)
    assert bool((taps[0] | taps[1]).equal(inner)) and not bool((taps[0] & taps[1]).any())
    launches = expected_launches(c)
    runs = []
    for _ in range(2):
        yg, pre, may = out_buf(be, lo.g, owned + 1, owned, taps[0], 8, lo.guard, 2 * c.D, HOLD)
        after = []
        for dz in range(2):
            snap = _snapshot(ops)
            _emu_log(be)
            K.check(lib.dinv_conv_up2x2_bf16s_3d(gb(li.g), gb(lo.g), _p(xg.t, li.guard * 8), None if x2g is None else _p(x2g.t, li.guard * 8),
                                                 _p(wgs[dz].t), cin_p, cout_p, _p(yg.t, lo.guard * 8), c.D, dz, st))
            be.sync()
            _check_log(be, c.id, [launches[dz]])
            _unchanged(c.id, ops, snap)
            # every word outside the tap's slices keeps the bits it had before the call (prefill, or the other tap's result)
            may_dz = torch.zeros_like(may)
            may_dz[:owned][:, taps[dz]] = True
            full = check_out(c, cls, lo.g, yg, pre if dz == 0 else _bits(after[0]).view(pre.shape), may_dz, owned, 8, frame_poison=True,
                             guard=lo.guard, depth=2 * c.D)
            after.append(full.clone())
        runs.append(after)
    for k in range(2):
        assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), f"{c.id}/{cls}: the second round gives other bits"
    first, both = runs[0]
    nanb = int(torch.tensor(float("nan")).view(torch.int32))
    assert bool((_bits(first)[:owned][:, taps[1]] == nanb).all())       # tap 0 left the slices of tap 1 alone (their NaN prefill)
    out = _volume(lo, both[:owned].contiguous(), c.V, c.cout, cls, c.id)
    adds_x2 = d["x2"] is not None
    ratio = compare(c.id, cls, out, d["ref"], split_bound(d["conv_mag"], x2=adds_x2), l2=True)
    half = torch.nan_to_num(_volume(lo, first[:owned].contiguous(), c.V, c.cout, "special", c.id), nan=0.0)
    want = d["ref"].clone()
    want[:, :, 1::2] = 0
    compare(c.id + "/dz0", cls, half, want, split_bound(d["conv_mag"], x2=adds_x2))
    return ratio, _bits(out).clone()


def run(be, case, cls):
    """(worst fraction of the class's ceiling, bits of the result) of one (case, class)"""
    if case.kind in C3_KINDS:
        return run_c3(be, case, cls)[:2]
    if case.kind == "pair":
        return run_pair(be, case, cls)[:2]
    return (run_down if case.kind == "down" else run_up)(be, case, cls)


def family(c):
    if c.kind == "direct":
        return "direct-thin" if c.cout <= 16 else "direct-wide"
    return "split" if c.kind == "pair" else c.kind


def run_case(be, case, cls):
    """run one (case, class); prints and returns the worst fraction of the class's ceiling (0 for the bit-exact classes)"""
    ratio = run(be, case, cls)[0]
    print(f"{case.id}/{cls}: " + (f"worst / bound = {ratio:.3g} ({family(case)})" if cls == "randn" else "exact"))
    return ratio


# ------------------------------------------------------------------ what production launches (models/drunet3d.py: Ops3d)
NC = (16, 32, 64, 128)
SETTINGS = {"infer-fp32": (False, "fp32"), "infer-bf16split": (False, "bf16split"), "train-fp32": (True, "bf16split")}


def production_items(emu):
    """(layer, setting) pairs of one run; the emulation leaves the 128 -> 128 block on the wide fp32 kernel to the device (30 s of
    fibers; the 64 -> 64 block takes the same kernel instance)"""
    return [(l, s) for l in production_layers() for s in SETTINGS if not (emu and l[0] == "block3" and s != "infer-bf16split")]


def production_layers():
    """every layer shape of the four-level 16 / 32 / 64 / 128 network on the smallest legal problem: (name, what, level, side of the
    problem) - [1, c, 8, 8, 8], and [1, c, 16, 16, 16] for the level-2 -> 3 stride-2 pair (its half grid would be 1 x 1 x 1 otherwise)"""
    out = [("head", "conv", 0, 8), ("tail", "conv", 0, 8)]
    out += [(f"block{i}", "block", i, 8) for i in range(4)]
    out += [(f"down{i}", "down", i, 8 if i < 2 else 16) for i in range(3)]
    out += [(f"up{i}", "up", i, 8 if i < 2 else 16) for i in range(3)]
    return out


def production_case(name, what, i, side, train, prec):
    """the table-style case of the launch(es) Ops3d must make for a layer in a setting - the dispatch of Ops3d.conv3 restated: the thin
    kernel for <= 16 -> <= 16 channels in every setting, the bf16-split kernel otherwise unless fp32 arithmetic is selected (training:
    train_forward_precision, here "fp32"; inference: conv_precision), the ReLU temporary pre-split exactly when the bf16-split
    kernels run a block at inference"""
    fp32 = True if train else prec == "fp32"
    s = side >> i
    if what == "conv":
        cin, cout = (3, NC[0]) if name == "head" else (NC[0], 2)
        return Case(id=f"prod-{name}", kind="direct", V=1, D=s, H=s, W=s, cin=cin, cout=cout)
    if what == "block":
        ch = NC[i]
        split = ch > 16 and not fp32
        return Case(id=f"prod-{name}-{'split' if split else 'fp32'}", kind="pair", V=1, D=s, H=s, W=s, cin=ch, cout=ch,
                    fmt="presplit" if split and not train else "direct", wide=False)
    h = s // 2
    cin, cout = (NC[i], NC[i + 1]) if what == "down" else (NC[i + 1], NC[i])
    return Case(id=f"prod-{name}", kind=what, V=1, D=h, H=h, W=h, cin=cin, cout=cout)


def run_production(be, name, what, i, side, setting):
    """one layer through Ops3d.conv3 / down / up in one setting: the launches are those of production_case (the emulation's launch
    log), the result has the bits of the same call made through the table's runner (and so equals fp64: data class `int`), the
    pre-split flag of the temporary is what the dispatch says, and everything outside the interior of the result is zero"""
    from deepinv_amd.models import drunet3d as T3
    train, prec = SETTINGS[setting]
    c = production_case(name, what, i, side, train, prec)
    model = types.SimpleNamespace(train_forward_precision="fp32", conv_precision=prec)
    ops = T3.Ops3d(model, torch.empty(1, 1, side, side, side, device=be.device), train)
    try:
        if what == "block":
            _, ybits, tbits, d1, d2 = run_pair(be, c, "int")
            x = _vol(be, T3, ops.lv[i], d1["x"])
            _emu_log(be)
            a1 = ops.conv3(i, be.dev(d1["w"]), x, relu=True, fp32=ops.fp32)
            y = ops.conv3(i, be.dev(d2["w"]), a1, res=x, fp32=ops.fp32)
            be.sync()
            _check_log(be, f"{c.id}/{setting}", expected_launches(c))
            assert a1.presplit == (c.fmt == "presplit"), f"{c.id}/{setting}: the temporary's pre-split flag is {a1.presplit}"
            lv = ops.lv[i]
            tv, _ = imgs_vol(from_buf(lv.g, decode(a1.t.cpu(), a1.presplit), lv.guard), 1)
            assert torch.equal(_bits(tv[:, :c.cout]), tbits), f"{c.id}/{setting}: the temporary differs from the table's call"
            assert outside_interior_is_zero(lv.g, a1.t.cpu(), lv.guard, lv.D)
            lvo = lv
        else:
            _, ybits = run(be, c, "int")
            d = data(c, "int")
            lvi = ops.lv[i + 1] if what == "up" else ops.lv[i]
            lvo = ops.lv[i + 1] if what == "down" else ops.lv[i]
            x = _vol(be, T3, lvi, d["x"])
            _emu_log(be)
            if what == "conv":
                y = ops.conv3(i, be.dev(d["w"]), x, fp32=ops.fp32_ends)
            else:
                y = (ops.down if what == "down" else ops.up)(i, be.dev(d["w"]), x, fp32=ops.fp32)
            be.sync()
            _check_log(be, f"{c.id}/{setting}", expected_launches(c))
            assert not y.presplit
        out, clean = _vol_out(lvo, y, c.cout)
        assert clean, f"{c.id}/{setting}: frames, padding slices, guard planes, slack or padded channels of the result are not zero"
        assert torch.equal(_bits(out), ybits), f"{c.id}/{setting}: Ops3d's result differs from the table's call"
    finally:
        be.K.clear_pack_cache()
        T3.release_buffers()
