"""ctypes wrappers for the DRUNet MFMA convolution kernels (csrc/drunet.hip)."""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import check, declare_once, lib, ptr, stream_ptr


class ActGeom(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
        ("hp", ctypes.c_int32), ("wp", ctypes.c_int32),
        ("plane", ctypes.c_int64), ("np", ctypes.c_int64), ("sl", ctypes.c_int64), ("cs", ctypes.c_int64),
    ]


# tuning constants of the fp32 setting (module attributes, no environment knobs): output tile of the Winograd kernel the
# ResBlock convolutions take (4: csrc/drunet_wino4.hip, 2: csrc/drunet_wino.hip) and the fewest workgroup tiles (64 couts x
# 32 tile positions) a launch must have for the F(4x4,3x3) kernel (one persistent workgroup per CU: 256 on MI355X)
FP32_WINOGRAD_TILE = 4
WINOGRAD4_MIN_TILES = 32
# True: the F(4x4,3x3) launches of the fp32 setting evaluate their multiplies as a three-part bf16 split, six products on the bf16
# matrix cores (dinv_conv3x3_winograd4_bf16x3: same per-layer accuracy, 3/8 of the matrix-pipe time).  Off by default: sustained,
# the package power limit makes the two forms equally fast at every batch (scripts/r05/bf16x3_e2e.py)
FP32_WINOGRAD4_BF16X3 = False
# False: the F(4x4,3x3) launches get no workspace, i.e. the incomplete last round of tiles is not cut along the input channels
# (diagnostic switch: bench.py --no-tail-split)
WINOGRAD4_TAIL_SPLIT = True


def _declare(l):
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    G = ctypes.POINTER(ActGeom)
    l.dinv_act_geom_init.argtypes = [i32, i32, i32, G]
    l.dinv_act_pack.argtypes = [G, vp, i32, vp, i32, f32, vp, vp]
    l.dinv_act_unpack.argtypes = [G, vp, i32, vp, vp]
    l.dinv_conv3x3.argtypes = [G, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp]
    l.dinv_conv3x3_tail.argtypes = [G, vp, vp, vp, i32, i32, vp, vp]
    if hasattr(l, "dinv_conv3x3_winograd"):     # (not part of the host emulation build, tests/emu/Makefile)
        l.dinv_conv3x3_winograd.argtypes = [G, vp, vp, i32, i32, vp, vp, i32, vp]
    l.dinv_conv3x3_winograd4.argtypes = [G, vp, vp, i32, i32, vp, vp, i32, vp, ctypes.c_size_t, vp]
    l.dinv_conv3x3_winograd4_bf16x3.argtypes = [G, vp, vp, i32, i32, vp, vp, i32, vp, ctypes.c_size_t, vp]
    l.dinv_conv3x3_winograd4_workspace_bytes.restype = ctypes.c_size_t
    l.dinv_conv3x3_winograd4_workspace_bytes.argtypes = []
    l.dinv_conv3x3_winograd4_last_split.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(i32)]
    l.dinv_conv3x3_split.argtypes = [G, vp, vp, i32, i32, vp, vp, i32, vp]
    l.dinv_conv3x3_wsplit.argtypes = [G, vp, vp, i32, i32, vp, vp, i32, vp]
    l.dinv_conv3x3x3_split.argtypes = [G, vp, vp, i32, i32, vp, vp, i32, i32, vp]
    l.dinv_conv3x3x3.argtypes = [G, vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, vp]
    l.dinv_conv_down2x2.argtypes = [G, G, vp, vp, i32, i32, vp, vp]
    l.dinv_conv_down2x2_bf16s.argtypes = [G, G, vp, vp, i32, i32, vp, vp]
    l.dinv_conv_down2x2_bf16x3.argtypes = [G, G, vp, vp, i32, i32, vp, vp]
    l.dinv_conv_up2x2_bf16s.argtypes = [G, G, vp, vp, vp, i32, i32, vp, vp]
    l.dinv_conv_wgrad_workspace_bytes.restype = ctypes.c_size_t
    l.dinv_conv_wgrad_workspace_bytes.argtypes = [G, i32, i32, i32]
    l.dinv_conv_wgrad.argtypes = [G, G, vp, i32, vp, i32, i32, vp, i32, vp, ctypes.c_size_t, vp]
    l.dinv_relu_backward.argtypes = [ctypes.c_int64, vp, vp, vp]
    l.dinv_conv_down2x2_bf16s_3d.argtypes = [G, G, vp, vp, i32, i32, vp, i32, i32, i32, vp]
    l.dinv_conv_up2x2_bf16s_3d.argtypes = [G, G, vp, vp, vp, i32, i32, vp, i32, i32, vp]
    l.dinv_conv_wgrad_3d.argtypes = [G, G, vp, i32, vp, i32, vp, i32, vp, ctypes.c_size_t, i32, i32, vp]
    l.dinv_conv_wgrad_3x3x3.argtypes = [G, vp, i32, vp, i32, ctypes.c_int64, vp, i32, vp, ctypes.c_size_t, vp]
    l.dinv_conv_up2x2.argtypes = [G, G, vp, vp, vp, i32, i32, vp, vp]
    l.dinv_conv3x3_bias.argtypes = [G, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, vp]
    l.dinv_conv3x3_winograd4_bias.argtypes = [G, vp, vp, vp, i32, i32, vp, i32, vp, ctypes.c_size_t, vp]
    l.dinv_conv3x3_tail_bias.argtypes = [G, vp, vp, vp, i32, i32, vp, vp, vp]
    l.dinv_bias_grad_workspace_bytes.restype = ctypes.c_size_t
    l.dinv_bias_grad_workspace_bytes.argtypes = [G, i32]
    l.dinv_bias_grad.argtypes = [G, vp, i32, vp, i32, vp, ctypes.c_size_t, vp]


def _l():
    return declare_once(lib(), _declare)


def geom(batch: int, h: int, w: int) -> ActGeom:
    g = ActGeom()
    check(_l().dinv_act_geom_init(batch, h, w, ctypes.byref(g)))
    return g


def alloc(g: ActGeom, channels: int, device) -> torch.Tensor:
    """zero-initialised activation buffer [ceil(channels/8), cs, 8] (padded pixel rows, channels blocked by 8)"""
    return torch.zeros(((channels + 7) // 8, g.cs, 8), device=device, dtype=torch.float32)


def pack_conv3x3_weight(w: torch.Tensor, mt: int | None = None) -> tuple[torch.Tensor, int, int]:
    """OIHW [Cout,Cin,3,3] -> [Cout/MT][Cin/8][9 taps][MT][8] (zero padded). Returns (packed, cin_p, cout_p)."""
    cout, cin = w.shape[:2]
    cin_p = (cin + 7) // 8 * 8
    cout_p = (cout + 31) // 32 * 32
    if mt is None:
        mt = 64 if cout_p % 64 == 0 else 32
    wp = torch.zeros((cout_p, cin_p, 3, 3), device=w.device, dtype=torch.float32)
    wp[:cout, :cin] = w.detach().float()
    wp = wp.reshape(cout_p // mt, mt, cin_p // 8, 8, 9).permute(0, 2, 4, 1, 3).contiguous()
    return wp, cin_p, cout_p


def pack_tail_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW [Cout<=4, Cin, 3, 3] -> [Cin/8][9 taps][Cout][8] for conv3x3_tail"""
    cout, cin = w.shape[:2]
    if cout > 4 or cin % 8:
        raise ValueError(f"tail packing needs cout <= 4 and cin % 8 == 0, got {cout},{cin}")
    return w.detach().float().reshape(cout, cin // 8, 8, 9).permute(1, 3, 0, 2).contiguous()


def pack_thin_weight(w: torch.Tensor) -> tuple[torch.Tensor, int]:
    """OIHW [Cout<=16, Cin, 3, 3] -> the one 16-wide cout tile of the thin-layer kernel (dinv_conv3x3 / dinv_conv3x3_bias with
    cout_tile = 16): [1][Cin/8][9 taps][16][8], zero padded.  Returns (packed, cin_p)."""
    cout, cin = w.shape[:2]
    if cout > 16:
        raise ValueError(f"thin packing needs cout <= 16, got {cout}")
    cin_p = (cin + 7) // 8 * 8
    wp = torch.zeros((16, cin_p, 3, 3), device=w.device, dtype=torch.float32)
    wp[:cout, :cin] = w.detach().float()
    return wp.reshape(1, 16, cin_p // 8, 8, 9).permute(0, 2, 4, 1, 3).contiguous(), cin_p


def pack_bias(b: torch.Tensor | None, cout_p: int, device=None) -> torch.Tensor:
    """bias [Cout] -> fp32 [cout_p], zero padded (what the bias epilogues read: one float per padded output channel)"""
    out = torch.zeros(cout_p, device=device if b is None else b.device, dtype=torch.float32)
    if b is not None:
        out[:b.shape[0]] = b.detach().float()
    return out


def _bf16_parts(w: torch.Tensor, n: int) -> list[torch.Tensor]:
    """the exact n-part bf16 split of an fp32 tensor, leading part first: every part is the residual left by the parts before it,
    rounded to nearest even (n = 2: hi = bf16(w), lo = bf16(w - hi); n = 3: hi, mid, lo - 24 significand bits)"""
    parts = [w.bfloat16()]
    for _ in range(n - 1):
        w = w - parts[-1].float()
        parts.append(w.bfloat16())
    return parts


def _pack_split_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW [Cout,Cin,3,3] -> two-part bf16 split (hi = bf16(w), lo = bf16(w - hi)),
    [Cout/64][Cin/16][dy 3][plane 2][dx 3][cblk 2][co 64][ci 8] (bf16)"""
    cout, cin = w.shape[:2]
    if cin % 16 or cout % 64:
        raise ValueError(f"bf16-split packing needs cin % 16 == 0 and cout % 64 == 0, got {cin},{cout}")
    planes = torch.stack(_bf16_parts(w.detach().float(), 2))                  # [2, Cout, Cin, 3, 3]
    planes = planes.reshape(2, cout // 64, 64, cin // 16, 2, 8, 3, 3)         # pl, ct, co, s, cblk, ci, dy, dx
    return planes.permute(1, 3, 6, 0, 7, 4, 2, 5).contiguous()               # ct, s, dy, pl, dx, cblk, co, ci


def split2d_row_perm() -> torch.Tensor:
    """MFMA A-row -> cout permutation inside a 32-row tile for csrc/drunet_split2d.hip: row 8g + 4h + e carries cout
    16 (g >> 1) + 8 h + 4 (g & 1) + e, so that the 16 accumulator registers of lane half h are the complete 8-channel blocks
    2k + h (k = 0, 1) of its pixel."""
    i = torch.arange(32)
    g, h, e = i >> 3, (i >> 2) & 1, i & 3
    return 16 * (g >> 1) + 8 * h + 4 * (g & 1) + e


def pack_split2d_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW [Cout,Cin,3,3] -> two-part bf16 split (hi = bf16(w), lo = bf16(w - hi)), packed for csrc/drunet_split2d.hip:
    [Cout/64][Cin/16][dy 3][plane 2][dx 3][cblk 2][row 64][ci 8] (bf16), rows of each 32-row tile permuted by
    `split2d_row_perm`"""
    packed = _pack_split_weight(w)                     # ct, s, dy, pl, dx, cblk, co 64, ci 8
    perm = split2d_row_perm().to(packed.device)
    idx = torch.cat((perm, 32 + perm))
    return packed.index_select(6, idx).contiguous()


def pack_wsplit_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW [Cout,Cin,3,3] -> Winograd F(2,3) weights along the kernel columns, U0 = g0, U1 = (g0+g1+g2)/2,
    U2 = (g0-g1+g2)/2, U3 = g2 per kernel row (fp64, rounded once to fp32), two-part bf16 split, packed for
    csrc/drunet_wsplit.hip as MFMA A fragments: [Cout/64][Cin/16][dy 3][point 4][m 2][plane 2][cblk 2][row 32][ci 8] (bf16),
    rows of each 32-row tile permuted by `split2d_row_perm`"""
    cout, cin = w.shape[:2]
    if cin % 16 or cout % 64:
        raise ValueError(f"Winograd bf16-split packing needs cin % 16 == 0 and cout % 64 == 0, got {cin},{cout}")
    g = w.detach().double()                                                     # [co, ci, dy, dx]
    u = torch.stack((g[..., 0], (g[..., 0] + g[..., 1] + g[..., 2]) / 2, (g[..., 0] - g[..., 1] + g[..., 2]) / 2, g[..., 2])).float()
    planes = torch.stack(_bf16_parts(u, 2))                                      # [pl 2, k 4, co, ci, dy 3]
    planes = planes.reshape(2, 4, cout // 64, 2, 32, cin // 16, 2, 8, 3)         # pl, k, ct, m, r, s, cblk, ci, dy
    planes = planes.index_select(4, split2d_row_perm().to(planes.device))
    return planes.permute(2, 5, 8, 1, 3, 0, 6, 4, 7).contiguous()               # ct, s, dy, k, m, pl, cblk, r, ci


def pack_split3d_weight(w5: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,3,3,3] -> the per-depth-tap packs of pack_split2d_weight stacked behind the cout tile:
    [Cout/64][dz 3][Cin/16][dy 3][plane 2][dx 3][cblk 2][row 64][ci 8] (bf16) for dinv_conv3x3x3_split"""
    return torch.stack([pack_split2d_weight(w5[:, :, dz]) for dz in range(3)], dim=1).contiguous()


def pack_winograd_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW [Cout,Cin,3,3] -> U = G g G^T (fp64, rounded once) packed [Cout/64][Cin/8][ci 8][co 64][16];
    needs Cin % 16 == 0, Cin >= 32 and Cout % 64 == 0 (the ResBlock convs; the kernel pipelines channel blocks
    in pairs and peels the last four)."""
    cout, cin = w.shape[:2]
    if cin % 16 or cin < 32 or cout % 64:
        raise ValueError(f"winograd packing needs cin % 16 == 0, cin >= 32 and cout % 64 == 0, got {cin},{cout}")
    G = [[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]]
    u = filter_transform(G, w.detach().double()).float().reshape(cout // 64, 64, cin // 8, 8, 16)
    return u.permute(0, 2, 3, 1, 4).contiguous()


def filter_transform(G, g: torch.Tensor) -> torch.Tensor:
    """G g G^T over the last two dimensions of g [..., 3, 3] for an n x 3 matrix G given as nested Python floats, as
    scalar-coefficient combinations of slices (fp64 elementwise arithmetic where the weights live): no matrix-multiply library is
    called for an n x 3 . 3 x 3 . 3 x n product per filter (a batched fp64 GEMM through rocBLAS / Tensile otherwise)"""
    def comb(coefs, parts):
        acc = None
        for c, p in zip(coefs, parts):
            if c != 0.0:
                acc = p * c if acc is None else acc + p * c
        return acc if acc is not None else torch.zeros_like(parts[0])

    rows = torch.stack([comb(Gi, [g[..., a, :] for a in range(3)]) for Gi in G], dim=-2)          # [..., n, 3] = G g
    return torch.stack([comb(Gj, [rows[..., :, b] for b in range(3)]) for Gj in G], dim=-1)       # [..., n, n] = (G g) G^T


def winograd4_matrices(dtype=torch.float64, device=None):
    """(B^T, G, A^T) of Winograd F(4x4, 3x3) (interpolation points 0, +-1, +-2, inf; Lavin & Gray 2016):
    Y = A^T [ (G g G^T) . (B^T d B) ] A for a 6x6 input patch d and a 3x3 filter g"""
    bt = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
                       [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=dtype, device=device)
    g = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6],
                      [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=dtype, device=device)
    at = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]],
                      dtype=dtype, device=device)
    return bt, g, at


# Winograd point 6 * row + col held by each of the 36 point slots of csrc/drunet_wino4.hip: every wave's nine consecutive slots
# are a full row of the 6 x 6 transform followed by half a row (the halves of rows 1 and 4), so that every wave's epilogue
# retires the same six accumulators first
WINOGRAD4_POINT_SLOTS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 15, 16, 17, 9, 10, 11,
                         18, 19, 20, 21, 22, 23, 24, 25, 26, 30, 31, 32, 33, 34, 35, 27, 28, 29)


def pack_winograd4_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW [Cout,Cin,3,3] -> U = G g G^T of Winograd F(4x4,3x3) (fp64, rounded once to fp32), packed for
    csrc/drunet_wino4.hip as the MFMA A fragments of the wave that uses them:
    [Cout/64][Cin/8][wave = 4 c2 + q][k 9][lane = 32 h + r][m 4] holds U[point slot 9 q + k][cout 64 ct + 32 c2 + r][cin 8 cb + 4 h + m];
    needs Cin % 16 == 0 and Cout % 64 == 0"""
    cout, cin = w.shape[:2]
    if cin % 16 or cout % 64:
        raise ValueError(f"winograd F(4,3) packing needs cin % 16 == 0 and cout % 64 == 0, got {cin},{cout}")
    _, G, _ = winograd4_matrices(device="cpu")
    u = filter_transform(G.tolist(), w.detach().double()).float()       # [co, ci, 6, 6]
    u = u.reshape(cout, cin, 36)[:, :, list(WINOGRAD4_POINT_SLOTS)]     # slot order: see WINOGRAD4_POINT_SLOTS
    u = u.reshape(cout // 64, 2, 32, cin // 8, 2, 4, 4, 9)              # ct, c2, r, cb, h, m, q, k
    return u.permute(0, 3, 1, 6, 7, 4, 2, 5).contiguous()               # ct, cb, c2, q, k, h, r, m


def pack_winograd4_bf16x3_weight(w: torch.Tensor) -> torch.Tensor:
    """OIHW [Cout,Cin,3,3] -> the U of pack_winograd4_weight (fp64, rounded once to fp32) as its exact THREE-part bf16 split
    u = uh + um + ul (round to nearest even each), packed for dinv_conv3x3_winograd4_bf16x3: per (cout tile, channel block, wave,
    point) 1536 bytes = [lane 64][um 4 | uh 4] then [lane 64][ul 4] (bf16): the (um, uh) and (uh, ul) operand windows of the
    wave's three bf16 MFMAs, loaded as 16 + 8 bytes per lane.  Returns a bfloat16 tensor [Cout/64][Cin/8][8][9][768]"""
    u = pack_winograd4_weight(w)                                        # ct, cb, c2, q, k, h, r, m   (fp32)
    hi, mid, lo = _bf16_parts(u, 3)
    ct, cb = u.shape[:2]
    mh = torch.stack((mid, hi), dim=-2).reshape(ct, cb, 8, 9, 512)      # [h, r][part 2][m 4]
    return torch.cat((mh, lo.reshape(ct, cb, 8, 9, 256)), dim=-1).contiguous()


def pack_down_weight(w: torch.Tensor) -> torch.Tensor:
    """Conv2d k2 s2 weight [Cout,Cin,2,2] -> [tap=dy*2+dx][Cin/8][Cout][8]"""
    cout, cin = w.shape[:2]
    return w.detach().float().permute(2, 3, 1, 0).reshape(4, cin // 8, 8, cout).permute(0, 1, 3, 2).contiguous()


def pack_down_bf16s_weight(w: torch.Tensor, parts: int = 2) -> torch.Tensor:
    """Conv2d k2 s2 weight [Cout,Cin,2,2] -> `parts`-part bf16 split packed [tap=dy*2+dx][Cin/16][plane `parts`][cblk 2][Cout][ci 8]"""
    cout, cin = w.shape[:2]
    if cin % 16 or cout % 64:
        raise ValueError(f"bf16-split down packing needs cin % 16 == 0 and cout % 64 == 0, got {cin},{cout}")
    planes = torch.stack(_bf16_parts(w.detach().float(), parts)).reshape(parts, cout, cin // 16, 2, 8, 2, 2)   # pl, co, s, cblk, ci, dy, dx
    return planes.permute(5, 6, 2, 0, 3, 1, 4).contiguous()                       # dy, dx, s, pl, cblk, co, ci


def pack_down_bf16x3_weight(w: torch.Tensor) -> torch.Tensor:
    """Conv2d k2 s2 weight [Cout,Cin,2,2] -> THREE-part bf16 split (hi, mid, lo: 24 significand bits) packed
    [tap=dy*2+dx][Cin/16][plane 3][cblk 2][Cout][ci 8] for dinv_conv_down2x2_bf16x3 (six products: fp32-equivalent)"""
    return pack_down_bf16s_weight(w, parts=3)


def pack_up_bf16s_weight(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d k2 s2 weight [Cin,Cout,2,2] -> two-part bf16 split packed [Cin/16][tap=dy*2+dx][plane 2][cblk 2][Cout][ci 8]"""
    cin, cout = w.shape[:2]
    if cin % 16 or cout % 64:
        raise ValueError(f"bf16-split up packing needs cin % 16 == 0 and cout % 64 == 0, got {cin},{cout}")
    planes = torch.stack(_bf16_parts(w.detach().float(), 2)).reshape(2, cin // 16, 2, 8, cout, 2, 2)   # pl, s, cblk, ci, co, dy, dx
    return planes.permute(1, 5, 6, 0, 2, 4, 3).contiguous()                       # s, dy, dx, pl, cblk, co, ci


def pack_up_weight(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d k2 s2 weight [Cin,Cout,2,2] -> [tap=dy*2+dx][Cin/8][Cout][8]"""
    cin, cout = w.shape[:2]
    return w.detach().float().permute(2, 3, 0, 1).reshape(4, cin // 8, 8, cout).permute(0, 1, 3, 2).contiguous()


class ConvPacks(NamedTuple):
    """the packs of ONE 3x3 convolution, one field per kernel that may run it (None: that kernel does not take the layer)"""
    p64: torch.Tensor                       # direct fp32 kernel, 64-wide cout tiles (32-wide where cout_p % 64: then p32 is p64)
    p32: torch.Tensor                       # direct fp32 kernel, 32-wide cout tiles
    cin_p: int                              # padded channel counts of the two direct packs (what the launches are given)
    cout_p: int
    wino2: torch.Tensor | None = None       # pack_winograd_weight
    split2d: torch.Tensor | None = None     # pack_split2d_weight
    wsplit: torch.Tensor | None = None      # pack_wsplit_weight
    wino4: torch.Tensor | None = None       # pack_winograd4_weight
    wino4x3: torch.Tensor | None = None     # pack_winograd4_bf16x3_weight
    bias: torch.Tensor | None = None        # pack_bias to cout_p

    def pick(self, g) -> torch.Tensor:
        """the direct pack for launch geometry g: 64-wide cout tiles unless that grid would leave the chip under-filled (< 3 rounds
        of the 512 resident workgroup slots): then 32-wide tiles double the number of workgroups (small per-GPU batches)"""
        if self.p64.shape[3] == 64 and ((g.np + 255) // 256) * (self.cout_p // 64) < 1536:
            return self.p32
        return self.p64


def conv_packs(w: torch.Tensor, bias: torch.Tensor | None = None, precision: str | None = None) -> ConvPacks:
    """ConvPacks of an OIHW weight: the two direct packs and the bias; with `precision`, also the packs of that setting's ResBlock
    kernels where the layer has their shape ("bf16split": split2d, wsplit; "fp32": wino2, wino4 and, with FP32_WINOGRAD4_BF16X3,
    wino4x3)"""
    p64, cin_p, cout_p = pack_conv3x3_weight(w)
    p32 = pack_conv3x3_weight(w, mt=32)[0] if p64.shape[3] == 64 else p64
    ok = w.shape[0] % 64 == 0 and w.shape[1] % 16 == 0
    split, fp32 = ok and precision == "bf16split", ok and precision == "fp32"
    return ConvPacks(p64, p32, cin_p, cout_p,
                     wino2=pack_winograd_weight(w) if fp32 and w.shape[1] >= 32 else None,
                     split2d=pack_split2d_weight(w) if split else None,
                     wsplit=pack_wsplit_weight(w) if split else None,
                     wino4=pack_winograd4_weight(w) if fp32 else None,
                     wino4x3=pack_winograd4_bf16x3_weight(w) if fp32 and FP32_WINOGRAD4_BF16X3 else None,
                     bias=pack_bias(bias, cout_p) if bias is not None else None)


class StridePacks(NamedTuple):
    """the packs of ONE 2x2 stride-2 layer, strided or transposed, one field per kernel that may run it (None: that kernel does not
    take the layer); `launch_down` / `launch_up` run the layer"""
    direct: torch.Tensor                    # direct fp32 kernel: pack_down_weight / pack_up_weight
    split: torch.Tensor | None = None       # two-part bf16 split: pack_down_bf16s_weight / pack_up_bf16s_weight
    x3: torch.Tensor | None = None          # three-part bf16 split, six products (fp32-equivalent): pack_down_bf16x3_weight


def stride_packs(w: torch.Tensor, up: bool = False, precision: str | None = None) -> StridePacks:
    """StridePacks of a Conv2d [Cout,Cin,2,2] or (`up`) ConvTranspose2d [Cin,Cout,2,2] weight: the direct pack; with `precision`, also
    the pack of that setting's kernel where the layer has its shape ("bf16split": split; "fp32": x3 - the fp32-MFMA kernel is bound
    by that pipe -, strided layers only)"""
    cin, cout = w.shape[:2] if up else (w.shape[1], w.shape[0])
    ok = cout % 64 == 0 and cin % 16 == 0
    if up:
        return StridePacks(pack_up_weight(w), split=pack_up_bf16s_weight(w) if ok and precision == "bf16split" else None)
    return StridePacks(pack_down_weight(w),
                       split=pack_down_bf16s_weight(w) if ok and precision == "bf16split" else None,
                       x3=pack_down_bf16x3_weight(w) if ok and precision == "fp32" else None)


# Packed weights of the training / 3-D paths are cached per source tensor: an unfolded network calls the denoiser
# `max_iter` times per training step with the same weights and every layer needs a pack (a dozen small torch ops) per
# call otherwise - more host time than the kernels take.  One entry per (kind, storage address, shape, sub): the entry
# remembers the tensor's version counter, and a call that finds another version REPLACES the entry (an optimizer step
# bumps the counter of every parameter, so the packs of the previous step are dropped right there instead of piling up).
# An entry keeps its source tensor alive, so the address cannot be handed to another tensor while the entry exists.
# Not detected: in-place updates through `p.data` (hand-written SGD / EMA: `.data` ops do not bump the counter) and
# inference-mode tensors (no counter) - call `clear_pack_cache()` after such an update (load_state_dict, torch.optim and
# `deepinv_amd.training.Trainer` need nothing: they bump the counter / call it).
_PACKS: dict = {}


def clear_pack_cache():
    """drop every cached weight pack (after in-place weight updates the version counter does not see)"""
    _PACKS.clear()


def cached_pack(kind, w, make, sub=0):
    try:
        ver = w._version
    except RuntimeError:      # inference tensors carry no version counter
        ver = -1
    key = (kind, w.data_ptr(), tuple(w.shape), sub)
    hit = _PACKS.get(key)
    if hit is None or hit[1] != ver:
        if hit is None and len(_PACKS) > 4096:
            _PACKS.clear()
        hit = _PACKS[key] = (make(), ver, w)
    return hit[0]


def weights_version(module) -> tuple:
    """changes whenever a parameter of `module` is updated in place or replaced: what the packs a model keeps were made from
    (tensors created under torch.inference_mode() carry no version counter - reading it raises)"""
    params = list(module.parameters())
    return tuple(0 if p.is_inference() else p._version for p in params) + tuple(p.data_ptr() for p in params)


def pack_input(g, x, sigma, act):
    dev = x.device
    if isinstance(sigma, torch.Tensor):
        if sigma.numel() == 1:
            mode, sp, sv = 0, None, float(sigma.item()) if not sigma.is_cuda else None
            if sv is None:  # device scalar: avoid a host sync, expand on device
                sigma = sigma.reshape(1).expand(g.batch).contiguous().float()
                mode, sp, sv = 1, sigma, 0.0
        elif sigma.numel() == g.batch:
            mode, sp, sv = 1, sigma.reshape(-1).contiguous().float().to(dev), 0.0
        else:
            mode, sp, sv = 2, sigma.contiguous().float().to(dev), 0.0
    else:
        mode, sp, sv = 0, None, float(sigma)
    check(_l().dinv_act_pack(ctypes.byref(g), ptr(x), x.shape[1], ptr(sp), mode, sv, ptr(act), stream_ptr(dev)))


def unpack_output(g, act, cout, y):
    check(_l().dinv_act_unpack(ctypes.byref(g), ptr(act), cout, ptr(y), stream_ptr(y.device)))


# ---- optional live profiling: HIP events around every conv3x3 launch on the launch stream
_prof = None


def profile_begin():
    global _prof
    _prof = []


def profile_end():
    """per-kernel totals of the 3x3 conv launches since profile_begin():
    {kernel: {"ms", "launches", "direct_flops" (2*9*Cin*Cout*pixels), "mfma_flops" (executed on the MFMA pipe:
    the same for the direct kernel, 16/36 of it per 2x2 tile for Winograd F(2x2,3x3))}}"""
    global _prof
    rec, _prof = _prof, None
    out = {}
    if not rec:
        return out
    torch.cuda.synchronize()
    for e0, e1, name, direct, mfma in rec:
        d = out.setdefault(name, {"ms": 0.0, "launches": 0, "direct_flops": 0.0, "mfma_flops": 0.0})
        d["ms"] += e0.elapsed_time(e1)
        d["launches"] += 1
        d["direct_flops"] += direct
        d["mfma_flops"] += mfma
    return out


class _profiled:
    """``with _profiled(kernel, direct_flops, mfma_flops):`` around ONE launch - between profile_begin() and profile_end() the launch
    is bracketed by two HIP events and noted under the kernel's name with its two flop counts; otherwise nothing happens"""
    __slots__ = ("rec",)

    def __init__(self, kernel, direct_flops, mfma_flops):
        self.rec = None
        if _prof is not None:
            self.rec = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), kernel, direct_flops, mfma_flops)

    def __enter__(self):
        if self.rec is not None:
            self.rec[0].record()

    def __exit__(self, *exc):
        if self.rec is not None:
            self.rec[1].record()
            _prof.append(self.rec)


def _conv_flops(g, cin, cout):
    """2 * 9 * Cin * Cout per interior pixel: what the direct form of a 3x3 convolution executes"""
    return 2.0 * 9 * cin * cout * g.batch * g.height * g.width


def conv3x3(g, x, wpk, cin, cout, y, cout_valid=None, x2=None, res1=None, res2=None, relu=False, cin_valid=None):
    """wpk: packed weight tensor [cout/MT][cin/8][9][MT][8]; MT is read off its shape"""
    co = cout if cout_valid is None else cout_valid
    fl = _conv_flops(g, cin if cin_valid is None else cin_valid, co)
    with _profiled("conv3x3_kernel", fl, fl):
        check(_l().dinv_conv3x3(ctypes.byref(g), ptr(x), ptr(x2), ptr(wpk), cin, cout, co, int(wpk.shape[3]), ptr(y), ptr(res1),
                                ptr(res2), int(relu), stream_ptr(y.device)))


def pack_conv3x3x3_weight(w5: torch.Tensor) -> tuple[torch.Tensor, int, int]:
    """[Cout, Cin, 3, 3, 3] -> fp32 pack of dinv_conv3x3x3: [cout/MT][dz][cin/8][9 taps][MT][8] (zero padded; MT = 16 for
    Cout <= 16 - the thin-layer kernel -, else 64 / 32 as in pack_conv3x3_weight).  Returns (packed, cin_p, cout_p)."""
    cout, cin = w5.shape[:2]
    cin_p = (cin + 7) // 8 * 8
    if cout <= 16:
        mt, cout_p = 16, 16
    else:
        cout_p = (cout + 31) // 32 * 32
        mt = 64 if cout_p % 64 == 0 else 32
    wp = torch.zeros((cout_p, cin_p, 3, 3, 3), device=w5.device, dtype=torch.float32)
    wp[:cout, :cin] = w5.detach().float()
    # (co/mt, mt, ci/8, 8, dz, 9) -> (co/mt, dz, ci/8, 9, mt, 8)
    wp = wp.reshape(cout_p // mt, mt, cin_p // 8, 8, 3, 9).permute(0, 4, 2, 5, 1, 3).contiguous()
    return wp, cin_p, cout_p


def conv3x3x3(g, x, wpk, cin, cout, y, depth, cout_valid=None, res1=None, relu=False, gate=False):
    """fp32 3x3x3 convolution of volumes stored as stacks of depth + 2 slices, ONE launch (depth taps inside the K loop
    of csrc/drunet.hip: conv3x3_kernel / conv3_thin_kernel); wpk from pack_conv3x3x3_weight; views as for conv3x3x3_split.
    gate (thin kernel): y = res1 > 0 ? conv : 0"""
    check(_l().dinv_conv3x3x3(ctypes.byref(g), ptr(x), ptr(wpk), cin, cout, cout if cout_valid is None else cout_valid,
                              int(wpk.shape[4]), ptr(y), ptr(res1), int(relu) | (2 if gate else 0), int(depth), stream_ptr(y.device)))


def conv3x3_tail(g, x, wtail, cin, cout, y, x2=None):
    """last layer on the vector ALU: y[:cout] = conv3x3(x (+x2)); wtail from pack_tail_weight"""
    check(_l().dinv_conv3x3_tail(ctypes.byref(g), ptr(x), ptr(x2), ptr(wtail), cin, cout, ptr(y), stream_ptr(y.device)))


def conv3x3_split(g, x, wsplit, cin, cout, y, res1=None, relu=False, x_presplit=False, y_presplit=False, gate=False):
    """y = [relu](conv3x3(x)) (+res1) on the bf16 matrix cores, two-part exact operand split, 2-D pixel tiles
    (csrc/drunet_split2d.hip); wsplit from pack_split2d_weight.  `x_presplit` / `y_presplit`: the activation buffer holds
    (8 bf16 high parts | 8 bf16 low parts) per pixel and channel block instead of 8 fp32 values (same 32 bytes)."""
    flags = (1 if x_presplit else 0) | (2 if y_presplit else 0) | (4 if relu else 0) | (8 if gate else 0)   # gate: y = res1 > 0 ? conv : 0
    fl = _conv_flops(g, cin, cout)
    with _profiled("conv3x3_split2d_kernel", fl, 3.0 * fl):
        check(_l().dinv_conv3x3_split(ctypes.byref(g), ptr(x), ptr(wsplit), cin, cout, ptr(y), ptr(res1), flags,
                                      stream_ptr(y.device)))


def conv3x3_wsplit(g, x, wws, cin, cout, y, res1=None, relu=False):
    """y = [relu](conv3x3(x)) (+res1): Winograd F(2,3) along rows on the bf16 matrix cores, two-part operand split
    (csrc/drunet_wsplit.hip); wws from pack_wsplit_weight; even image width"""
    fl = _conv_flops(g, cin, cout)
    with _profiled("conv3x3_wsplit_kernel", fl, 2.0 * fl):                 # 12 of 18 multiplies, three products each
        check(_l().dinv_conv3x3_wsplit(ctypes.byref(g), ptr(x), ptr(wws), cin, cout, ptr(y), ptr(res1), 4 if relu else 0,
                                       stream_ptr(y.device)))


def conv3x3x3_split(g, x, wsplit, cin, cout, y, depth, res1=None, relu=False, x_presplit=False, y_presplit=False, gate=False):
    """3x3x3 convolution of volumes stored as stacks of depth + 2 slices, one launch (depth taps inside the K loop of
    csrc/drunet_split2d.hip); wsplit from pack_split3d_weight; x / y / res1 are views whose first plane is a volume's
    leading zero slice, with one more readable plane on each side of x"""
    flags = (1 if x_presplit else 0) | (2 if y_presplit else 0) | (4 if relu else 0) | (8 if gate else 0)   # gate: y = res1 > 0 ? conv : 0
    check(_l().dinv_conv3x3x3_split(ctypes.byref(g), ptr(x), ptr(wsplit), cin, cout, ptr(y), ptr(res1), flags, int(depth),
                                    stream_ptr(y.device)))


def conv3x3_winograd(g, x, wino, cin, cout, y, res1=None, relu=False):
    """y = [relu](conv3x3(x)) (+res1) via Winograd F(2x2,3x3); wino from pack_winograd_weight"""
    tiles = g.batch * ((g.height + 1) // 2) * ((g.width + 1) // 2)
    with _profiled("conv3x3_wino_kernel", _conv_flops(g, cin, cout), 2.0 * 16 * cin * cout * tiles):
        check(_l().dinv_conv3x3_winograd(ctypes.byref(g), ptr(x), ptr(wino), cin, cout, ptr(y), ptr(res1), int(relu),
                                         stream_ptr(y.device)))


_W4_WS: dict = {}


def winograd4_workspace(device):
    """the workspace of dinv_conv3x3_winograd4's tail split for the CURRENT stream of `device` (zero-filled once; the library
    keeps its ticket words zero between launches).  Launches on one stream are ordered, so one buffer serves every layer issued
    there; two streams of a device must not share one (their tail parts would take each other's tickets and partial outputs),
    hence the key (device, stream)."""
    if not WINOGRAD4_TAIL_SPLIT:
        return None
    device = torch.device(device)
    if device.type == "cuda":
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (idx, torch.cuda.current_stream(idx).cuda_stream)
    else:
        key = (str(device), 0)
    ws = _W4_WS.get(key)
    if ws is None:
        ws = _W4_WS[key] = torch.zeros(_l().dinv_conv3x3_winograd4_workspace_bytes(), device=device, dtype=torch.uint8)
    return ws


def winograd4_last_split():
    """(parts per tail tile, tail tiles per XCD) of this thread's last conv3x3_winograd4 launch"""
    f, n = ctypes.c_int32(0), ctypes.c_int32(0)
    check(_l().dinv_conv3x3_winograd4_last_split(ctypes.byref(f), ctypes.byref(n)))
    return f.value, n.value


def conv3x3_winograd4(g, x, wino4, cin, cout, y, res1=None, relu=False, workspace=None):
    """y = [relu](conv3x3(x)) (+res1) via Winograd F(4x4,3x3) on the fp32 matrix cores (csrc/drunet_wino4.hip); wino4 from
    pack_winograd4_weight; height and width multiples of 4; `workspace` (winograd4_workspace(device)) enables the tail split"""
    tiles = g.batch * (g.height // 4) * (g.width // 4)
    with _profiled("conv3x3_wino4_kernel", _conv_flops(g, cin, cout), 2.0 * 36 * cin * cout * tiles):
        check(_l().dinv_conv3x3_winograd4(ctypes.byref(g), ptr(x), ptr(wino4), cin, cout, ptr(y), ptr(res1), int(relu),
                                          ptr(workspace), 0 if workspace is None else workspace.numel(), stream_ptr(y.device)))


def conv3x3_winograd4_bf16x3(g, x, wino4x3, cin, cout, y, res1=None, relu=False, workspace=None):
    """conv3x3_winograd4 with the multiplies as a three-part bf16 split, six products on the bf16 matrix cores (fp32-equivalent:
    csrc/drunet_wino4.hip, BF3); wino4x3 from pack_winograd4_bf16x3_weight"""
    tiles = g.batch * (g.height // 4) * (g.width // 4)
    # executed: 6 bf16 products per fp32 multiply of the F(4x4) form
    with _profiled("conv3x3_wino4_kernel<bf16x3>", _conv_flops(g, cin, cout), 2.0 * 6 * 36 * cin * cout * tiles):
        check(_l().dinv_conv3x3_winograd4_bf16x3(ctypes.byref(g), ptr(x), ptr(wino4x3), cin, cout, ptr(y), ptr(res1), int(relu),
                                                 ptr(workspace), 0 if workspace is None else workspace.numel(), stream_ptr(y.device)))


def down2x2(gi, go, x, w, cin, cout, y):
    check(_l().dinv_conv_down2x2(ctypes.byref(gi), ctypes.byref(go), ptr(x), ptr(w), cin, cout, ptr(y), stream_ptr(y.device)))


def down2x2_bf16s(gi, go, x, wsplit, cin, cout, y):
    """the same 2x2 stride-2 convolution on the bf16 matrix cores (weights from pack_down_bf16s_weight)"""
    check(_l().dinv_conv_down2x2_bf16s(ctypes.byref(gi), ctypes.byref(go), ptr(x), ptr(wsplit), cin, cout, ptr(y),
                                       stream_ptr(y.device)))


def down2x2_bf16x3(gi, go, x, wsplit3, cin, cout, y):
    """the same 2x2 stride-2 convolution with the three-part operand split and six products: fp32-equivalent
    (weights from pack_down_bf16x3_weight)"""
    check(_l().dinv_conv_down2x2_bf16x3(ctypes.byref(gi), ctypes.byref(go), ptr(x), ptr(wsplit3), cin, cout, ptr(y),
                                        stream_ptr(y.device)))


def up2x2_bf16s(gi, go, x, x2, wsplit, cin, cout, y):
    """the same transposed convolution on the bf16 matrix cores (weights from pack_up_bf16s_weight)"""
    check(_l().dinv_conv_up2x2_bf16s(ctypes.byref(gi), ctypes.byref(go), ptr(x), ptr(x2), ptr(wsplit), cin, cout, ptr(y),
                                     stream_ptr(y.device)))


def up2x2(gi, go, x, x2, w, cin, cout, y):
    check(_l().dinv_conv_up2x2(ctypes.byref(gi), ctypes.byref(go), ptr(x), ptr(x2), ptr(w), cin, cout, ptr(y),
                               stream_ptr(y.device)))


def launch_down(gi, go, x, pk: StridePacks, cin, cout, y):
    """y = the 2x2 stride-2 convolution of x, on the kernel whose pack `pk` holds (the arithmetic of the ResBlock convolutions of the
    setting the packs were built for)"""
    if pk.split is not None:
        down2x2_bf16s(gi, go, x, pk.split, cin, cout, y)
    elif pk.x3 is not None:
        down2x2_bf16x3(gi, go, x, pk.x3, cin, cout, y)
    else:
        down2x2(gi, go, x, pk.direct, cin, cout, y)


def launch_up(gi, go, x, x2, pk: StridePacks, cin, cout, y):
    """y = the 2x2 stride-2 transposed convolution of x (+ x2), on the kernel whose pack `pk` holds"""
    if pk.split is not None:
        up2x2_bf16s(gi, go, x, x2, pk.split, cin, cout, y)
    else:
        up2x2(gi, go, x, x2, pk.direct, cin, cout, y)


def conv_wgrad(gs, gl, s, m, l, n, taps, dw=None, accumulate=False):
    """dw[m][n][t] (+)= sum_p S[m][p] L[n][map(p) + off_t] (csrc/drunet_bwd.hip); returns dw of shape [m, n, k, k]"""
    k = 3 if taps == 9 else 2
    if dw is None:
        dw = torch.empty((m, n, k, k), device=s.device, dtype=torch.float32)
        accumulate = False
    ws = torch.empty(_l().dinv_conv_wgrad_workspace_bytes(ctypes.byref(gs), m, n, taps), device=s.device, dtype=torch.uint8)
    check(_l().dinv_conv_wgrad(ctypes.byref(gs), ctypes.byref(gl), ptr(s), m, ptr(l), n, taps, ptr(dw), int(accumulate), ptr(ws),
                               ws.numel(), stream_ptr(s.device)))
    return dw


def conv_wgrad_3x3x3(g, s, m, l_first, n, depth_stride):
    """[m, n, 3, 3, 3] weight gradient of a 3x3x3 layer in one call: the three depth taps are the second grid dimension of ONE launch
    and of one reduction (csrc/drunet_bwd.hip: dinv_conv_wgrad_3x3x3); l_first = the layer input shifted by -1 slice"""
    dw = torch.empty((m, n, 3, 3, 3), device=s.device, dtype=torch.float32)
    ws = torch.empty(3 * _l().dinv_conv_wgrad_workspace_bytes(ctypes.byref(g), m, n, 9), device=s.device, dtype=torch.uint8)
    check(_l().dinv_conv_wgrad_3x3x3(ctypes.byref(g), ptr(s), m, ptr(l_first), n, int(depth_stride), ptr(dw), 0, ptr(ws), ws.numel(),
                                     stream_ptr(s.device)))
    return dw


def relu_backward(act, grad):
    """grad <- grad * (act > 0) in place, on whole activation buffers"""
    check(_l().dinv_relu_backward(grad.numel(), ptr(act), ptr(grad), stream_ptr(grad.device)))
    return grad


def down2x2_bf16s_3d(gi, go, x, wsplit, cin, cout, y, depth_out, dz, accumulate):
    """depth tap dz of a 2x2x2 stride-2 convolution (volumes as stacks of D + 2 slices); wsplit = pack_down_bf16s_weight(w[:, :, dz])"""
    check(_l().dinv_conv_down2x2_bf16s_3d(ctypes.byref(gi), ctypes.byref(go), ptr(x), ptr(wsplit), cin, cout, ptr(y), depth_out, dz,
                                          int(accumulate), stream_ptr(y.device)))


def up2x2_bf16s_3d(gi, go, x, wsplit, cin, cout, y, depth_in, dz):
    """depth tap dz of a 2x2x2 stride-2 transposed convolution: writes the slices 2 z + dz of the output volume"""
    check(_l().dinv_conv_up2x2_bf16s_3d(ctypes.byref(gi), ctypes.byref(go), ptr(x), None, ptr(wsplit), cin, cout, ptr(y), depth_in,
                                        dz, stream_ptr(y.device)))


def conv_wgrad_3d(gs, gl, s, m, l, n, depth_s, dz):
    """[m, n, 2, 2] weight gradient of depth tap dz of a 2x2x2 stride-2 layer"""
    dw = torch.empty((m, n, 2, 2), device=s.device, dtype=torch.float32)
    ws = torch.empty(_l().dinv_conv_wgrad_workspace_bytes(ctypes.byref(gs), m, n, 4), device=s.device, dtype=torch.uint8)
    check(_l().dinv_conv_wgrad_3d(ctypes.byref(gs), ctypes.byref(gl), ptr(s), m, ptr(l), n, ptr(dw), 0, ptr(ws), ws.numel(), depth_s,
                                  dz, stream_ptr(s.device)))
    return dw


# ---- DnCNN (models/dncnn.py): the same convolutions with a bias in the epilogue
def conv3x3_bias(g, x, wpk, bias, cin, cout, y, cout_valid=None, res1=None, relu=False):
    """y = relu(conv3x3(x) + bias) or conv3x3(x) + bias (+res1) on the direct fp32 kernel; wpk from pack_conv3x3_weight (MT = 32 / 64)
    or pack_thin_weight (cout = 16); bias from pack_bias (cout floats)"""
    mt = int(wpk.shape[3])
    co = cout if cout_valid is None else cout_valid
    with _profiled("conv3_thin_kernel" if mt == 16 else "conv3x3_kernel", _conv_flops(g, cin, co), 2.0 * 9 * cin * cout * g.np):
        check(_l().dinv_conv3x3_bias(ctypes.byref(g), ptr(x), ptr(wpk), ptr(bias), cin, cout, co, mt, ptr(y), ptr(res1), int(relu),
                                     stream_ptr(y.device)))


def conv3x3_winograd4_bias(g, x, wino4, bias, cin, cout, y, relu=False, workspace=None):
    """y = [relu](conv3x3(x) + bias) via Winograd F(4x4,3x3) (csrc/drunet_wino4.hip, bias in the epilogue); wino4 from
    pack_winograd4_weight; height and width multiples of 4"""
    tiles = g.batch * (g.height // 4) * (g.width // 4)
    with _profiled("conv3x3_wino4_kernel", _conv_flops(g, cin, cout), 2.0 * 36 * cin * cout * tiles):
        check(_l().dinv_conv3x3_winograd4_bias(ctypes.byref(g), ptr(x), ptr(wino4), ptr(bias), cin, cout, ptr(y), int(relu),
                                               ptr(workspace), 0 if workspace is None else workspace.numel(), stream_ptr(y.device)))


def conv3x3_tail_bias(g, x, wtail, bias, cin, cout, y, res=None):
    """last layer on the vector ALU: y[:cout] = conv3x3(x) + bias (+ res, first channel block); wtail from pack_tail_weight"""
    with _profiled("tail3x3_shift_kernel", _conv_flops(g, cin, cout), 0.0):
        check(_l().dinv_conv3x3_tail_bias(ctypes.byref(g), ptr(x), ptr(wtail), ptr(bias), cin, cout, ptr(y), ptr(res), stream_ptr(y.device)))


def bias_grad(g, gy, c, db=None, accumulate=False):
    """db[ch] (+)= sum of gy[ch] over the interior pixels, ch < c (csrc/drunet_bwd.hip: fixed-order, deterministic); returns db [c]"""
    if db is None:
        db = torch.empty(c, device=gy.device, dtype=torch.float32)
        accumulate = False
    ws = torch.empty(_l().dinv_bias_grad_workspace_bytes(ctypes.byref(g), c), device=gy.device, dtype=torch.uint8)
    check(_l().dinv_bias_grad(ctypes.byref(g), ptr(gy), c, ptr(db), int(accumulate), ptr(ws), ws.numel(), stream_ptr(gy.device)))
    return db
