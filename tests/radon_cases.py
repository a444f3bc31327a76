"""Shared by tests/test_radon_gpu.py (the gfx950 library) and tests/test_emu_radon_cases.py (the same kernel sources on the host
emulation): one table of Radon cases, each meant to reach one dispatch path of csrc/radon.hip and csrc/radon_tiled.hip (the
tiled and gather parallel-beam pairs, the interpolating back-projection, the fan-beam pair, the FFT and direct ramp filters) at
one of its edges, the fp64 references, a restatement of the dispatch rules of deepinv_amd/hip/radon.py and the C launchers
(expected_launches), and the runner that calls the C entry points on guarded buffers (fft_cases.Guarded).

The references restate the operator the kernels implement in exact arithmetic on the fp32 host tables the device reads (cos /
sin, the fan tables, ixtab), promoted to fp64: sample (j, i) of angle a sits at (ix, iy) = ctr + R (j - ctr, i - ctr), it counts
when floor(ix), floor(iy) lie in [-1, G - 1], and its four bilinear taps read the zero-padded (or disc-masked) image.  Every
element is checked against a bound of the form
    |y - y64| <= beta * (u * n * M + ulp(G) * T)
with u = 2^-24, n the terms summed per output, M the same operator applied to absolute values and T the sum of the absolute
values over the 4 x 4 pixel neighbourhood of every sample (unit weights): the positions live at the fp32 spacing of G, and a
position that rounds across an integer adds or drops a tap of weight ulp(G).  A wrong or dropped tap is an O(1 / taps) error
against that measure; an output with zero measure must be exactly zero.  The ramp filter is checked per column (FFT path) or
per element (direct path) against the linear convolution with h[0] = 1/2, h[odd d] = -2 / (pi d)^2."""
import ctypes
import math
from dataclasses import dataclass

import torch

from fft_cases import POISON, Guarded

from deepinv_amd.hip.radon import RadonDesc, RadonPlan

U = 2.0 ** -24
TILED_MAX_GRID = 4096             # MAXG of csrc/radon_tiled.hip
RAMP_FFT_MAX_P = 8192             # deepinv_amd/hip/radon.py
MAX_LDS = 160 * 1024              # kMaxLdsBytes
GATHER_LDS = 64 * 1024            # the LDS tables of the first-generation kernels
MAX_IMAGES = 65535                # images per ramp / back-projection call (grid z)


def ulp(x):
    """fp32 spacing at x (x >= 1)"""
    return 2.0 ** (math.floor(math.log2(x)) - 23)


# ------------------------------------------------------------------ host tables (as deepinv_amd.hip.radon builds them)
class RadonGeom:
    """the host tables exactly as deepinv_amd.hip.radon.RadonGeometry builds them (fp32, CPU)"""

    def __init__(self, angles_deg, width, circle):
        sqrt2 = (2 * torch.ones(1)).sqrt()
        self.W = int(width)
        if circle:
            self.G, self.pad = self.W, 0
        else:
            self.G = int((sqrt2 * self.W).ceil())
            pad = int((sqrt2 * self.W - self.W).ceil())
            self.pad = (self.W + pad) // 2 - self.W // 2
        self.circle = bool(circle)
        a = torch.as_tensor(angles_deg, dtype=torch.float32)
        theta = a * 4 * torch.ones(1).atan() / 180
        self.A = int(a.numel())
        self.cs = torch.stack([theta.cos(), theta.sin()], dim=1).contiguous()
        self.xn = torch.linspace(-1, 1, self.G).contiguous()
        X = torch.arange(self.A, dtype=torch.float32) * 2.0 / (self.A - 1) - 1.0 if self.A > 1 else torch.zeros(1)
        self.ixtab = (((X + 1.0) / 2) * (self.A - 1)).contiguous()

    def desc(self, n_img, scale=1.0):
        return RadonDesc(n_img, self.W, self.G, self.pad, self.A, int(self.circle), float(scale), 0)

    def plan_host(self, lib, n_img, kw=0):
        """dinv_radon_plan_init: (plan, int32 blob); kw = 1, 2, 4, 8 forces the angles per workgroup, 0 = automatic"""
        d = self.desc(n_img)
        blob = torch.zeros(lib.dinv_radon_plan_bytes(ctypes.byref(d)) // 4, dtype=torch.int32)
        pl = RadonPlan()
        pl.kw = kw
        rc = lib.dinv_radon_plan_init(ctypes.byref(d), ctypes.c_void_p(self.cs.data_ptr()), ctypes.byref(pl),
                                      ctypes.c_void_p(blob.data_ptr()))
        if rc != 0:
            raise RuntimeError(f"dinv_radon_plan_init error {rc}: {lib.dinv_last_error().decode()}")
        return pl, blob

    def disc(self):
        """the inscribed-disc mask of the pack kernels (fp32 arithmetic, radon.py:270-283); all ones without circle"""
        if not self.circle:
            return torch.ones(self.W, self.W, dtype=torch.bool)
        k = torch.arange(self.W, dtype=torch.float32)
        ax = 2.0 * k / float(self.W - 1) - 1.0
        return (ax[:, None] * ax[:, None] + ax[None, :] * ax[None, :]) <= 1.0


class FanGeom(RadonGeom):
    """fan-beam tables from the product's own host code (deepinv_amd.hip.radon.fan_tables: pure torch)"""

    def __init__(self, angles_deg, width, circle, fan_parameters=None):
        super().__init__(angles_deg, width, circle)
        import os
        import sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if root not in sys.path:
            sys.path.insert(0, root)
        from deepinv_amd.hip.radon import fan_tables
        self.fp, self.xm, self.sc, self.yd = fan_tables(self.G, self.W, fan_parameters)
        self.n_det = int(self.yd.numel())


# ------------------------------------------------------------------ fp64 references
def _padded(geo, x, border=2):
    """x [n, W, W] -> [n, G + 2 border, G + 2 border] fp64: disc mask, zero padding, `border` zero pixels around the grid"""
    n = x.shape[0]
    G, b = geo.G, border
    out = torch.zeros(n, G + 2 * b, G + 2 * b, dtype=torch.float64)
    xm = x.double() * geo.disc().double()
    out[:, b + geo.pad:b + geo.pad + geo.W, b + geo.pad:b + geo.pad + geo.W] = xm
    return out


def _sample_sum(img, ix, iy, G, b=2):
    """sum over the samples (ix, iy) [R, S] of their bilinear value in img [n, G+2b, G+2b] (weighted) and of the 4 x 4
    neighbourhood (unit weights) of |img|: ([n, R], [n, R], [n, R]) = (value, value of |img|, T)"""
    fx, fy = torch.floor(ix), torch.floor(iy)
    ok = (fx >= -1) & (fx <= G - 1) & (fy >= -1) & (fy <= G - 1)
    tx, ty = ix - fx, iy - fy
    x0 = (fx.clamp(-2, G).long() + b)
    y0 = (fy.clamp(-2, G).long() + b)
    n, P = img.shape[0], img.shape[-1]
    flat, absf = img.reshape(n, -1), img.abs().reshape(n, -1)
    okd = ok.double()
    val = torch.zeros(n, ix.shape[0], dtype=torch.float64)
    mag = torch.zeros_like(val)
    T = torch.zeros_like(val)
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            idx = ((y0 + dy).clamp(0, P - 1) * P + (x0 + dx).clamp(0, P - 1)).reshape(-1)
            a = absf[:, idx].view(n, *ix.shape)
            T += (a * okd).sum(-1)
            if dx in (0, 1) and dy in (0, 1):
                w = ((tx if dx else 1 - tx) * (ty if dy else 1 - ty)) * okd
                val += (flat[:, idx].view(n, *ix.shape) * w).sum(-1)
                mag += (a * w).sum(-1)
    return val, mag, T


def ref_forward(geo, x, angles=None, chunk=1 << 22):
    """fp64 parallel-beam forward of x [n, W, W] for the angle indices `angles` (None: all): (y, M, T) each [n, G, len]"""
    G = geo.G
    angles = list(range(geo.A)) if angles is None else list(angles)
    img = _padded(geo, x)
    ctr = 0.5 * (G - 1)
    d = torch.arange(G, dtype=torch.float64) - ctr
    outs = [torch.zeros(x.shape[0], G, len(angles), dtype=torch.float64) for _ in range(3)]
    rows = max(1, chunk // G)
    cs = geo.cs.double()
    for k, a in enumerate(angles):
        c, s = float(cs[a, 0]), float(cs[a, 1])
        for j0 in range(0, G, rows):
            dj = d[j0:j0 + rows, None]
            ix = ctr + c * dj + s * d[None, :]
            iy = ctr - s * dj + c * d[None, :]
            for o, r in zip(outs, _sample_sum(img, ix, iy, G)):
                o[:, j0:j0 + rows, k] = r
    return outs


def ref_adjoint(geo, v, pixels=None):
    """fp64 transpose of ref_forward applied to v [n, G, A] at the image pixels `pixels` ([P] flat indices into W x W; None:
    all), by the lattice points within reach of every pixel: (x, A^T |v|, T^T |v|) each [n, P].  Exactly the transpose: every
    sample whose 4 x 4 neighbourhood holds the pixel lies within 3 lattice steps of the pixel's inverse image."""
    G, W = geo.G, geo.W
    n = v.shape[0]
    pix = torch.arange(W * W) if pixels is None else torch.as_tensor(pixels)
    row, col = pix // W, pix % W
    live = geo.disc().reshape(-1)[pix].double()
    px, py = (col + geo.pad).double(), (row + geo.pad).double()
    ctr = 0.5 * (G - 1)
    dx, dy = px - ctr, py - ctr
    vd = v.double()
    va = vd.abs()
    x = torch.zeros(n, pix.numel(), dtype=torch.float64)
    m = torch.zeros_like(x)
    T = torch.zeros_like(x)
    off = torch.arange(-3, 4, dtype=torch.float64)
    cs = geo.cs.double()
    for a in range(geo.A):
        c, s = float(cs[a, 0]), float(cs[a, 1])
        ux, uy = torch.floor(c * dx - s * dy + ctr), torch.floor(s * dx + c * dy + ctr)
        j = ux[:, None, None] + off[None, :, None]          # [P, 7, 1]
        i = uy[:, None, None] + off[None, None, :]          # [P, 1, 7]
        ix = ctr + c * (j - ctr) + s * (i - ctr)
        iy = ctr - s * (j - ctr) + c * (i - ctr)
        fx, fy = torch.floor(ix), torch.floor(iy)
        ok = (j >= 0) & (j <= G - 1) & (i >= 0) & (i <= G - 1) & (fx >= -1) & (fx <= G - 1) & (fy >= -1) & (fy <= G - 1)
        ex, ey = px[:, None, None] - fx, py[:, None, None] - fy
        w = (1 - (ix - px[:, None, None]).abs()).clamp_min(0) * (1 - (iy - py[:, None, None]).abs()).clamp_min(0) * ok
        near = (ok & (ex >= -1) & (ex <= 2) & (ey >= -1) & (ey <= 2)).double()
        jj = j.expand_as(ix).clamp(0, G - 1).long()
        vj, vaj = vd[:, :, a][:, jj], va[:, :, a][:, jj]          # [n, P, 7, 7]
        x += (vj * w).sum((-1, -2))
        m += (vaj * w).sum((-1, -2))
        T += (vaj * near).sum((-1, -2))
    return x * live, m * live, T * live


def ref_backproject(geo, v):
    """iradon_kernel in fp64 on the fp32 tables: x[row, col] = sum_a bilinear(v, ixtab[a], ((xg c - yg s + 1) / 2)(G - 1)), zero
    padding, disc mask on the fp32 grid values: (x, |.| of the same, T over rows floor - 1 .. floor + 2 of the two columns)"""
    G, W, A = geo.G, geo.W, geo.A
    n = v.shape[0]
    xn = geo.xn.double()
    xg, yg = xn[geo.pad:geo.pad + W][None, :], xn[geo.pad:geo.pad + W][:, None]   # [1, W] cols, [W, 1] rows
    live = torch.ones(W, W, dtype=torch.bool)
    if geo.circle:
        xf = geo.xn[geo.pad:geo.pad + W]
        live = (xf[None, :] * xf[None, :] + xf[:, None] * xf[:, None]) <= 1.0
    vd = v.double().reshape(n, G * A)
    va = vd.abs()
    out = [torch.zeros(n, W, W, dtype=torch.float64) for _ in range(3)]
    cs, ixt = geo.cs.double(), geo.ixtab.double()
    for a in range(A):
        t = xg * float(cs[a, 0]) - yg * float(cs[a, 1])
        iy = ((t + 1) / 2) * (G - 1)
        ix = float(ixt[a])
        fy, fx = torch.floor(iy), math.floor(ix)
        ty, tx = iy - fy, ix - fx
        for dy in range(-1, 3):
            for dx in range(0, 2):
                yy, xx = fy + dy, fx + dx
                ok = ((yy >= 0) & (yy < G) & (0 <= xx < A)).double()
                idx = (yy.clamp(0, G - 1).long() * A + min(max(xx, 0), A - 1)).reshape(-1)
                g, ga = vd[:, idx].view(n, W, W), va[:, idx].view(n, W, W)
                out[2] += ga * ok
                if dy in (0, 1):
                    w = (ty if dy else 1 - ty) * (tx if dx else 1 - tx) * ok
                    out[0] += g * w
                    out[1] += ga * w
    return [o * live for o in out]


def _fan_samples(geo, angles):
    """(ix, iy) [len(angles), n_det, G] of the fan-beam samples R(theta) (xm_i, yd_d sc_i), grid_sample-unnormalised"""
    cs = geo.cs.double()[list(angles)]
    c, s = cs[:, 0, None, None], cs[:, 1, None, None]
    xj = geo.xm.double()[None, None, :]
    xi = geo.yd.double()[None, :, None] * geo.sc.double()[None, None, :]
    gx, gy = c * xj + s * xi, -s * xj + c * xi
    gm1 = geo.G - 1
    return ((gx + 1) / 2) * gm1, ((gy + 1) / 2) * gm1


def ref_fan_forward(geo, x):
    """fp64 fan-beam forward: (y, M, T) each [n, n_det, A]"""
    img = _padded(geo, x)
    ix, iy = _fan_samples(geo, range(geo.A))
    outs = _sample_sum(img, ix.reshape(-1, geo.G), iy.reshape(-1, geo.G), geo.G)
    return [o.view(x.shape[0], geo.A, geo.n_det).transpose(1, 2) for o in outs]


def ref_fan_adjoint(geo, v):
    """fp64 transpose of ref_fan_forward by scattering every sample's taps: (x, A^T |v|, T^T |v|) each [n, W, W]"""
    G, b = geo.G, 2
    P = G + 2 * b
    n = v.shape[0]
    ix, iy = _fan_samples(geo, range(geo.A))                      # [A, D, G]
    fx, fy = torch.floor(ix), torch.floor(iy)
    ok = ((fx >= -1) & (fx <= G - 1) & (fy >= -1) & (fy <= G - 1)).double()
    tx, ty = ix - fx, iy - fy
    x0, y0 = fx.clamp(-2, G).long() + b, fy.clamp(-2, G).long() + b
    vv = v.double().permute(0, 2, 1)[:, :, :, None].expand(n, geo.A, geo.n_det, G)   # [n, A, D, G]
    outs = [torch.zeros(n, P * P, dtype=torch.float64) for _ in range(3)]
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            idx = ((y0 + dy).clamp(0, P - 1) * P + (x0 + dx).clamp(0, P - 1)).reshape(-1)
            outs[2].index_add_(1, idx, (vv.abs() * ok).reshape(n, -1))
            if dx in (0, 1) and dy in (0, 1):
                w = (tx if dx else 1 - tx) * (ty if dy else 1 - ty) * ok
                outs[0].index_add_(1, idx, (vv * w).reshape(n, -1))
                outs[1].index_add_(1, idx, (vv.abs() * w).reshape(n, -1))
    live = geo.disc().double()
    sl = slice(b + geo.pad, b + geo.pad + geo.W)
    return [o.view(n, P, P)[:, sl, sl] * live for o in outs]


def ramp_taps(N):
    """h[d], d = 0 .. N - 1 of the ramp filter's linear convolution"""
    d = torch.arange(N, dtype=torch.float64)
    h = torch.where(d % 2 == 1, -2.0 / (math.pi * d) ** 2, torch.zeros_like(d))
    h[0] = 0.5
    return h


def ref_ramp(y, absolute=False):
    """out[n, j, a] = sum_m h[|j - m|] y[n, m, a] in fp64 (FFT of length >= 2N: the linear convolution); absolute: |h| * |y|"""
    N = y.shape[-2]
    h = ramp_taps(N)
    yy = y.double()
    if absolute:
        h, yy = h.abs(), yy.abs()
    L = 1 << max(1, math.ceil(math.log2(2 * N)))
    hf = torch.zeros(L, dtype=torch.float64)
    hf[:N] = h
    hf[L - N + 1:] = h[1:].flip(0)
    Y = torch.fft.rfft(yy, n=L, dim=-2)
    out = torch.fft.irfft(Y * torch.fft.rfft(hf)[:, None], n=L, dim=-2)[..., :N, :]
    return out.clamp_min(0) if absolute else out


def ramp_pair_measure(y, P):
    """u log2(P) times the norm of the complex column each angle column travels in through ramp_fft_kernel: columns 2c and 2c + 1
    are the real and imaginary part of one transform, so the rounding error of either scales with the norm of the pair (a lone
    last column of an odd angle count: its own norm).  y [n, N, A] -> [n, 1, A]"""
    sq = y.double().pow(2).sum(-2, keepdim=True)
    A = y.shape[-1]
    partner = torch.arange(A) ^ 1
    has = partner < A
    pair = sq + torch.where(has, sq[..., partner.clamp(max=A - 1)], torch.zeros_like(sq))
    return pair.sqrt() * U * math.log2(P)


def ramp_fft_ratio(out, y, P):
    """worst over columns of max_j |out - ref| / ramp_pair_measure"""
    err = (out.detach().cpu().double().reshape(y.shape) - ref_ramp(y)).abs().amax(-2, keepdim=True)
    meas = ramp_pair_measure(y, P)
    return worst_ratio(err, torch.zeros_like(meas), meas)


# ------------------------------------------------------------------ error bounds
# beta of every path: max over elements of |out - ref| / measure, the measure of each path given in the module docstring and
# in run_case; measured on the host emulation (`python -m pytest tests/test_emu_radon_cases.py -s` prints every case's worst)
# and the bound at about 4x the worst there.
BOUNDS = {
    "fwd_tiled": 0.5,           # worst 0.126 emulated / 0.126 on the device (tiled-W40-A30-n2-norm)
    "fwd_gather": 0.26,         # worst 0.064 emulated (gather-W11c-A24-n3-on-circle) / 0.091 on the device (the 264-image case)
    "adj_tiled": 0.6,           # worst 0.142 / 0.142 (tiled-W37-A1-n2-one)
    "adj_gather": 0.8,          # worst 0.195 / 0.195 (gather-W37-A1-n2-one)
    "backproject": 0.7,         # worst 0.164 (bp-W16c-A2) / 0.153 (bp-W16-A2)
    "fan_fwd": 1.0,             # worst 0.237 / 0.237 (fan-W3c-det16375-lds-edge)
    "fan_adj": 0.35,            # worst 0.085 / 0.048 (fan-W31-det20-belowG-n5)
    # in units of u log2(P) ||(y_2c, y_2c+1)|| (ramp_pair_measure): worst 0.275 emulated / 0.277 on the device
    # (ramp-fft-ct8-N3-A3-n4000), 0.299 over the 196611 columns of the 65537-image test on the device
    "ramp_fft": 1.1,
    "ramp_direct": 0.7,         # worst 0.163 / 0.163 (ramp-direct-N23-A16-n2), in units of u N (|h| * |y|)
}
DOT_BOUND = 1e-7          # |<Ax, v> - <x, A^T v>| / (||Ax|| ||v||) of the pair a case reached


# ------------------------------------------------------------------ the dispatch rules, restated
def nb_of(n_img):
    return 8 if n_img >= 8 else 4 if n_img >= 4 else 2 if n_img >= 2 else 1


def ramp_padded(N):
    p = 64
    while p < 2 * N:
        p *= 2
    return p


def ramp_ct(P):
    """columns per workgroup of ramp_fft_kernel: the largest of 8, 4, 2, 1 whose twiddles + columns fit the LDS"""
    ct = 8
    while ct > 1 and (P + ct * (P + 1)) * 8 > MAX_LDS:
        ct >>= 1
    return ct


def classes(geo):
    """angles per (class, direction) as build_plan sorts them: plain +, plain -, swap +, swap -"""
    out = [0, 0, 0, 0]
    for c, s in geo.cs.tolist():
        swap = abs(s) > abs(c)
        slope = s if swap else c
        out[(2 if swap else 0) + (0 if slope > 0 else 1)] += 1
    return out


def forward_is_tiled(case, kw):
    """radon.py _fwd: the tiled forward for G <= TILED_MAX_GRID with a plan of >= 4 angles per workgroup or FORCE_TILED"""
    return not case.gather and case.geo.G <= TILED_MAX_GRID and (kw >= 4 or case.force_tiled)


def adjoint_is_tiled(case):
    return not case.gather and case.geo.G <= TILED_MAX_GRID


def expected_launches(case, op, kw=None):
    """the instantiations and block sizes the emulation's launch log must show for op "fwd" / "adj" / "bp" / "ramp" /
    "fan_fwd" / "fan_adj" of `case` (kw: the plan's angles per workgroup)"""
    geo = case.geo
    nb = nb_of(case.n_img)
    if op == "fwd":
        if forward_is_tiled(case, kw):
            cl = classes(geo)
            pf = 9 if kw == 8 else 18
            out = [f"radon_pack_image2<{nb}> x256"]
            if cl[0] + cl[1]:
                out.append(f"radon_fwd_tiled_kernel<{nb}, false, {pf}> x{64 * kw}")
            if cl[2] + cl[3]:
                out.append(f"radon_fwd_tiled_kernel<{nb}, true, {pf}> x{64 * kw}")
            return out
        return [f"radon_pack_image<{nb}> x256", f"radon_fwd_kernel<{nb}> x256"]
    if op == "adj":
        if adjoint_is_tiled(case):
            return [f"radon_pack_sino2<{nb}> x256", f"radon_adj_tiled_kernel<{nb}> x256"]
        return [f"radon_pack_sino<{nb}> x256", f"radon_adj_kernel<{nb}> x256"]
    if op == "bp":
        return ["iradon_kernel x256"]
    if op == "ramp":
        P = ramp_padded(case.N)
        return ["ramp_fft_kernel x256" if P <= RAMP_FFT_MAX_P and not case.direct else "ramp_kernel x256"]
    if op == "fan_fwd":
        return [f"radon_pack_image<{nb}> x256", f"radon_fan_fwd_kernel<{nb}> x256"]
    if op == "fan_adj":
        return [f"radon_pack_sino<{nb}> x256", f"radon_fan_adj_kernel<{nb}> x256"]
    raise ValueError(op)


def expected_chunks(geo, kw):
    """(n_chunks_plain, n_chunks_swap) of a plan with kw angles per workgroup: one run of chunks per (class, direction)"""
    cl = classes(geo)
    ch = [-(-k // kw) for k in cl]
    return ch[0] + ch[1], ch[2] + ch[3]


def plan_slack(geo, pl, blob):
    """the smallest distance, in columns, between a tap of a valid sample (fp64 position) and the edge of the LDS window the plan
    gives its (chunk, ray block, band), on the left and on the right.  dinv_radon_plan_init keeps one column of margin on either
    side (the taps sit at fp32 positions, which may round across an integer), so both must be >= 1 - except against the zero
    ring, column -1, which nothing lies left of."""
    blob = blob.cpu().numpy() if isinstance(blob, torch.Tensor) else blob
    G, A, kw, BH = geo.G, geo.A, pl.kw, pl.band_h
    nch_max = (A + kw - 1) // kw + 4
    angles = blob[:nch_max * kw].reshape(nch_max, kw)
    off = nch_max * kw + nch_max
    wtab = torch.from_numpy(blob[off:off + nch_max * pl.n_jblocks * pl.n_bands].reshape(nch_max, pl.n_jblocks, pl.n_bands))
    nch = pl.n_chunks_plain + pl.n_chunks_swap
    assert sorted(int(a) for a in angles[:nch].ravel() if a >= 0) == list(range(A)), "every angle in exactly one chunk"
    ctr = 0.5 * (G - 1)
    d = torch.arange(G, dtype=torch.float64) - ctr
    jb = (torch.arange(G) // 64)[:, None].expand(G, G)
    cs = geo.cs.double()
    left = right = 1 << 30
    for ch in range(nch):
        swap = ch >= pl.n_chunks_plain
        for a in angles[ch]:
            if a < 0:
                continue
            c, s = float(cs[a, 0]), float(cs[a, 1])
            ix = ctr + c * d[:, None] + s * d[None, :]
            iy = ctr - s * d[:, None] + c * d[None, :]
            u, v = (iy, ix) if swap else (ix, iy)
            u0, v0 = torch.floor(u).long(), torch.floor(v).long()
            ok = (u0 >= -1) & (u0 <= G - 1) & (v0 >= -1) & (v0 <= G - 1)
            band = ((v0 + 1) // BH).clamp(0, pl.n_bands - 1)
            w = wtab[ch][jb, band]
            wx0, ww = (w & 0xffff) - 8, w >> 16
            ls = (u0 - wx0)[ok & (wx0 > -1)]
            rs = (wx0 + ww - 1 - (u0 + 1))[ok]
            left = min(left, int(ls.min()) if ls.numel() else left)
            right = min(right, int(rs.min()) if rs.numel() else right)
    return left, right


# ------------------------------------------------------------------ the case table
BORDERS = (0., 44.9, 45., 45.1, 89.9, 90., 90.1, 134.9, 135., 135.1, 179.9)
WILD = (-30., 200., 359., 720.5, 17., 93., -91., 17., 400.25, 271.)        # negative, above 360, unsorted, a duplicate
FULL = tuple(float(a) for a in (torch.arange(24) * 15.0 + 1.5))             # all four (class, direction) runs


def uniform(n, stop=180.0):
    return tuple(float(a) for a in torch.linspace(0, stop, n + 1)[:-1])


@dataclass
class Case:
    id: str
    kind: str                   # "par", "bp", "fan", "ramp", "reject"
    emu: bool                   # small enough for the host emulation
    W: int = 0
    angles: tuple = ()
    circle: bool = False
    n_img: int = 1
    gather: bool = False        # ENABLE_TILED = False
    force_tiled: bool = False   # FORCE_TILED
    kw_force: int = 0           # plan.kw on entry to dinv_radon_plan_init
    kw_expect: int = 0          # the plan's kw the case is meant to reach (0: not tiled)
    scale: float = 1.0
    norm: float = 0.0           # a device norm scalar (tiled entries), 0: none
    fan: dict = None
    N: int = 0                  # ramp: detectors, angles in A_ramp
    A_ramp: int = 0
    direct: bool = False        # ENABLE_RAMP_FFT = False
    subset: bool = False        # check a subset of angles / pixels against fp64 (large cases)
    reject: str = ""            # rejection: which one

    @property
    def geo(self):
        if not hasattr(self, "_geo"):
            if self.kind == "fan":
                self._geo = FanGeom(self.angles, self.W, self.circle, self.fan)
            else:
                self._geo = RadonGeom(self.angles, self.W, self.circle)
        return self._geo


def _par(cases, W, angles, n_img=1, circle=False, gather=False, emu=True, tag="", **kw):
    c = Case("", "par", emu, W=W, angles=tuple(angles), circle=circle, n_img=n_img, gather=gather, **kw)
    path = "gather" if gather or c.geo.G > TILED_MAX_GRID else "tiled"
    c.id = f"{path}-W{W}{'c' if circle else ''}-A{len(angles)}-n{n_img}" + tag
    cases.append(c)


FAN_A = {"pixel_spacing": 0.1, "source_radius": 6.0, "detector_radius": 6.0, "n_detector_pixels": 20, "detector_spacing": 0.34}
FAN_FINE = {"pixel_spacing": 0.1, "source_radius": 8.0, "detector_radius": 2.0, "n_detector_pixels": 150,
            "detector_spacing": 0.03}


def build_cases():
    cases = []
    # ---- NB = 1, 2, 4, 8 with ragged last groups, on both pairs; class borders, any angle list, A = 1
    for gather in (False, True):
        _par(cases, 64, uniform(45), 1, gather=gather, kw_expect=0 if gather else 8)
        _par(cases, 50, uniform(45), 3, circle=True, gather=gather, kw_expect=0 if gather else 8)
        _par(cases, 97, BORDERS, 5, gather=gather, kw_expect=0 if gather else 8, tag="-borders")
        _par(cases, 33, WILD, 9, gather=gather, force_tiled=True, tag="-wild")
        _par(cases, 45, uniform(17), 15, gather=gather, tag="-g64")
        _par(cases, 37, (30.,), 2, gather=gather, force_tiled=True, tag="-one")
        _par(cases, 37, (90.,), 1, circle=True, gather=gather, force_tiled=True, tag="-one90")
    # ---- tiled forward plans: kw = 8 / 4 as production chooses, kw = 2 / 1 forced, all four (class, direction) runs
    _par(cases, 128, uniform(30), 9, kw_expect=4, tag="-kw4")
    for kw in (1, 2, 4, 8):
        _par(cases, 40, FULL, 3 if kw < 4 else 1, kw_force=kw, force_tiled=True, kw_expect=kw, tag=f"-full-kw{kw}")
    _par(cases, 33, WILD, 4, kw_force=1, force_tiled=True, kw_expect=1, tag="-wild-kw1")
    # ---- image sizes: the smallest, odd / even, G around multiples of 64 (ray blocks) and 16 (bands)
    # the adjoint's staged segment at 45 degrees: a lattice point 12 detectors below a tile centre whose coordinate is nearly an
    # integer still carries weight (odd G puts the centre of the diagonal tiles on an integer)
    _par(cases, 57, (45., 135., 225., 315.), 2, force_tiled=True, tag="-seg45")
    _par(cases, 71, uniform(24), 1, circle=True, force_tiled=True, tag="-seg45")
    # discs with points on the circle: (0.6, 0.8) is a pixel centre at W = 11 and 71; fp32 rounds 0.6^2 + 0.8^2 to 1, a fused
    # multiply-add to 1 + 2^-23 (those pixels are inside the reference's mask)
    for gather in (False, True):
        _par(cases, 11, uniform(24), 3, circle=True, gather=gather, force_tiled=True, tag="-on-circle")
    _par(cases, 2, uniform(8), 1, force_tiled=True, tag="-smallest")
    _par(cases, 2, uniform(5), 2, circle=True, force_tiled=True, tag="-smallest")
    _par(cases, 2, uniform(8), 1, gather=True, tag="-smallest")
    for W, circle in ((44, False), (46, False), (63, True), (64, True), (65, True), (47, True), (48, True), (31, False)):
        _par(cases, W, uniform(24), 2, circle=circle, force_tiled=True, tag="-edge")
    # ---- normalisation: scale and a device norm scalar (tiled), scale (gather)
    _par(cases, 40, uniform(30), 2, scale=0.37, norm=13.5, force_tiled=True, tag="-norm")
    _par(cases, 40, uniform(30), 2, circle=True, scale=2.5, gather=True, tag="-scale")
    # ---- device only: config 3 and larger geometries, G = 4096 / 4097, the packs' grid-stride loops
    _par(cases, 512, uniform(720), 8, emu=False, kw_expect=8, subset=True, tag="-cfg3")
    _par(cases, 512, uniform(720), 3, circle=True, emu=False, kw_expect=8, subset=True, norm=7.25)
    _par(cases, 1024, uniform(720), 2, emu=False, kw_expect=4, subset=True, tag="-kw4")
    _par(cases, 2896, uniform(720), 1, emu=False, subset=True, tag="-G4096")
    _par(cases, 2896, (0., 0.25, 0.5, 0.75, 44.9, 45., 45.1, 45.2, 89.75, 90., 90.25, 90.5), 1, force_tiled=True, kw_force=4,
         kw_expect=4, emu=False, subset=True, tag="-G4096-forced")
    _par(cases, 2897, uniform(12), 1, emu=False, subset=True, tag="-G4097")
    _par(cases, 4097, BORDERS, 2, circle=True, emu=False, subset=True, tag="-G4097")
    _par(cases, 512, uniform(720), 256, emu=False, kw_expect=8, subset=True, tag="-gridstride")
    _par(cases, 512, uniform(720), 264, gather=True, emu=False, subset=True, tag="-gridstride")
    # ---- interpolating back-projection
    for W, A, circle in ((16, 2, False), (16, 2, True), (33, 90, False), (32, 60, True), (2, 1, False), (11, 24, True)):
        cases.append(Case(f"bp-W{W}{'c' if circle else ''}-A{A}", "bp", True, W=W, angles=uniform(A), circle=circle, n_img=3))
    cases.append(Case("bp-W512-A720", "bp", False, W=512, angles=uniform(720), n_img=2))
    # ---- fan beam, NB 1 / 2 / 4 / 8, detector counts below and above G
    for n, (W, circle, fan) in zip((1, 2, 5, 9, 3), ((16, False, FAN_A), (24, True, FAN_FINE), (31, False, FAN_A),
                                                 (24, False, FAN_FINE), (11, True, FAN_A))):
        g = FanGeom((0.,), W, circle, fan)
        cases.append(Case(f"fan-W{W}{'c' if circle else ''}-det{g.n_det}-{'above' if g.n_det > g.G else 'below'}G-n{n}",
                          "fan", True, W=W, angles=uniform(10, 360.0), circle=circle, n_img=n, fan=fan))
    cases.append(Case("fan-W3c-det16375-lds-edge", "fan", True, W=3, angles=(0., 77.), circle=True, n_img=1,
                      fan={"pixel_spacing": 0.25, "source_radius": 1.0, "detector_radius": 1.0, "n_detector_pixels": 16375,
                           "detector_spacing": 0.0001}))
    # ---- ramp filter: P = 64 at N = 1 and 32, CT = 8 with a column tail, thousands of short columns (the tail of the per-column
    # error), CT = 2 at N = 1025 / 2048, CT = 1 at 2049 / 4096, the direct kernel at N = 4097 and at its 64 KiB limit; odd, even
    # and single angle columns
    for N, A, n, direct, emu in ((1, 1, 1, False, True), (32, 5, 2, False, True), (33, 2, 1, False, True),
                                 (91, 45, 2, False, True), (200, 16, 1, False, True), (60, 17, 3, False, True),
                                 (3, 3, 4000, False, True), (7, 5, 2000, False, True),
                                 (1025, 3, 1, False, True), (2048, 4, 2, False, True), (2049, 3, 1, False, True),
                                 (4096, 1, 1, False, True), (23, 16, 2, True, True), (4097, 2, 1, False, True),
                                 (725, 720, 3, False, False), (4096, 37, 3, False, False), (1025, 720, 2, False, False),
                                 (16384, 3, 1, False, False), (2048, 720, 8, True, False)):
        P = ramp_padded(N)
        path = "direct" if direct or P > RAMP_FFT_MAX_P else f"fft-ct{ramp_ct(P)}"
        cases.append(Case(f"ramp-{path}-N{N}-A{A}-n{n}", "ramp", emu, n_img=n, N=N, A_ramp=A, direct=direct))
    # ---- rejections: an error, no launch, the output untouched
    for what in ("tiled-G4097-fwd", "tiled-G4097-adj", "plan-mismatch", "bad-kw", "ws-small-tiled-fwd", "ws-small-tiled-adj",
                 "ws-small-gather-fwd", "ws-small-gather-adj", "ramp-P", "ramp-plan", "ramp-alias-fft", "ramp-alias-direct",
                 "ramp-65536-fft", "ramp-65536-direct", "ramp-direct-N16385", "bp-65536", "gather-adj-lds",
                 "fan-fwd-lds", "fan-adj-lds"):
        cases.append(Case(f"reject-{what}", "reject", True, reject=what))
    ids = [c.id for c in cases]
    assert len(ids) == len(set(ids)), "duplicate case ids"
    return cases


CASES = build_cases()


# ------------------------------------------------------------------ the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.radon), `device` of its
    buffers, `stream()` -> the stream argument, `fft_plan(n)` -> (plan struct, host table), and - on the emulation -
    `launches()`, the instantiations launched since `reset()`"""

    def __init__(self, lib, device, stream, fft_plan=None, reset=None, launches=None):
        self.lib, self.device, self._stream, self.fft_plan = lib, torch.device(device), stream, fft_plan
        self.reset, self.launches = reset, launches
        self.keep = []

    def dev(self, t):
        """a device copy kept alive until the next case: a pointer handed to the library must outlive the launch"""
        d = t.contiguous().to(self.device)
        self.keep.append(d)
        return d

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def err(self):
        return self.lib.dinv_last_error().decode()

    def expect(self, name, want):
        if self.launches is not None and want is not None:
            got = self.launches()
            assert got == want, f"{name}: launched {got}, the restated dispatch expects {want}"

    def call(self, name, *args, expect=None):
        if self.reset:
            self.reset()
        rc = getattr(self.lib, name)(*args)
        self.expect(name, expect)
        return rc

    def run(self, name, *args, expect=None):
        rc = self.call(name, *args, expect=expect)
        if rc != 0:
            raise RuntimeError(f"{name} error {rc}: {self.err()}")

    def ws(self, nbytes):
        return torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device=self.device)

    def plan(self, geo, n_img, kw=0):
        pl, blob = geo.plan_host(self.lib, n_img, kw)
        return pl, self.dev(blob[:pl.blob_words])

    def ramp_tables(self, N):
        """(P, fft plan, device table, device filter) as radon.py _ramp_tables builds them"""
        P = int(self.lib.dinv_radon_ramp_padded_size(ctypes.c_int32(N)))
        plan, table_host = self.fft_plan(P)
        filt = torch.zeros(P, dtype=torch.float32)
        rc = self.lib.dinv_radon_ramp_filter_init(ctypes.c_int32(P), ctypes.c_void_p(table_host.data_ptr()),
                                                  ctypes.c_void_p(filt.data_ptr()))
        assert rc == 0, self.err()
        return P, plan, self.dev(table_host), self.dev(filt)


def _p(t):
    return ctypes.c_void_p(0 if t is None else (t if isinstance(t, int) else t.data_ptr()))


def _sz(n):
    return ctypes.c_size_t(int(n))


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
    return bits.view(torch.float32)


def run_case(r, case):
    """runs `case` on runner `r`, asserts everything it checks and returns the worst error ratio of each operation"""
    gen = torch.Generator().manual_seed(_seed(case))
    r.keep.clear()
    return {"par": _run_par, "bp": _run_bp, "fan": _run_fan, "ramp": _run_ramp, "reject": _run_reject}[case.kind](r, case, gen)


def _rows(case):
    """images checked against fp64: all, or for a large batch the first image and the last (ragged) group"""
    n = case.n_img
    if not case.subset or n <= 2:
        return list(range(n))
    nb = nb_of(n)
    last = (n - 1) // nb * nb
    return sorted({0} | set(range(last, n)))


def _angle_subset(case, gen):
    """every angle within 0.3 degrees of a multiple of 45 (the class borders) plus a fixed random set"""
    A = case.geo.A
    if not case.subset:
        return list(range(A))
    ang = torch.tensor(case.angles, dtype=torch.float64)
    near = ((ang / 45.0 - torch.round(ang / 45.0)).abs() * 45.0 <= 0.3).nonzero().flatten().tolist()
    k = 2 if case.geo.G >= 4096 else 5
    near = near[::3] if case.geo.G >= 4096 else near
    rnd = torch.randperm(A, generator=gen)[:k].tolist()
    return sorted(set(near) | set(rnd))


def _pixel_subset(case, gen):
    """every tile-border row and column (tiles of 16) of a band of the image plus random pixels; None: all"""
    W = case.geo.W
    if not case.subset:
        return None
    lines = [15, 16] if W > 2048 else [15, 16, 31, 32, W - 1]
    r0 = int(torch.randint(0, W, (1,), generator=gen)) // 16 * 16
    sel = set()
    for l in lines:
        span = range(0, W, 1 if W <= 600 else 3)
        sel.update(l * W + c for c in span)                     # a tile-border row
        sel.update(r * W + l for r in span)                     # a tile-border column
        sel.update((r0 + l % 16) * W + c for c in range(0, W, 7))
    sel.update(torch.randint(0, W * W, (400,), generator=gen).tolist())
    return torch.tensor(sorted(sel))


def _par_measure(geo, M, T):
    return U * geo.G * M + ulp(geo.G) * T


def _adj_measure(geo, m, T):
    return U * geo.A * m + ulp(geo.G) * T


def _run_par(r, case, gen):
    geo = case.geo
    n, G, A, W = case.n_img, geo.G, geo.A, geo.W
    x = torch.randn(n, W, W, generator=gen)
    v = torch.randn(n, G, A, generator=gen)
    xd, vd = r.dev(x), r.dev(v)
    norm = r.dev(torch.tensor([case.norm])) if case.norm else None
    errs = {}
    # forward
    kw = 0
    pl = blob = None
    if G <= TILED_MAX_GRID and not case.gather:
        pl, blob = r.plan(geo, n, case.kw_force)
        kw = pl.kw
        assert (pl.n_chunks_plain, pl.n_chunks_swap) == expected_chunks(geo, kw)
    if case.kw_expect:
        assert kw == case.kw_expect, f"the plan has kw = {kw}, the case is meant for kw = {case.kw_expect}"
    tiled_f = forward_is_tiled(case, kw)
    if tiled_f and not case.subset:
        assert min(plan_slack(geo, pl, blob)) >= 1, "a tap without one column of margin inside its planned window"
    want = expected_launches(case, "fwd", kw)
    d = geo.desc(n, case.scale)
    y = Guarded(n * G * A, r.device)
    if tiled_f:
        ws = r.ws(r.lib.dinv_radon_tiled_workspace_bytes(ctypes.byref(d), 0))
        call = lambda: r.run("dinv_radon_forward_tiled", ctypes.byref(d), ctypes.byref(pl), _p(blob), _p(xd), _p(r.dev(geo.xn)),
                             _p(r.dev(geo.cs)), _p(norm), _p(y.t), _p(ws), _sz(ws.numel()), r._stream(), expect=want)
    else:
        ws = r.ws(r.lib.dinv_radon_workspace_bytes(ctypes.byref(d), 0))
        call = lambda: r.run("dinv_radon_forward", ctypes.byref(d), _p(xd), _p(r.dev(geo.xn)), _p(r.dev(geo.cs)), _p(y.t),
                             _p(ws), _sz(ws.numel()), r._stream(), expect=want)
    call()
    if r.launches is not None and tiled_f:
        assert not (ctypes.c_int.in_dll(r.lib, "dinv_emu_window_misses").value), "a tap outside the planned window"
    fwd_bits = _check_buffer(r, "forward", y, call)
    del ws
    k = case.scale / (case.norm if (case.norm and tiled_f) else 1.0)
    rows = _rows(case)
    angs = _angle_subset(case, gen)
    yr, M, T = ref_forward(geo, x[rows], angs)
    got = fwd_bits.view(n, G, A)[rows][:, :, angs]
    errs["fwd"] = worst_ratio(got, yr * k, _par_measure(geo, M, T) * abs(k))
    key = "fwd_tiled" if tiled_f else "fwd_gather"
    assert errs["fwd"] <= BOUNDS[key], f"forward: worst |y - y64| / measure {errs['fwd']:.3g} > {BOUNDS[key]}"
    # adjoint
    tiled_a = adjoint_is_tiled(case)
    want = expected_launches(case, "adj")
    xt = Guarded(n * W * W, r.device)
    if tiled_a:
        ws = r.ws(r.lib.dinv_radon_tiled_workspace_bytes(ctypes.byref(d), 1))
        call = lambda: r.run("dinv_radon_adjoint_tiled", ctypes.byref(d), _p(vd), _p(r.dev(geo.xn)), _p(r.dev(geo.cs)), _p(norm),
                             _p(xt.t), _p(ws), _sz(ws.numel()), r._stream(), expect=want)
    else:
        ws = r.ws(r.lib.dinv_radon_workspace_bytes(ctypes.byref(d), 1))
        call = lambda: r.run("dinv_radon_adjoint", ctypes.byref(d), _p(vd), _p(r.dev(geo.xn)), _p(r.dev(geo.cs)), _p(xt.t),
                             _p(ws), _sz(ws.numel()), r._stream(), expect=want)
    call()
    if r.launches is not None and tiled_a:
        assert not (ctypes.c_int.in_dll(r.lib, "dinv_emu_segment_misses").value), "a tap outside the staged segment"
    adj_bits = _check_buffer(r, "adjoint", xt, call)
    del ws
    ka = case.scale / (case.norm if (case.norm and tiled_a) else 1.0)
    pix = _pixel_subset(case, gen)
    xr, m, Ta = ref_adjoint(geo, v[rows], pix)
    got = adj_bits.view(n, W * W)[rows]
    got = got if pix is None else got[:, pix]
    errs["adj"] = worst_ratio(got, xr * ka, _adj_measure(geo, m, Ta) * abs(ka))
    key = "adj_tiled" if tiled_a else "adj_gather"
    assert errs["adj"] <= BOUNDS[key], f"adjoint: worst |x - x64| / measure {errs['adj']:.3g} > {BOUNDS[key]}"
    # dot test of the pair in fp64 (the scales of both sides divided out)
    lhs = rhs = ny = nv = 0.0
    disc = geo.disc().double()
    for b in range(n):                      # image by image: the large batches stay within memory
        yy, vv = fwd_bits.view(n, G, A)[b].double() / k, v[b].double()
        xx = adj_bits.view(n, W, W)[b].double() / ka
        lhs += float((yy * vv).sum())
        rhs += float((x[b].double() * disc * xx).sum())
        ny += float((yy * yy).sum())
        nv += float((vv * vv).sum())
    dot = abs(lhs - rhs) / max(math.sqrt(ny * nv), 1e-300)
    errs["dot"] = dot
    assert dot <= DOT_BOUND, f"dot test {dot:.3g}"
    assert torch.equal(xd.cpu(), x) and torch.equal(vd.cpu(), v), "the calls modified their input"
    return errs


def _run_bp(r, case, gen):
    geo = case.geo
    n, G, A, W = case.n_img, geo.G, geo.A, geo.W
    v = torch.randn(n, G, A, generator=gen)
    vd = r.dev(v)
    d = geo.desc(n, case.scale)
    out = Guarded(n * W * W, r.device)
    call = lambda: r.run("dinv_radon_backproject", ctypes.byref(d), _p(vd), _p(r.dev(geo.xn)), _p(r.dev(geo.cs)),
                         _p(r.dev(geo.ixtab)), _p(out.t), r._stream(), expect=expected_launches(case, "bp"))
    call()
    bits = _check_buffer(r, "back-projection", out, call)
    xr, m, T = ref_backproject(geo, v)
    e = worst_ratio(bits.view(n, W, W), xr, U * A * m + ulp(G) * T)
    assert e <= BOUNDS["backproject"], f"back-projection: worst ratio {e:.3g}"
    return {"bp": e}


def _run_fan(r, case, gen):
    geo = case.geo
    n, G, A, W, D = case.n_img, geo.G, geo.A, geo.W, geo.n_det
    x = torch.randn(n, W, W, generator=gen)
    v = torch.randn(n, D, A, generator=gen)
    xd, vd = r.dev(x), r.dev(v)
    d = geo.desc(n, 1.0)
    tabs = [r.dev(t) for t in (geo.xm, geo.sc, geo.yd, geo.cs)]
    y = Guarded(n * D * A, r.device)
    ws = r.ws(r.lib.dinv_radon_fan_workspace_bytes(ctypes.byref(d), ctypes.c_int32(D), ctypes.c_int32(0)))
    call = lambda: r.run("dinv_radon_fan_forward", ctypes.byref(d), ctypes.c_int32(D), _p(xd), *[_p(t) for t in tabs], _p(y.t),
                         _p(ws), _sz(ws.numel()), r._stream(), expect=expected_launches(case, "fan_fwd"))
    call()
    fb = _check_buffer(r, "fan forward", y, call)
    yr, M, T = ref_fan_forward(geo, x)
    errs = {"fwd": worst_ratio(fb.view(n, D, A), yr, U * G * M + ulp(G) * T)}
    assert errs["fwd"] <= BOUNDS["fan_fwd"], f"fan forward: worst ratio {errs['fwd']:.3g}"
    xt = Guarded(n * W * W, r.device)
    ws = r.ws(r.lib.dinv_radon_fan_workspace_bytes(ctypes.byref(d), ctypes.c_int32(D), ctypes.c_int32(1)))
    call = lambda: r.run("dinv_radon_fan_adjoint", ctypes.byref(d), ctypes.c_int32(D), _p(vd), *[_p(t) for t in tabs], _p(xt.t),
                         _p(ws), _sz(ws.numel()), r._stream(), expect=expected_launches(case, "fan_adj"))
    call()
    ab = _check_buffer(r, "fan adjoint", xt, call)
    xr, m, Ta = ref_fan_adjoint(geo, v)
    errs["adj"] = worst_ratio(ab.view(n, W, W), xr, U * A * m + ulp(G) * Ta)
    assert errs["adj"] <= BOUNDS["fan_adj"], f"fan adjoint: worst ratio {errs['adj']:.3g}"
    yy, xx = fb.double().view(n, D, A), ab.double().view(n, W, W)
    lhs, rhs = float((yy * v.double()).sum()), float((x.double() * geo.disc().double() * xx).sum())
    errs["dot"] = abs(lhs - rhs) / max(float(yy.norm() * v.double().norm()), 1e-300)
    assert errs["dot"] <= DOT_BOUND, f"dot test {errs['dot']:.3g}"
    return errs


def _run_ramp(r, case, gen):
    n, N, A = case.n_img, case.N, case.A_ramp
    y = torch.randn(n, N, A, generator=gen)
    yd = r.dev(y)
    out = Guarded(n * N * A, r.device)
    want = expected_launches(case, "ramp")
    P = ramp_padded(N)
    assert int(r.lib.dinv_radon_ramp_padded_size(ctypes.c_int32(N))) == P
    fft = P <= RAMP_FFT_MAX_P and not case.direct
    if fft:
        P, plan, table, filt = r.ramp_tables(N)
        call = lambda: r.run("dinv_radon_ramp_fft", ctypes.c_int32(n), ctypes.c_int32(N), ctypes.c_int32(A), ctypes.c_int32(P),
                             ctypes.byref(plan), _p(table), _p(filt), _p(yd), _p(out.t), r._stream(), expect=want)
    else:
        call = lambda: r.run("dinv_radon_ramp", ctypes.c_int32(n), ctypes.c_int32(N), ctypes.c_int32(A), _p(yd), _p(out.t),
                             r._stream(), expect=want)
    call()
    bits = _check_buffer(r, "ramp", out, call).view(n, N, A)
    ref = ref_ramp(y)
    if fft:
        e = ramp_fft_ratio(bits, y, P)
    else:
        e = worst_ratio(bits, ref, U * N * ref_ramp(y, absolute=True))
    key = "ramp_fft" if fft else "ramp_direct"
    assert e <= BOUNDS[key], f"ramp: worst ratio {e:.3g} > {BOUNDS[key]}"
    return {"ramp": e}


# ------------------------------------------------------------------ rejections
def _run_reject(r, case, gen):
    """the entry point returns an error, launches nothing and leaves its (poisoned) output alone; every buffer has its true
    size (a workspace one byte short of what the call needs is a real allocation of that size)"""
    what = case.reject
    fdev = lambda n: r.dev(torch.randn(int(n), generator=gen))
    out = None
    args = None
    msg = None
    if what.startswith("tiled-G4097"):
        geo = RadonGeom((0., 30.), 2897, False)
        assert geo.G == 4097
        d = geo.desc(1, 1.0)
        out = Guarded(geo.G * geo.A if what.endswith("fwd") else geo.W * geo.W, r.device)
        src = fdev(geo.W * geo.W if what.endswith("fwd") else geo.G * geo.A)
        ws = r.ws(1 << 20)
        pl = RadonPlan()
        pl.grid, pl.n_angles, pl.kw = geo.G, geo.A, 1
        if what.endswith("fwd"):
            name, args = "dinv_radon_forward_tiled", (ctypes.byref(d), ctypes.byref(pl), _p(ws), _p(src), _p(r.dev(geo.xn)),
                                                      _p(r.dev(geo.cs)), _p(None), _p(out.t), _p(ws), _sz(ws.numel()))
        else:
            name, args = "dinv_radon_adjoint_tiled", (ctypes.byref(d), _p(src), _p(r.dev(geo.xn)), _p(r.dev(geo.cs)), _p(None),
                                                      _p(out.t), _p(ws), _sz(ws.numel()))
        msg = "above the tiled kernels' limit"
        assert r.lib.dinv_radon_tiled_workspace_bytes(ctypes.byref(d), ctypes.c_int32(0)) == 0
    elif what in ("plan-mismatch", "bad-kw", "ws-small-tiled-fwd"):
        geo = RadonGeom(uniform(12), 20, False)
        d = geo.desc(2, 1.0)
        other = RadonGeom(uniform(13), 20, False)
        pl, blob = r.plan(other if what == "plan-mismatch" else geo, 2)
        need = r.lib.dinv_radon_tiled_workspace_bytes(ctypes.byref(d), 0)
        ws = r.ws(need - 1 if what == "ws-small-tiled-fwd" else need)
        if what == "bad-kw":
            pl.kw = 3
        out = Guarded(2 * geo.G * geo.A, r.device)
        name = "dinv_radon_forward_tiled"
        args = (ctypes.byref(d), ctypes.byref(pl), _p(blob), _p(fdev(2 * geo.W * geo.W)), _p(r.dev(geo.xn)), _p(r.dev(geo.cs)),
                _p(None), _p(out.t), _p(ws), _sz(ws.numel()))
        msg = {"plan-mismatch": "plan does not match", "bad-kw": "bad plan", "ws-small-tiled-fwd": "workspace too small"}[what]
    elif what in ("ws-small-tiled-adj", "ws-small-gather-fwd", "ws-small-gather-adj"):
        geo = RadonGeom(uniform(12), 20, True)
        d = geo.desc(3, 1.0)
        adj = what.endswith("adj")
        fn = r.lib.dinv_radon_tiled_workspace_bytes if "tiled" in what else r.lib.dinv_radon_workspace_bytes
        ws = r.ws(fn(ctypes.byref(d), ctypes.c_int32(int(adj))) - 1)
        out = Guarded(3 * (geo.W * geo.W if adj else geo.G * geo.A), r.device)
        src = fdev(3 * (geo.G * geo.A if adj else geo.W * geo.W))
        tabs = (_p(r.dev(geo.xn)), _p(r.dev(geo.cs)))
        if what == "ws-small-tiled-adj":
            name, args = "dinv_radon_adjoint_tiled", (ctypes.byref(d), _p(src), *tabs, _p(None), _p(out.t), _p(ws), _sz(ws.numel()))
        else:
            name = "dinv_radon_adjoint" if adj else "dinv_radon_forward"
            args = (ctypes.byref(d), _p(src), *tabs, _p(out.t), _p(ws), _sz(ws.numel()))
        msg = "workspace too small"
    elif what.startswith("ramp"):
        N, A, n = (16385, 1, 1) if what == "ramp-direct-N16385" else (40, 3, 65536 if "65536" in what else 2)
        src = fdev(n * N * A)
        out = Guarded(n * N * A, r.device)
        oarg = src if "alias" in what else out.t
        if what.endswith("direct") or what == "ramp-direct-N16385":
            name, args = "dinv_radon_ramp", (ctypes.c_int32(n), ctypes.c_int32(N), ctypes.c_int32(A), _p(src), _p(oarg))
        else:
            P, plan, table, filt = r.ramp_tables(N)
            if what == "ramp-plan":
                plan, table = r.fft_plan(P * 2)[0], table
            Parg = P * 2 if what == "ramp-P" else P
            name, args = "dinv_radon_ramp_fft", (ctypes.c_int32(n), ctypes.c_int32(N), ctypes.c_int32(A), ctypes.c_int32(Parg),
                                                 ctypes.byref(plan), _p(table), _p(filt), _p(src), _p(oarg))
        msg = {"alias": "aliased", "65536": "too many sinograms", "N16385": "detector axis too long", "ramp-P": "plan does not",
               "ramp-plan": "plan does not"}
        msg = next(v for k, v in msg.items() if k in what)
    elif what == "bp-65536":
        geo = RadonGeom((10.,), 2, False)
        n = 65536
        d = geo.desc(n, 1.0)
        out = Guarded(n * geo.W * geo.W, r.device)
        name, args = "dinv_radon_backproject", (ctypes.byref(d), _p(fdev(n * geo.G * geo.A)), _p(r.dev(geo.xn)),
                                                _p(r.dev(geo.cs)), _p(r.dev(geo.ixtab)), _p(out.t))
        msg = "too many images"
    elif what == "gather-adj-lds":
        # (ceil(G / 2) * 2) * 4 + A * 8 > 64 KiB: G = 4097 with 6144 angles (6143 fit)
        geo = RadonGeom(uniform(6144), 4097, True)
        d = geo.desc(1, 1.0)
        assert ((geo.G + 1) // 2 * 2) * 4 + 6143 * 8 <= GATHER_LDS < ((geo.G + 1) // 2 * 2) * 4 + geo.A * 8
        ws = r.ws(r.lib.dinv_radon_workspace_bytes(ctypes.byref(d), ctypes.c_int32(1)))
        out = Guarded(geo.W * geo.W, r.device)
        name, args = "dinv_radon_adjoint", (ctypes.byref(d), _p(fdev(geo.G * geo.A)), _p(r.dev(geo.xn)), _p(r.dev(geo.cs)),
                                            _p(out.t), _p(ws), _sz(ws.numel()))
        msg = "too many angles/detectors"
    elif what.startswith("fan"):
        if what == "fan-fwd-lds":      # 2 G floats of LDS tables: G = 8193 is one past 64 KiB
            geo = FanGeom((0., 40.), 8193, True, {"n_detector_pixels": 4})
            D = geo.n_det
            adj = False
        else:                          # 3 G + n_det floats: n_det = 16376 at G = 3 is one past 64 KiB (16375: the edge case)
            geo = FanGeom((0., 40.), 3, True, {"n_detector_pixels": 16376})
            D = geo.n_det
            adj = True
        d = geo.desc(1, 1.0)
        ws = r.ws(r.lib.dinv_radon_fan_workspace_bytes(ctypes.byref(d), ctypes.c_int32(D), ctypes.c_int32(int(adj))))
        out = Guarded(geo.W * geo.W if adj else D * geo.A, r.device)
        src = fdev(D * geo.A if adj else geo.W * geo.W)
        name = "dinv_radon_fan_adjoint" if adj else "dinv_radon_fan_forward"
        args = (ctypes.byref(d), ctypes.c_int32(D), _p(src), *[_p(r.dev(t)) for t in (geo.xm, geo.sc, geo.yd, geo.cs)],
                _p(out.t), _p(ws), _sz(ws.numel()))
        msg = "LDS tables"
    else:
        raise ValueError(what)
    rc = r.call(name, *args, r._stream(), expect=[])
    assert rc != 0, f"{name} accepted a call it must reject ({case.id})"
    got = r.err()
    assert msg in got, f"rejected for '{got}', the case expects '{msg}'"
    r.sync()
    assert out.untouched(), f"{name}: a rejected call wrote to its output"
    return {}


def run_empty(r):
    """B * C = 0: every entry point returns 0, launches nothing and writes nothing"""
    geo = RadonGeom(uniform(12), 20, False)
    d = geo.desc(0, 1.0)
    out = Guarded(16, r.device)
    dummy = r.dev(torch.zeros(16))
    pl, blob = r.plan(geo, 1)
    tabs = (_p(r.dev(geo.xn)), _p(r.dev(geo.cs)))
    calls = [("dinv_radon_forward_tiled", (ctypes.byref(d), ctypes.byref(pl), _p(blob), _p(dummy), *tabs, _p(None), _p(out.t),
                                           _p(dummy), _sz(0))),
             ("dinv_radon_adjoint_tiled", (ctypes.byref(d), _p(dummy), *tabs, _p(None), _p(out.t), _p(dummy), _sz(0))),
             ("dinv_radon_forward", (ctypes.byref(d), _p(dummy), *tabs, _p(out.t), _p(dummy), _sz(0))),
             ("dinv_radon_adjoint", (ctypes.byref(d), _p(dummy), *tabs, _p(out.t), _p(dummy), _sz(0))),
             ("dinv_radon_backproject", (ctypes.byref(d), _p(dummy), *tabs, _p(r.dev(geo.ixtab)), _p(out.t))),
             ("dinv_radon_ramp", (ctypes.c_int32(0), ctypes.c_int32(7), ctypes.c_int32(3), _p(dummy), _p(out.t)))]
    fg = FanGeom(uniform(4), 20, False)
    ftabs = [_p(r.dev(t)) for t in (fg.xm, fg.sc, fg.yd, fg.cs)]
    fd = fg.desc(0, 1.0)
    for name in ("dinv_radon_fan_forward", "dinv_radon_fan_adjoint"):
        calls.append((name, (ctypes.byref(fd), ctypes.c_int32(fg.n_det), _p(dummy), *ftabs, _p(out.t), _p(dummy), _sz(0))))
    P, plan, table, filt = r.ramp_tables(7)
    calls.append(("dinv_radon_ramp_fft", (ctypes.c_int32(0), ctypes.c_int32(7), ctypes.c_int32(3), ctypes.c_int32(P),
                                          ctypes.byref(plan), _p(table), _p(filt), _p(dummy), _p(out.t))))
    for name, args in calls:
        rc = r.call(name, *args, r._stream(), expect=[])
        assert rc == 0, f"{name} with no images: error {r.err()}"
    r.sync()
    assert out.untouched()
