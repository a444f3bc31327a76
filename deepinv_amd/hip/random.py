"""ctypes wrappers of csrc/random.hip: fused additive Gaussian noise, the Poisson-family noise models and the Cartesian MRI
mask-line generator."""
from __future__ import annotations

import ctypes

import torch

from . import check, declare_once, lib, ptr, require_hip, stream_ptr


def _declare(l):
    vp, i32, i64, u64, f32, f64 = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float,
                                   ctypes.c_double)
    l.dinv_gaussian_noise.argtypes = [i64, i64, vp, vp, f32, u64, u64, vp, vp]
    l.dinv_poisson_noise.argtypes = [i64, i64, vp, vp, f32, vp, f32, i32, i32, f32, u64, u64, vp, vp, vp]
    l.dinv_mri_mask_lines.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, f64, i32, u64, u64, vp, vp]


def _l():
    return declare_once(lib(), _declare)


def philox_state(gen: torch.Generator | None, device, n_blocks: int):
    """(seed, offset) for a kernel that consumes `n_blocks` Philox counters, taken from - and advanced on - the torch
    generator that the reference would have drawn from (the given one, else the device's default generator), so that
    torch.manual_seed / Generator.manual_seed keep their meaning: same seed -> same numbers, successive calls differ."""
    if gen is None:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        gen = torch.cuda.default_generators[idx]
    seed, off = gen.initial_seed(), gen.get_offset()
    gen.set_offset(off + 4 * ((int(n_blocks) + 3) // 4))     # torch keeps Philox offsets in multiples of 4
    return seed & 0xFFFFFFFFFFFFFFFF, off


def gaussian_noise(x: torch.Tensor, sigma, gen: torch.Generator | None = None) -> torch.Tensor:
    """x + sigma * N(0, I) in one pass (sigma: float, 0-dim tensor, or one value per batch sample)"""
    dev = require_hip(x)
    xc = x.contiguous().float()
    y = torch.empty_like(xc)
    n = xc.numel()
    per, sig_t, sig_f = n, None, 0.0
    if isinstance(sigma, torch.Tensor) and sigma.numel() > 1:
        if sigma.numel() != xc.shape[0]:
            raise ValueError(f"sigma has {sigma.numel()} entries for a batch of {xc.shape[0]}")
        sig_t = sigma.reshape(-1).to(dev, torch.float32).contiguous()
        per = n // xc.shape[0]
    elif isinstance(sigma, torch.Tensor):
        if sigma.is_cuda:            # keep a device scalar on the device: one-entry per-"sample" table over the whole tensor
            sig_t = sigma.reshape(1).to(dev, torch.float32)
        else:
            sig_f = float(sigma)
    else:
        sig_f = float(sigma)
    seed, off = philox_state(gen, dev, (n + 3) // 4)
    check(_l().dinv_gaussian_noise(n, max(per, 1), ptr(xc), ptr(sig_t), sig_f, seed, off, ptr(y), stream_ptr(dev)))
    return y


POISSON, POISSON_GAUSSIAN, POISSON_LOG = 0, 1, 2            # include/deepinv_amd.h: DINV_POISSON*
POISSON_NORMALIZE, POISSON_CLIP_POSITIVE = 1, 2


def poisson_eligible(x: torch.Tensor, *params) -> bool:
    """the kernel serves a HIP fp32 tensor outside autograd with scalar or one-per-sample parameters"""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 1) or (torch.is_grad_enabled() and x.requires_grad):
        return False
    for p in params:
        if isinstance(p, torch.Tensor):
            if p.numel() not in (1, x.shape[0]) or (torch.is_grad_enabled() and p.requires_grad):
                return False
    return True


def poisson_noise(x: torch.Tensor, mode: int, gain, sigma=0.0, normalize: bool = False, clip_positive: bool = False,
                  min_gain: float = 0.0, gen: torch.Generator | None = None):
    """One pass of dinv_poisson_noise over x (csrc/random.hip).  gain / sigma: float, one-element tensor or one value per batch
    sample; a tensor that lives on the device stays there (no host read).  In mode POISSON_LOG, `gain` carries N0 and `sigma` mu.
    Returns (y, bad): bad is None under clip_positive or POISSON_LOG, else [negative input seen, non-positive gain seen] - the
    one host read of the call, in place of the reference's torch.any; when either is set the generator is left where it was."""
    dev = require_hip(x)
    xc = x.contiguous().float()
    y = torch.empty_like(xc)
    n = xc.numel()
    B = xc.shape[0]
    tensors = [p for p in (gain, sigma) if isinstance(p, torch.Tensor)]
    for p in tensors:
        if p.numel() not in (1, B):
            raise ValueError(f"a noise parameter has {p.numel()} entries for a batch of {B}")
    rows = B if any(p.numel() > 1 for p in tensors) else 1        # one table row per sample, or one for the whole tensor

    def arg(p):
        if isinstance(p, torch.Tensor) and (p.is_cuda or p.numel() > 1):
            return p.detach().reshape(-1).to(dev, torch.float32).expand(rows).contiguous(), 0.0
        return None, float(p)

    g_t, g_f = arg(gain)
    s_t, s_f = arg(sigma)
    flags = (POISSON_NORMALIZE if normalize else 0) | (POISSON_CLIP_POSITIVE if clip_positive else 0)
    bad = None
    if not clip_positive and mode != POISSON_LOG:
        bad = torch.zeros(2, device=dev, dtype=torch.int32)
    if gen is None:
        gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    seed, off = philox_state(gen, dev, n)                          # element i owns counter off + i
    check(_l().dinv_poisson_noise(n, max(n // max(rows, 1), 1), ptr(xc), ptr(g_t), g_f, ptr(s_t), s_f, int(mode), flags,
                                  float(min_gain), seed, off, ptr(bad), ptr(y), stream_ptr(dev)))
    if bad is not None:
        bad = [bool(v) for v in bad.tolist()]
        if any(bad):
            gen.set_offset(off)
    return y, bad


def mri_mask_lines(batch, channels, times, height, width, n_lines, center, mode, pdf, accel, n_offsets, device,
                   gen: torch.Generator | None = None) -> torch.Tensor:
    """mask [batch, channels, times, height, width] of sampled k-space columns (csrc/random.hip)"""
    device = torch.device(device)
    mask = torch.empty((batch, channels, times, height, width), device=device, dtype=torch.float32)
    require_hip(mask)
    seed, off = philox_state(gen, device, batch * times * 1024 + batch)
    check(_l().dinv_mri_mask_lines(batch, channels, times, height, width, int(n_lines), int(center[0]), int(center[1]), int(mode),
                                   ptr(pdf), float(accel), int(n_offsets), seed, off, ptr(mask), stream_ptr(device)))
    return mask
