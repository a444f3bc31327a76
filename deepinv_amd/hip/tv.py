"""ctypes wrappers of csrc/tv.hip: the fused Chambolle-Pock iteration of TVDenoiser / TVL1Denoiser, the finite differences and
their adjoint, and TVPrior.fn / grad (include/deepinv_amd.h, "Total variation").  Every launch goes to the current stream of
the operands' device.  fp32 contiguous operands; the callers (models/tv.py, optim/prior.py) validate them."""
from __future__ import annotations

import ctypes

import torch

from . import check, declare_once, lib, ptr, require_hip, stream_ptr


def _declare(l):
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    l.dinv_tv_cp_partials.restype = i32
    l.dinv_tv_cp_partials.argtypes = [i64]
    l.dinv_tv_cp_iter.argtypes = [i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, f32, f32, f32, f32, vp, vp, vp]
    for name in ("dinv_tv_nabla", "dinv_tv_nabla_adjoint", "dinv_tv_grad"):
        getattr(l, name).argtypes = [i32, i64, i32, i32, i32, vp, vp, vp]
    l.dinv_tv_fn_blocks.restype = i32
    l.dinv_tv_fn_blocks.argtypes = [i64]
    l.dinv_tv_fn.argtypes = [i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]


def _l():
    return declare_once(lib(), _declare)


def geometry(shape) -> tuple[int, int, int, int, int, int]:
    """(nd, batch, channels, D, H, W) of an image shape [B, C, H, W] or [B, C, D, H, W]"""
    if len(shape) == 4:
        return 2, shape[0], shape[1], 1, shape[2], shape[3]
    if len(shape) == 5:
        return 3, shape[0], shape[1], shape[2], shape[3], shape[4]
    raise ValueError(f"TV operators take [B,C,H,W] or [B,C,D,H,W] tensors, got shape {tuple(shape)}")


class CPState:
    """The device state of one prox call: two ping-pong (x2, u2) pairs, the reduction partials and the int32 pair
    (done, iterations run)."""

    def __init__(self, y, x2, u2, lam, aniso: bool, tau: float, sigma: float, rho: float, crit: float):
        require_hip(y, x2, u2, lam)
        self.geo = geometry(y.shape)
        self.y, self.lam = y, lam
        self.x = (x2, torch.empty_like(x2))
        self.u = (u2, torch.empty_like(u2))
        self.partial = torch.empty(2 * _l().dinv_tv_cp_partials(y.numel()), device=y.device, dtype=torch.float32)
        self.state = torch.zeros(2, device=y.device, dtype=torch.int32)
        self.args = (1 if aniso else 0, float(tau), float(sigma), float(rho), float(crit))

    def step(self):
        """one iteration (a no-op on the device once the stopping test has fired)"""
        nd, B, C, D, H, W = self.geo
        aniso, tau, sigma, rho, crit = self.args
        check(_l().dinv_tv_cp_iter(nd, B, C, D, H, W, ptr(self.x[0]), ptr(self.x[1]), ptr(self.u[0]), ptr(self.u[1]),
                                   ptr(self.y), ptr(self.lam), aniso, tau, sigma, rho, crit, ptr(self.partial),
                                   ptr(self.state), stream_ptr(self.y.device)))

    def result(self):
        """(x2, u2, iterations run, stopping test fired): reads the device state (one host synchronisation)"""
        done, it = self.state.tolist()
        return self.x[it & 1], self.u[it & 1], it, bool(done)


def nabla(x):
    nd, B, C, D, H, W = geometry(x.shape)
    require_hip(x)
    out = torch.empty((*x.shape, nd), device=x.device, dtype=torch.float32)
    check(_l().dinv_tv_nabla(nd, B * C, D, H, W, ptr(x), ptr(out), stream_ptr(x.device)))
    return out


def nabla_adjoint(v):
    if v.dim() not in (5, 6) or v.shape[-1] != v.dim() - 3:
        raise ValueError(f"nabla_adjoint takes a [B,C,H,W,2] or [B,C,D,H,W,3] field, got shape {tuple(v.shape)}")
    nd, B, C, D, H, W = geometry(v.shape[:-1])
    require_hip(v)
    out = torch.empty(v.shape[:-1], device=v.device, dtype=torch.float32)
    check(_l().dinv_tv_nabla_adjoint(nd, B * C, D, H, W, ptr(v), ptr(out), stream_ptr(v.device)))
    return out


def grad(x):
    nd, B, C, D, H, W = geometry(x.shape)
    require_hip(x)
    out = torch.empty_like(x)
    check(_l().dinv_tv_grad(nd, B * C, D, H, W, ptr(x), ptr(out), stream_ptr(x.device)))
    return out


def fn(x, l1: bool = False):
    nd, B, C, D, H, W = geometry(x.shape)
    require_hip(x)
    out = torch.empty(B, device=x.device, dtype=torch.float32)
    part = torch.empty(B * _l().dinv_tv_fn_blocks(x.numel() // B), device=x.device, dtype=torch.float32)
    check(_l().dinv_tv_fn(nd, 1 if l1 else 0, B, C, D, H, W, ptr(x), ptr(out), ptr(part), stream_ptr(x.device)))
    return out
