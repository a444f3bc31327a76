"""ctypes wrappers of csrc/tgv.hip: the Chambolle-Pock iteration of TGVDenoiser and the epsilon / epsilon^T pair
(include/deepinv_amd.h, "Total generalized variation").  Every launch goes to the current stream of the operands' device.
fp32 contiguous operands; the caller (models/tgv.py) validates them."""
from __future__ import annotations

import ctypes

import torch

from . import check, declare_once, lib, ptr, require_hip, stream_ptr
from .tv import geometry


def _declare(l):
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    l.dinv_tgv_cp_partials.restype = i32
    l.dinv_tgv_cp_partials.argtypes = [i64]
    l.dinv_tgv_cp_iter.argtypes = [i32] * 6 + [vp] * 9 + [f32] * 4 + [vp] * 5
    for name in ("dinv_tgv_epsilon", "dinv_tgv_epsilon_adjoint"):
        getattr(l, name).argtypes = [i32, i64, i32, i32, i32, vp, vp, vp]


def _l():
    return declare_once(lib(), _declare)


class CPState:
    """The device state of one prox call: two ping-pong (x2, r2, u2) sets, the z / w scratch that carries 2x - x2 and
    2r - r2 from the primal launch to the dual one, the reduction partials and the int32 pair (done, iterations run)."""

    def __init__(self, y, x2, r2, u2, lam1, lam2, tau: float, sigma: float, rho: float, crit: float):
        require_hip(y, x2, r2, u2, lam1, lam2)
        self.geo = geometry(y.shape)
        self.y, self.lam1, self.lam2 = y, lam1, lam2
        self.x = (x2, torch.empty_like(x2))
        self.r = (r2, torch.empty_like(r2))
        self.u = (u2, torch.empty_like(u2))
        self.z = torch.empty_like(y)
        self.w = torch.empty_like(r2)
        self.partial = torch.empty(2 * _l().dinv_tgv_cp_partials(y.numel()), device=y.device, dtype=torch.float32)
        self.state = torch.zeros(2, device=y.device, dtype=torch.int32)
        self.args = (float(tau), float(sigma), float(rho), float(crit))

    def step(self):
        """one iteration (a no-op on the device once the stopping test has fired)"""
        nd, B, C, D, H, W = self.geo
        tau, sigma, rho, crit = self.args
        check(_l().dinv_tgv_cp_iter(nd, B, C, D, H, W, ptr(self.x[0]), ptr(self.x[1]), ptr(self.r[0]), ptr(self.r[1]),
                                    ptr(self.u[0]), ptr(self.u[1]), ptr(self.y), ptr(self.lam1), ptr(self.lam2), tau, sigma,
                                    rho, crit, ptr(self.z), ptr(self.w), ptr(self.partial), ptr(self.state),
                                    stream_ptr(self.y.device)))

    def result(self):
        """(x2, r2, u2, iterations run, stopping test fired): reads the device state (one host synchronisation)"""
        done, it = self.state.tolist()
        return self.x[it & 1], self.r[it & 1], self.u[it & 1], it, bool(done)


def epsilon(v):
    if v.dim() not in (5, 6) or v.shape[-1] != v.dim() - 3:
        raise ValueError(f"epsilon takes a [B,C,H,W,2] or [B,C,D,H,W,3] field, got shape {tuple(v.shape)}")
    nd, B, C, D, H, W = geometry(v.shape[:-1])
    require_hip(v)
    out = torch.empty((*v.shape[:-1], nd * nd), device=v.device, dtype=torch.float32)
    check(_l().dinv_tgv_epsilon(nd, B * C, D, H, W, ptr(v), ptr(out), stream_ptr(v.device)))
    return out


def epsilon_adjoint(u):
    if u.dim() not in (5, 6) or u.shape[-1] != (u.dim() - 3) ** 2:
        raise ValueError(f"epsilon_adjoint takes a [B,C,H,W,4] or [B,C,D,H,W,9] field, got shape {tuple(u.shape)}")
    nd, B, C, D, H, W = geometry(u.shape[:-1])
    require_hip(u)
    out = torch.empty((*u.shape[:-1], nd), device=u.device, dtype=torch.float32)
    check(_l().dinv_tgv_epsilon_adjoint(nd, B * C, D, H, W, ptr(u), ptr(out), stream_ptr(u.device)))
    return out
