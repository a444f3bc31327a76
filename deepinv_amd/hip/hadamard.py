"""ctypes wrappers of csrc/hadamard.hip: the Walsh-Hadamard transform and the fused operators of SinglePixelCamera
(include/deepinv_amd.h, "Walsh-Hadamard transform").  Every launch goes to the current stream of the operands' device.
fp32 only: an input of another dtype raises, it is not cast.  Each call is a ``torch.autograd.Function`` whose backward is the
same library call with the transposed flags, so a network unfolded over the operator trains without leaving the kernels.
The mask is a buffer of the operator: no gradient flows to it."""
from __future__ import annotations

import ctypes

import torch

from . import check, declare_once, lib, ptr, require_hip, stream_ptr

PRE_MASK, PRE_DAGGER = 1, 2
SYM_MASK, SYM_MASK2, SYM_PROX, SYM_PROX_ADJ_Y, SYM_DAGGER = 1 << 4, 2 << 4, 3 << 4, 4 << 4, 5 << 4
SECOND, NO_TRANSFORM, LAST_AXIS, NO_NORMALIZE = 0x100, 0x200, 0x400, 0x800
MAX_SIDE = 1024

# flags of the transposed operator (H2 is symmetric, the symbols are diagonal)
_TRANSPOSE = {SYM_MASK: PRE_MASK, PRE_MASK: SYM_MASK, SYM_MASK2 | SECOND: SYM_MASK2 | SECOND,
              SYM_MASK2 | NO_TRANSFORM: SYM_MASK2 | NO_TRANSFORM, PRE_DAGGER: SYM_DAGGER, SYM_DAGGER: PRE_DAGGER}


def _declare(l):
    vp, i32, i64, f32, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    l.dinv_hadamard_workspace_bytes.restype = sz
    l.dinv_hadamard_workspace_bytes.argtypes = [i64, i32, i32]
    l.dinv_hadamard.argtypes = [vp, vp, i64, i32, i32, i32, f32, vp, sz, vp]
    l.dinv_hadamard_apply.argtypes = [vp, vp, vp, vp, i64, i32, i32, i64, i32, f32, f32, vp, sz, vp]


def _l():
    return declare_once(lib(), _declare)


def _operand(t: torch.Tensor, what: str) -> torch.Tensor:
    """a contiguous, 16-byte aligned fp32 tensor on the HIP device"""
    if t.dtype != torch.float32:
        raise TypeError(f"the Hadamard kernels are fp32: {what} has dtype {t.dtype}; convert it with .float()")
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _sides(shape, last_axis=False):
    if len(shape) < (1 if last_axis else 2):
        raise ValueError(f"expected a tensor with at least {1 if last_axis else 2} dimensions, got shape {tuple(shape)}")
    W = int(shape[-1])
    H = 1 if last_axis else int(shape[-2])
    for n in (H, W):
        if n < 1 or n & (n - 1):
            raise ValueError("n must be a power of 2")
        if n > MAX_SIDE:
            raise ValueError(f"the Hadamard kernels take sides of at most {MAX_SIDE}, got {n}")
    return H, W


def _transform(x, last_axis, normalize):
    require_hip(x)
    H, W = _sides(x.shape, last_axis)
    x = _operand(x, "the input")
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    flags = (LAST_AXIS if last_axis else 0) | (0 if normalize else NO_NORMALIZE)
    check(_l().dinv_hadamard(ptr(x), ptr(out), x.numel() // (H * W), H, W, flags, 1.0, None, 0, stream_ptr(x.device)))
    return out


class _Transform(torch.autograd.Function):
    @staticmethod
    def forward(x, last_axis, normalize):
        return _transform(x, last_axis, normalize)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _, ctx.last_axis, ctx.normalize = inputs

    @staticmethod
    def backward(ctx, g):
        return _Transform.apply(g, ctx.last_axis, ctx.normalize), None, None


def fwht(x: torch.Tensor, last_axis: bool = False, normalize: bool = True) -> torch.Tensor:
    """the natural-order Walsh-Hadamard transform of the last two axes (or of the last one), orthonormal when ``normalize``"""
    return _Transform.apply(x, bool(last_axis), bool(normalize))


def _apply(x, mask, flags, add=0.0, y=None):
    require_hip(x, mask, y)
    if x.dim() < 3 or mask.dim() != x.dim() or tuple(mask.shape[1:]) != tuple(x.shape[1:]) or mask.shape[0] not in (1, x.shape[0]):
        raise ValueError(f"the mask must have shape [1 or B, C, H, W] for an input [B, C, H, W]: got mask {tuple(mask.shape)} "
                         f"for input {tuple(x.shape)}")
    if y is not None and y.shape != x.shape:
        raise ValueError(f"y has shape {tuple(y.shape)}, expected {tuple(x.shape)}")
    H, W = _sides(x.shape)
    x, mask = _operand(x, "the input"), _operand(mask, "the mask")
    y = None if y is None else _operand(y, "y")
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    check(_l().dinv_hadamard_apply(ptr(x), ptr(y), ptr(mask), ptr(out), x.numel() // (H * W), H, W, mask.numel() // (H * W),
                                   flags, float(add), 1.0, None, 0, stream_ptr(x.device)))
    return out


class _Apply(torch.autograd.Function):
    """one linear operator of the table in include/deepinv_amd.h; backward is the transposed one"""

    @staticmethod
    def forward(x, mask, flags):
        return _apply(x, mask, flags)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _, mask, ctx.flags = inputs
        ctx.save_for_backward(mask)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return _Apply.apply(g, mask, _TRANSPOSE[ctx.flags]), None, None


class _Prox(torch.autograd.Function):
    """H2((mask y + H2(z) / gamma) / (mask^2 + 1 / gamma)): linear in (z, y)"""

    @staticmethod
    def forward(z, y, mask, ginv):
        return _apply(z, mask, SYM_PROX | SECOND, ginv, y)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _, _, mask, ctx.ginv = inputs
        ctx.save_for_backward(mask)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        gz = _ProxZ.apply(g, mask, ctx.ginv) if ctx.needs_input_grad[0] else None
        gy = _ProxY.apply(g, mask, ctx.ginv, False) if ctx.needs_input_grad[1] else None
        return gz, gy, None, None


class _ProxZ(torch.autograd.Function):
    """d prox / d z = H2 diag((1 / gamma) / (mask^2 + 1 / gamma)) H2, symmetric"""

    @staticmethod
    def forward(g, mask, ginv):
        return _apply(g, mask, SYM_PROX | SECOND, ginv, None)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _, mask, ctx.ginv = inputs
        ctx.save_for_backward(mask)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return _ProxZ.apply(g, mask, ctx.ginv), None, None


class _ProxY(torch.autograd.Function):
    """(d prox / d y)^T = diag(mask / (mask^2 + 1 / gamma)) H2, or its transpose H2 diag(...) (``transposed``)"""

    @staticmethod
    def forward(g, mask, ginv, transposed):
        if not transposed:
            return _apply(g, mask, SYM_PROX_ADJ_Y, ginv)
        # H2(w g) with w = mask / (mask^2 + 1 / gamma): the prox symbol with z = 0 ... which is the prox call itself at z = 0
        return _apply(torch.zeros_like(g), mask, SYM_PROX | SECOND, ginv, g)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _, mask, ctx.ginv, ctx.transposed = inputs
        ctx.save_for_backward(mask)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return _ProxY.apply(g, mask, ctx.ginv, not ctx.transposed), None, None, None


def forward(x, mask):
    """A x = mask H2(x)"""
    return _Apply.apply(x, mask, SYM_MASK)


def adjoint(y, mask):
    """A^T y = H2(mask y)"""
    return _Apply.apply(y, mask, PRE_MASK)


def adjoint_forward(x, mask):
    """A^T A x = H2(mask^2 H2(x)), the plane crossing HBM once each way where it is resident"""
    return _Apply.apply(x, mask, SYM_MASK2 | SECOND)


def forward_adjoint(y, mask):
    """A A^T y = mask^2 y  (H2 H2 = I: no transform)"""
    return _Apply.apply(y, mask, SYM_MASK2 | NO_TRANSFORM)


def dagger(y, mask):
    """A^+ y = H2(y (mask > 1e-5 ? 1 / mask : 0))"""
    return _Apply.apply(y, mask, PRE_DAGGER)


def prox_l2(z, y, mask, gamma: float):
    """argmin_x gamma / 2 |A x - y|^2 + 1 / 2 |x - z|^2 = H2((mask y + H2(z) / gamma) / (mask^2 + 1 / gamma))"""
    return _Prox.apply(z, y, mask, 1.0 / float(gamma))
