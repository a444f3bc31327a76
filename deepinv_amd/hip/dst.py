"""ctypes wrappers of csrc/dst.hip: the orthonormal DST-I of the last axis and the fused operators of StructuredRandom
(include/deepinv_amd.h, "DST-I, StructuredRandom and CompressedSensing").  Every launch goes to the current stream of the
operands' device.  fp32 only: an input of another dtype raises, it is not cast.  Each call is a ``torch.autograd.Function`` whose
backward is the adjoint kernel (``dst1`` is symmetric; ``structured_apply`` flips the adjoint flag).  The diagonals are buffers
of the operator: no gradient flows to them."""
from __future__ import annotations

import ctypes

import torch

from . import FftPlan, check, declare_once, fft_plan, lib, ptr, require_hip, stream_ptr

MAX_N = 2924        # DINV_DST_MAX_N: the largest row whose odd extension, tables and two line buffers fit the 160 KB of LDS


def _declare(l):
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    plan = ctypes.POINTER(FftPlan)
    l.dinv_dst_workspace_bytes.restype = sz
    l.dinv_dst_workspace_bytes.argtypes = [i64, i32]
    l.dinv_dst1.argtypes = [vp, vp, i64, i32, plan, vp, vp]
    l.dinv_structured_apply.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, i64, i32, i32, i32, plan, vp, vp]


def _l():
    return declare_once(lib(), _declare)


def _operand(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"the DST kernels are fp32: {what} has dtype {t.dtype}; convert it with .float()")
    return t.contiguous()


def check_length(n: int):
    if n > MAX_N:
        raise NotImplementedError(f"the DST-I kernel holds a row in LDS and takes rows of at most {MAX_N} elements, got {n}")
    if n < 1:
        raise ValueError("the transformed axis is empty")


def _dst1(x):
    require_hip(x)
    if x.dim() < 1:
        raise ValueError("dst1 needs a tensor with at least one dimension")
    n = int(x.shape[-1])
    check_length(n)
    x = _operand(x, "the input")
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    plan, table = fft_plan(2 * (n + 1), x.device)
    check(_l().dinv_dst1(ptr(x), ptr(out), x.numel() // n, n, ctypes.byref(plan), ptr(table), stream_ptr(x.device)))
    return out


class _Dst1(torch.autograd.Function):
    @staticmethod
    def forward(x):
        return _dst1(x)

    @staticmethod
    def setup_context(ctx, inputs, output):
        pass

    @staticmethod
    def backward(ctx, g):
        return _Dst1.apply(g)


def dst1(x: torch.Tensor) -> torch.Tensor:
    """the reference's DST-I of the last axis: ``-sqrt(2 / (n + 1)) sum_j x_j sin(pi (j + 1)(k + 1) / (n + 1))``"""
    return _Dst1.apply(x)


def _structured(x, diag, geom, layers, half, adjoint):
    """x is [planes, H_in, W_in]; geom = (in_hw, out_hw, work_hw, top, left, diag_rows): the side x has, the side the result
    has, the working side (the larger of the two), the offsets of the smaller side in it and the rows of one diagonal"""
    require_hip(x, diag if layers else None)
    (h_in, w_in), (h_out, w_out), (h_work, w_work), top, left, diag_rows = geom
    if x.dim() != 3 or tuple(x.shape[1:]) != (h_in, w_in):
        raise ValueError(f"expected an input [planes, {h_in}, {w_in}], got shape {tuple(x.shape)}")
    check_length(w_work)
    x = _operand(x, "the input")
    planes = int(x.shape[0])
    out = torch.empty((planes, h_out, w_out), dtype=x.dtype, device=x.device)
    if planes == 0:
        return out
    if layers:
        diag = _operand(diag, "the diagonals")
        if diag.numel() != layers * diag_rows * w_work:
            raise ValueError(f"the diagonals hold {diag.numel()} values, expected {layers} x {diag_rows} x {w_work}")
    plan, table = fft_plan(2 * (w_work + 1), x.device)
    check(_l().dinv_structured_apply(ptr(x), ptr(out), ptr(diag) if layers else None, planes, h_in, w_in, h_out, w_out, h_work,
                                     w_work, top, left, diag_rows, layers, half, int(adjoint), ctypes.byref(plan), ptr(table),
                                     stream_ptr(x.device)))
    return out


class _Structured(torch.autograd.Function):
    """A (adjoint = False) or A_adjoint of StructuredRandom as one launch; backward is the other one"""

    @staticmethod
    def forward(x, diag, geom, layers, half, adjoint):
        return _structured(x, diag, geom, layers, half, adjoint)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _, diag, ctx.geom, ctx.layers, ctx.half, ctx.adjoint = inputs
        ctx.save_for_backward(diag)

    @staticmethod
    def backward(ctx, g):
        (diag,) = ctx.saved_tensors
        i, o, w, top, left, rows = ctx.geom
        return _Structured.apply(g, diag, (o, i, w, top, left, rows), ctx.layers, ctx.half, not ctx.adjoint), None, None, None, None, None


def structured_apply(x, diag, geom, layers: int, half: bool, adjoint: bool):
    return _Structured.apply(x, diag, geom, int(layers), int(bool(half)), bool(adjoint))
