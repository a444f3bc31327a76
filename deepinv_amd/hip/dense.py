"""ctypes wrapper of csrc/dense.hip: ``out[I, R] = in[I, K] M^T`` in fp32 on the matrix cores, the product behind every operator
of CompressedSensing (include/deepinv_amd.h, dinv_dense_apply).  The launch goes to the current stream of the operands' device.
fp32 only.  The call is a ``torch.autograd.Function`` whose backward is the same kernel with ``transposed`` flipped, so the
device holds one copy of the matrix.  The matrix is a buffer of the operator: no gradient flows to it."""
from __future__ import annotations

import ctypes

import torch

from . import check, declare_once, lib, matrix_operand, ptr, require_hip, stream_ptr


def _declare(l):
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    l.dinv_dense_workspace_bytes.restype = sz
    l.dinv_dense_workspace_bytes.argtypes = [i64, i64, i64]
    l.dinv_dense_apply.argtypes = [vp, vp, vp, i64, i64, i64, i64, i32, vp, sz, vp]


def _l():
    return declare_once(lib(), _declare)


def _apply(x, M):
    require_hip(x, M)
    if x.dtype != torch.float32:
        raise TypeError(f"the dense kernel is fp32: the input has dtype {x.dtype}; convert it with .float()")
    R, K = M.shape
    if x.dim() != 2 or x.shape[1] != K:
        raise ValueError(f"expected an input [rows, {K}], got shape {tuple(x.shape)}")
    x = x.contiguous()
    I = x.shape[0]
    out = torch.empty((I, R), dtype=x.dtype, device=x.device)
    if I == 0:
        return out
    # a real matrix has no conjugate
    store, ldm, transposed, _ = matrix_operand(M, torch.float32, "the dense kernel is fp32: the matrix has dtype {dtype}")
    l = _l()
    nbytes = l.dinv_dense_workspace_bytes(I, K, R)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    check(l.dinv_dense_apply(ptr(x), ptr(store), ptr(out), I, K, R, ldm, transposed, ptr(ws), nbytes, stream_ptr(x.device)))
    return out


class _Dense(torch.autograd.Function):
    @staticmethod
    def forward(x, M):
        return _apply(x, M)

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.save_for_backward(inputs[1])

    @staticmethod
    def backward(ctx, g):
        (M,) = ctx.saved_tensors
        return _Dense.apply(g, M.t()), None


def apply(x: torch.Tensor, M: torch.Tensor) -> torch.Tensor:
    """``out[i, r] = sum_k x[i, k] M[r, k]`` (einsum "ik, rk -> ir")"""
    return _Dense.apply(x, M)
