"""ctypes wrapper of csrc/cdense.hip: ``out[I, R] = in[I, K] op(M)`` in complex64 on the fp32 matrix cores with a pointwise
epilogue, the product behind every operator of RandomPhaseRetrieval (include/deepinv_amd.h, dinv_cdense_apply).  The launch goes
to the current stream of the operands' device.  complex64 only: an input of another dtype raises, it is not cast.

The matrix is used as ``M[r, k]`` and is read where it lies: a row-major matrix, its transposed view and torch's lazily
conjugated views of either (``_A.conj().T``, ``M.mH``) map to the kernel's ``transposed`` and ``conj`` flags, so the device holds
one copy (:func:`deepinv_amd.hip.matrix_operand`, which hip/dense.py uses too).  The call is a ``torch.autograd.Function`` under the autograd rule of
hip/epilogue.py, with ``M.mH`` as the adjoint.  The matrix and the real array of an epilogue are buffers of the operator: no
gradient flows to them."""
from __future__ import annotations

import ctypes

import torch

from . import check, declare_once, lib, matrix_operand, ptr, require_hip, stream_ptr
from . import epilogue as ep
from .epilogue import ABS2, AMPLITUDE, NONE, WEIGHT, operand  # noqa: F401  (the codes are part of this module's interface)


def _declare(l):
    vp, i32, i64, sz, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float
    l.dinv_cdense_workspace_bytes.restype = sz
    l.dinv_cdense_workspace_bytes.argtypes = [i64, i64, i64]
    l.dinv_cdense_apply.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64, i32, i32, i32, f32, vp, sz, vp]


def _l():
    return declare_once(lib(), _declare)


def _matrix(M: torch.Tensor):
    """:func:`deepinv_amd.hip.matrix_operand` of a complex64 matrix"""
    return matrix_operand(M, torch.complex64,
                          "the complex dense kernel is complex64: the matrix has dtype {dtype}; convert it with .to(torch.cfloat)")


def _apply(x, M, epilogue, aux, eps):
    require_hip(x, M, aux)
    x = operand(x, "the input")
    R, K = M.shape
    if x.dim() != 2 or x.shape[1] != K:
        raise ValueError(f"expected an input [rows, {K}], got shape {tuple(x.shape)}")
    I = x.shape[0]
    out = torch.empty((I, R), dtype=torch.float32 if epilogue == ABS2 else torch.complex64, device=x.device)
    aux = ep.aux_operand(epilogue, aux, (I, R))
    store, ldm, transposed, conj = _matrix(M)
    if I == 0:
        return out
    l = _l()
    nbytes = l.dinv_cdense_workspace_bytes(I, K, R)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    check(l.dinv_cdense_apply(ptr(x), ptr(store), ptr(out), ptr(aux), I, K, R, ldm, transposed, conj, epilogue, float(eps), ptr(ws),
                              nbytes, stream_ptr(x.device)))
    return out


class _CDense(torch.autograd.Function):
    @staticmethod
    def forward(x, M, epilogue, aux, eps):
        return _apply(x, M, epilogue, aux, eps)

    @staticmethod
    def setup_context(ctx, inputs, output):
        x, M, epilogue, aux, _ = inputs
        ep.setup_context(ctx, output, x, M, epilogue, aux)

    @staticmethod
    def backward(ctx, g):
        M = ctx.saved_tensors[1]
        gx = ep.backward(ctx, g, run=lambda v, e, a: _CDense.apply(v, M, e, a, 0.0),
                         adjoint=lambda v: _CDense.apply(v, M.mH, NONE, None, 0.0))
        return gx, None, None, None, None


def apply(x: torch.Tensor, M: torch.Tensor, epilogue: int = NONE, aux: torch.Tensor | None = None, eps: float = 1e-12) -> torch.Tensor:
    """``z[i, r] = sum_k x[i, k] M[r, k]`` (einsum "ik, rk -> ir") through the epilogue: ``z``, ``|z|^2`` (real), ``z aux`` or
    ``z (1 - sqrt(aux / (|z|^2 + eps)))``"""
    return _CDense.apply(x, M, int(epilogue), aux, float(eps))
