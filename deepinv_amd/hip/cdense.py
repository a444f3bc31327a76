"""ctypes wrapper of csrc/cdense.hip: ``out[I, R] = in[I, K] op(M)`` in complex64 on the fp32 matrix cores with a pointwise
epilogue, the product behind every operator of RandomPhaseRetrieval (include/deepinv_amd.h, dinv_cdense_apply).  The launch goes
to the current stream of the operands' device.  complex64 only: an input of another dtype raises, it is not cast.

The matrix is used as ``M[r, k]`` and is read where it lies: a row-major matrix, its transposed view and torch's lazily
conjugated views of either (``_A.conj().T``, ``M.mH``) map to the kernel's ``transposed`` and ``conj`` flags, so the device holds
one copy.  The call is a ``torch.autograd.Function``: the backward of ``NONE`` is the adjoint form of the same kernel, the
backward of ``ABS2`` is ``2 B^H (z g)`` - the ``WEIGHT`` forward followed by the adjoint.  The matrix and the real array of an
epilogue are buffers of the operator: no gradient flows to them."""
from __future__ import annotations

import ctypes

import torch

from . import check, declare_once, lib, ptr, require_hip, stream_ptr

NONE, ABS2, WEIGHT, AMPLITUDE = 0, 1, 2, 3      # DINV_CDENSE_*


def _declare(l):
    vp, i32, i64, sz, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float
    l.dinv_cdense_workspace_bytes.restype = sz
    l.dinv_cdense_workspace_bytes.argtypes = [i64, i64, i64]
    l.dinv_cdense_apply.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64, i32, i32, i32, f32, vp, sz, vp]


def _l():
    return declare_once(lib(), _declare)


def _matrix(M: torch.Tensor):
    """(storage tensor, row stride, transposed, conj) of a 2-D complex64 matrix used as ``M[r, k]``: a row-major matrix as it
    is, the transposed view of one through the kernel's transposed form, a lazily conjugated view (``is_conj()``) of either
    through the conj flag, anything else through one contiguous copy"""
    if M.dim() != 2:
        raise ValueError(f"expected a matrix, got shape {tuple(M.shape)}")
    if M.dtype != torch.complex64:
        raise TypeError(f"the complex dense kernel is complex64: the matrix has dtype {M.dtype}; convert it with .to(torch.cfloat)")
    conj = int(M.is_conj())
    phys = M.conj() if conj else M          # the same storage with the conjugate bit cleared: no copy
    R, K = phys.shape
    if phys.stride(1) == 1 and phys.stride(0) >= K:
        return phys, phys.stride(0), 0, conj
    if phys.stride(0) == 1 and phys.stride(1) >= R:
        return phys, phys.stride(1), 1, conj
    return M.resolve_conj().contiguous(), K, 0, 0


def operand(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.complex64:
        raise TypeError(f"the phase-retrieval kernels are complex64: {what} has dtype {t.dtype}; convert it with .to(torch.cfloat)")
    return t.resolve_conj().contiguous()


def real_operand(t, shape, what: str) -> torch.Tensor:
    if t is None:
        raise ValueError(f"this epilogue needs {what}")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be real fp32 of the output's shape, got dtype {t.dtype}; convert it with .float()")
    if t.numel() != int(torch.Size(shape).numel()):
        raise ValueError(f"{what} must have the output's shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def _apply(x, M, epilogue, aux, eps):
    require_hip(x, M, aux)
    x = operand(x, "the input")
    R, K = M.shape
    if x.dim() != 2 or x.shape[1] != K:
        raise ValueError(f"expected an input [rows, {K}], got shape {tuple(x.shape)}")
    I = x.shape[0]
    out = torch.empty((I, R), dtype=torch.float32 if epilogue == ABS2 else torch.complex64, device=x.device)
    if epilogue in (WEIGHT, AMPLITUDE):
        aux = real_operand(aux, (I, R), "the weights" if epilogue == WEIGHT else "the measurements")
    else:
        aux = None
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
        x, M, ctx.epilogue, aux, _ = inputs
        if ctx.epilogue == AMPLITUDE:
            # the gradient of AmplitudeLoss itself: a value, not a node of the graph
            ctx.mark_non_differentiable(output)
            return
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x if ctx.epilogue == ABS2 else None, M, aux if ctx.epilogue == WEIGHT else None)

    @staticmethod
    def backward(ctx, g):
        x, M, aux = ctx.saved_tensors
        if ctx.epilogue == NONE:
            gx = _CDense.apply(g, M.mH, NONE, None, 0.0)
        elif ctx.epilogue == ABS2:
            gx = 2 * _CDense.apply(_CDense.apply(x, M, WEIGHT, g.float(), 0.0), M.mH, NONE, None, 0.0)
        else:
            gx = _CDense.apply(g * aux, M.mH, NONE, None, 0.0)
        return gx, None, None, None, None


def apply(x: torch.Tensor, M: torch.Tensor, epilogue: int = NONE, aux: torch.Tensor | None = None, eps: float = 1e-12) -> torch.Tensor:
    """``z[i, r] = sum_k x[i, k] M[r, k]`` (einsum "ik, rk -> ir") through the epilogue: ``z``, ``|z|^2`` (real), ``z aux`` or
    ``z (1 - sqrt(aux / (|z|^2 + eps)))``"""
    return _CDense.apply(x, M, int(epilogue), aux, float(eps))
