"""The pointwise epilogues ``DINV_CDENSE_*`` of the complex operators (hip/cdense.py, hip/cstructured.py, hip/ptycho.py) on the
Python side: their codes, the checks of their operands and their one autograd rule.

With ``z`` the value of the linear operator ``B``: ``NONE`` is ``z``, ``ABS2`` is ``|z|^2`` (real), ``WEIGHT`` is ``z aux`` and
``AMPLITUDE`` is ``z (1 - sqrt(aux / (|z|^2 + eps)))`` with ``aux`` real, of the output's shape."""
from __future__ import annotations

import torch

NONE, ABS2, WEIGHT, AMPLITUDE = 0, 1, 2, 3      # DINV_CDENSE_*


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


def aux_operand(epilogue: int, aux, shape):
    """the real array of ``WEIGHT`` / ``AMPLITUDE``, checked; None for the epilogues that read none"""
    if epilogue in (WEIGHT, AMPLITUDE):
        return real_operand(aux, shape, "the weights" if epilogue == WEIGHT else "the measurements")
    return None


def setup_context(ctx, output, x, operator, epilogue: int, aux):
    """what the backward of an epilogue needs: the input for ``ABS2``, the operator's own tensor (matrix, diagonals, probe), the
    real array for ``WEIGHT``; always in the order ``x, operator, aux`` of ``ctx.saved_tensors``"""
    ctx.epilogue = epilogue
    if epilogue == AMPLITUDE:
        # the gradient of AmplitudeLoss itself: a value, not a node of the graph
        ctx.mark_non_differentiable(output)
        return
    if ctx.needs_input_grad[0]:
        ctx.save_for_backward(x if epilogue == ABS2 else None, operator, aux if epilogue == WEIGHT else None)


def backward(ctx, g, run, adjoint, normal=None):
    """the gradient with respect to the input of ``run(x, epilogue, aux)``: ``adjoint(g)`` for ``NONE``,
    ``2 B^H (z g) = 2 adjoint(run(x, WEIGHT, g))`` for ``ABS2`` and ``adjoint(g aux)`` for ``WEIGHT``.  ``normal(x, w)`` is an
    operator's own fused ``adjoint(run(x, WEIGHT, w))``, where it has one."""
    x, _, aux = ctx.saved_tensors
    if ctx.epilogue == NONE:
        return adjoint(g)
    if ctx.epilogue == ABS2:
        return 2 * (normal(x, g.float()) if normal else adjoint(run(x, WEIGHT, g.float())))
    return adjoint(g * aux)
