"""Spectral initialisation and helpers for phase retrieval (reference deepinv/optim/phase_retrieval.py).  With a phase-retrieval
operator of this package one power iteration is two launches: the forward product with the weights ``T(y)`` as its epilogue, and
the adjoint; with ptychography it is the operator's ``normal_epilogue``, one pass per image."""
from __future__ import annotations

from typing import Callable

import torch


def default_preprocessing(y: torch.Tensor, physics=None) -> torch.Tensor:
    r""":math:`\max(1 - 1/y, -5)` (phase_retrieval.py:9-23)"""
    return torch.max(1 - 1 / y, torch.tensor(-5.0, device=y.device))


def correct_global_phase(x_est: torch.Tensor, x_ref: torch.Tensor, correct_magnitude: bool = False, dim=(-2, -1),
                         verbose: bool = False) -> torch.Tensor:
    r"""
    Multiplies ``x_est`` by the complex scalar :math:`c` (per batch entry and channel) that minimises
    :math:`\|c \hat{x} - x\|^2`, of unit modulus unless ``correct_magnitude`` (phase_retrieval.py:26-79).
    """
    if x_est.shape != x_ref.shape:
        raise ValueError(f"The shapes of the signals should be the same, got {tuple(x_est.shape)} and {tuple(x_ref.shape)}.")
    inner = (x_est.conj() * x_ref).sum(dim=dim, keepdim=True)
    if correct_magnitude:
        energy = (x_est.abs() ** 2).sum(dim=dim, keepdim=True)
        c = inner / (energy + 1e-12)
    else:
        c = inner / (inner.abs() + 1e-12)
    if verbose:
        print(f"Applying global phase shift (radians):\n{c.angle().squeeze(dim)}")
        print(f"Scaling factor:\n{c.abs().squeeze(dim)}")
    return c * x_est


def cosine_similarity(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    r""":math:`|\langle a, b \rangle| / (\|a\| \|b\|)` (phase_retrieval.py:82-103)"""
    if a.shape != b.shape:
        raise ValueError("Shape of Tensors are not equal.")
    a = a.flatten()
    b = b.flatten()
    norm_a = torch.sqrt(torch.dot(a.conj(), a).real)
    norm_b = torch.sqrt(torch.dot(b.conj(), b).real)
    return torch.abs(torch.dot(a.conj(), b)) / (norm_a * norm_b)


def spectral_methods(y: torch.Tensor, physics, x: torch.Tensor = None, n_iter: int = 50,
                     preprocessing: Callable = default_preprocessing, lamb: float = 10.0, x_true: torch.Tensor = None,
                     log: bool = False, log_metric: Callable = cosine_similarity, early_stop: bool = True, rtol: float = 1e-5,
                     verbose: bool = False):
    r"""
    Power iteration on :math:`M = \overline{B}^\top \text{diag}(T(y)) B + \lambda I` (phase_retrieval.py:106-193), with the
    reference's semantics: the norm of an iterate is taken over the whole batch, the result is scaled to ``sqrt(y.sum())``,
    ``early_stop`` compares successive iterates with ``rtol``, and the initial guess is ``randn_like(A_adjoint(y))`` when ``x``
    is ``None``.

    :return: the estimate, or ``(estimate, metrics)`` when ``log``.
    """
    from ..hip import epilogue as hep
    from ..physics.phase_retrieval import fused_operator

    if x is None:
        # always randn, never rand
        x = physics.A_adjoint(y)
        x = torch.randn_like(x)
    if log is True:
        metrics = []
    norm_x = torch.sqrt(y.sum())
    # y should have mean 1
    y = y / torch.mean(y)
    diag_T = preprocessing(y, physics)
    B = fused_operator(physics)
    fused = B is not None and diag_T.dtype == torch.float32 and tuple(diag_T.shape) == tuple(B.measurement_shape(x))
    if not fused:
        diag_T = diag_T.to(x)
    for i in range(n_iter):
        if fused and hasattr(B, "normal_epilogue"):
            x_new = B.normal_epilogue(x, hep.WEIGHT, diag_T)
        else:
            if fused:
                x_new = B.apply_epilogue(x, hep.WEIGHT, diag_T)
            else:
                x_new = physics.B(x)
                x_new = diag_T * x_new
            x_new = physics.B_adjoint(x_new)
        x_new = x_new + lamb * x
        x_new = x_new / torch.linalg.norm(x_new)
        if log:
            metrics.append(log_metric(x_new, x_true))
        if early_stop:
            if torch.linalg.norm(x_new - x) / torch.linalg.norm(x) < rtol:
                if verbose:
                    print(f"Power iteration early stopped at iteration {i}.")
                break
        x = x_new
    x = x * norm_x
    if log:
        return x, metrics
    return x


def spectral_methods_wrapper(y: torch.Tensor, physics, n_iter: int = 5000, **kwargs) -> dict:
    """:func:`spectral_methods` as the ``custom_init`` of an optimizer: ``{"est": (x, z)}`` (phase_retrieval.py:196-212)"""
    x = spectral_methods(y, physics, n_iter=n_iter, **kwargs)
    z = x.detach().clone()
    return {"est": (x, z)}
