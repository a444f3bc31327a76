"""``TVDenoiser`` / ``TVL1Denoiser`` (reference deepinv/models/tv.py:5-240) on the fused kernels of csrc/tv.hip.

Semantics kept from the reference:

* ``forward(y, ths)`` solves argmin_x 1/2 |x - y|^2 + ths |Dx|_{1,2} (anisotropic |Dx|_1 for ``TVL1Denoiser``) with the
  over-relaxed Chambolle-Pock iteration of tv.py:131-139, for ``[B,C,H,W]`` images and ``[B,C,D,H,W]`` volumes:
  ``x = (x2 - tau D^T u2 + tau y) / (1 + tau)``, ``u = P(u2 + sigma D(2x - x2))``, ``x2 += rho (x - x2)``,
  ``u2 += rho (u - u2)`` with ``sigma = 1 / tau / 2**(y.ndim - 1)`` (12.5 in 2-D, 6.25 in 3-D at tau = 0.01) and
  ``P(u) = u / max(|u|_2 / ths, 1)`` over the component axis (``TVL1Denoiser``: ``clamp(u, -ths, ths)``, tv.py:239-240).
* ``ths`` is a float, a per-sample tensor or a list, broadcast over ``[B,1,...]`` (Denoiser._handle_sigma,
  deepinv/models/base.py:48-100).
* Stopping rule (tv.py:141-148): ``rel_err = |x2_prev - x2| / |x2 + 1e-12|`` over the WHOLE batch; the loop stops after
  the iteration of index ``> 1`` whose ``rel_err < crit`` and returns that iterate (one sample can keep the others
  iterating).  The test runs on the device; the host looks at the flag every ``poll_every`` iterations through a pinned
  copy and an event query (as FixedPoint._run_device_stop), never with a blocking sync per iteration.
* Warm restart (tv.py:104-117, 150-151): the first call on an instance starts from ``x2 = y``, ``u2 = 0``; later calls
  with the same shape start from the stored ``x2`` / ``u2``; both are stored detached after every call.  ``u2`` has shape
  ``[*y.shape, nd]`` with the gradient component last, as in the reference.

``n_iter`` is the number of iterations the last call ran (the reference's loop index at ``break``, plus one).
There is no CPU path and no autograd through the prox: a CPU tensor raises ``RuntimeError``, a non-fp32 or complex
tensor ``TypeError``, an input that records gradients ``NotImplementedError``; a call during stream capture raises.
"""
from __future__ import annotations

import numpy as np
import torch

from ..hip import tv as K
from .base import Denoiser


def check_tv_input(x: torch.Tensor, what: str = "TV") -> torch.Tensor:
    """the package's TV operators take real fp32 HIP tensors outside autograd recording (returns x contiguous)"""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: only real float32 tensors are supported, got {x.dtype}")
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError(f"{what}: autograd through the TV kernels is not implemented (call it under torch.no_grad())")
    if not x.is_cuda:
        raise RuntimeError(f"{what}: deepinv_amd runs only on a HIP device (got a tensor on '{x.device}'); there is no CPU path")
    return x.contiguous()


def handle_ths(ths, batch_size: int, device) -> torch.Tensor:
    """per-sample thresholds [B] as fp32 on `device` (the cases of Denoiser._handle_sigma, base.py:48-100)"""
    if isinstance(ths, (float, int)):
        return torch.full((batch_size,), float(ths), dtype=torch.float32, device=device)
    if isinstance(ths, np.ndarray):
        ths = torch.from_numpy(ths)
    elif isinstance(ths, list):
        ths = torch.tensor(ths, dtype=torch.float32)
    elif not isinstance(ths, torch.Tensor):
        raise TypeError(f"Sigma must be a float, int, or torch.Tensor. Got {type(ths)}.")
    ths = ths.detach().squeeze().to(dtype=torch.float32, device=device)
    if ths.ndim == 0 or (ths.ndim == 1 and ths.size(0) == 1):
        return ths.reshape(1).expand(batch_size).contiguous()
    if ths.ndim == 1 and ths.size(0) == batch_size:
        return ths.contiguous()
    if ths.ndim == 1:
        raise ValueError(f"Sigma tensor size {ths.size(0)} does not match batch size {batch_size}.")
    raise ValueError(f"Sigma tensor has {ths.ndim} dimensions, expected 0 or 1.")


class TVDenoiser(Denoiser):
    r"""Proximal operator of the isotropic total variation (reference deepinv/models/tv.py:5-218): the unique solution of
    :math:`\arg\min_x \frac{1}{2}\|x-y\|_2^2 + \gamma \|Dx\|_{1,2}` by over-relaxed Chambolle-Pock with warm restart.
    See the module docstring for the exact rules; the iteration is one fused kernel pair per step (csrc/tv.hip)."""

    aniso = False
    poll_every = 8

    def __init__(self, verbose: bool = False, tau: float = 0.01, rho: float = 1.99, n_it_max: int = 1000, crit: float = 1e-5,
                 x2: torch.Tensor = None, u2: torch.Tensor = None, ths: float | torch.Tensor = None):
        super().__init__()
        self.verbose = verbose
        self.n_it_max = n_it_max
        self.crit = crit
        self.restart = True
        self.ths = ths
        self.tau = tau
        self.rho = rho
        self.x2 = x2
        self.u2 = u2
        self.has_converged = False
        self.n_iter = 0

    def forward(self, y: torch.Tensor, ths: float | torch.Tensor = None, **kwargs) -> torch.Tensor:
        """tv.py:86-152"""
        if ths is None and self.ths is None:
            raise RuntimeError("Regularization parameter (ths) was not passed at init nor at forward. Please provide ths to one "
                               "of these methods.")
        elif ths is None:
            ths = self.ths
        y = check_tv_input(y, type(self).__name__)
        if y.dim() not in (4, 5):
            raise ValueError(f"{type(self).__name__} takes [B,C,H,W] or [B,C,D,H,W] tensors, got shape {tuple(y.shape)}")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__} polls its device stopping flag from the host and cannot be captured "
                               "into a graph")
        nd = y.dim() - 2
        restart = self.restart or self.x2 is None or self.u2 is None or self.x2.shape != y.shape
        if restart:
            x2 = y.clone()
            u2 = torch.zeros((*y.shape, nd), device=y.device, dtype=y.dtype)
            self.restart = False
        else:
            x2 = check_tv_input(self.x2, type(self).__name__).clone()
            u2 = check_tv_input(self.u2, type(self).__name__).clone()
        sigma = 1 / self.tau / 2 ** (y.ndim - 1)          # tv.py:119-121
        lam = handle_ths(ths, y.shape[0], y.device)
        st = K.CPState(y, x2, u2, lam, self.aniso, self.tau, sigma, self.rho, self.crit)
        polls = []
        for it in range(self.n_it_max):
            st.step()
            if it % self.poll_every == self.poll_every - 1:
                host = torch.empty((), dtype=torch.int32, pin_memory=True)
                host.copy_(st.state[0], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                polls.append((ev, host))
            if polls and polls[0][0].query():
                if int(polls.pop(0)[1]):
                    break
        x2, u2, self.n_iter, self.has_converged = st.result()
        if self.verbose and self.has_converged:
            print("TV prox reached convergence")
        self.x2 = x2.detach()
        self.u2 = u2.detach()
        return x2

    @staticmethod
    def nabla(x: torch.Tensor) -> torch.Tensor:
        """forward differences [*x.shape, nd], zero on the last row / column / slice (tv.py:154-184)"""
        if x.ndim not in [4, 5]:
            raise ValueError(f"Input tensor must be 4D or 5D, got {x.ndim}D")
        return K.nabla(check_tv_input(x, "nabla"))

    @staticmethod
    def nabla_adjoint(x: torch.Tensor) -> torch.Tensor:
        """the exact adjoint of ``nabla`` (tv.py:186-218)"""
        if x.ndim not in [5, 6]:
            raise ValueError(f"Input tensor must be 5D or 6D, got {x.ndim}D")
        return K.nabla_adjoint(check_tv_input(x, "nabla_adjoint"))


class TVL1Denoiser(TVDenoiser):
    """Proximal operator of the anisotropic TV |Dx|_1 (reference tv.py:221-240): the dual projection is
    ``clamp(u, -ths, ths)`` per component instead of the isotropic norm ball."""

    aniso = True
