"""``TGVDenoiser`` (reference deepinv/models/tgv.py:7-310) on the kernels of csrc/tgv.hip.

Semantics kept from the reference:

* ``forward(y, ths)`` solves argmin_{x,r} 1/2 |x - y|^2 + lam1 |r|_{1,2} + lam2 |J(Dx - r)|_{1,F} (second-order total
  generalized variation) with the over-relaxed Chambolle-Pock iteration of tgv.py:148-171, for ``[B,C,H,W]`` images and
  ``[B,C,D,H,W]`` volumes, with ``lam1 = 0.1 ths``, ``lam2 = 0.15 ths`` per sample, ``tau = 0.01``, ``rho = 1.99`` and
  ``sigma = 1 / tau / (72 f)`` (``f = 3`` in 3-D, 1 in 2-D):
  ``t = tau eps^T(u2)``, ``x = (x2 - D^T t + tau y) / (1 + tau)``, ``r = s - s / max(|s| / (tau lam1), 1)`` with
  ``s = r2 + t``, ``u = P(u2 + sigma eps(D(2x - x2) - (2r - r2)))`` with ``P(v) = v / max(|v| / lam2, 1)``, then
  ``x2 += rho (x - x2)``, ``r2 += rho (r - r2)``, ``u2 += rho (u - u2)``.
* ``ths`` is a float, a per-sample tensor or a list (Denoiser._handle_sigma, deepinv/models/base.py:48-100).  ``ths > 0``
  is the contract: at ``ths = 0`` the reference divides 0 by 0 and returns NaN; this class does not check for it.
* Stopping rule (tgv.py:162-171): ``rel_err = |x2_prev - x2| / (|x2| + 1e-12)`` over the WHOLE batch; the loop stops after
  the iteration of index ``> 1`` whose ``rel_err < crit`` and returns that iterate.  The test runs on the device; the host
  looks at the flag every ``poll_every`` iterations through a pinned copy and an event query, never with a blocking sync
  per iteration.
* Warm restart (tgv.py:107-119): the first call on an instance starts from ``x2 = y``, ``r2 = 0``, ``u2 = 0``; later calls
  with the same shape start from the stored ``x2`` / ``r2`` / ``u2``, which are stored detached after every call.  ``r2`` is
  ``[*y.shape, nd]`` and ``u2`` ``[*y.shape, nd^2]`` with the component last, as in the reference.
* ``has_converged`` becomes True at the first call that meets the stopping rule and stays True, as in the reference.
* With ``verbose`` the reference's convergence and non-convergence messages are printed.  Its primal-cost print every 100
  iterations is not: it needs the cost on the host, which would bring back the per-iteration sync this class removes.

``n_iter`` is the number of iterations the last call ran (the reference's loop index at ``break``, plus one).
There is no CPU path and no autograd through the prox: a CPU tensor raises ``RuntimeError``, a non-fp32 or complex
tensor ``TypeError``, an input that records gradients ``NotImplementedError``; a call during stream capture raises.
"""
from __future__ import annotations

import torch

from ..hip import tgv as K
from .base import Denoiser
from .tv import TVDenoiser, check_tv_input, handle_ths


class TGVDenoiser(Denoiser):
    r"""Proximal operator of second-order total generalized variation (reference deepinv/models/tgv.py:7-310), by
    over-relaxed Chambolle-Pock with warm restart.  See the module docstring for the exact rules; one iteration is three
    launches with no host sync (csrc/tgv.hip)."""

    poll_every = 8

    def __init__(self, verbose: bool = False, n_it_max: int = 1000, crit: float = 1e-5, x2: torch.Tensor = None,
                 u2: torch.Tensor = None, r2: torch.Tensor = None, ths: float | torch.Tensor = None):
        super().__init__()
        self.verbose = verbose
        self.n_it_max = n_it_max
        self.crit = crit
        self.restart = True
        self.ths = ths
        self.tau = 0.01
        self.rho = 1.99
        self.x2 = x2
        self.r2 = r2
        self.u2 = u2
        self.has_converged = False
        self.n_iter = 0

    def forward(self, y: torch.Tensor, ths: float | torch.Tensor = None, **kwargs) -> torch.Tensor:
        """tgv.py:93-214"""
        if ths is None and self.ths is None:
            raise RuntimeError("Regularization parameter (ths) was not passed at init nor at forward. Please provide ths to one "
                               "of these methods.")
        elif ths is None:
            ths = self.ths
        name = type(self).__name__
        if isinstance(y, torch.Tensor) and y.dim() not in (4, 5):
            raise ValueError(f"{name} takes [B,C,H,W] or [B,C,D,H,W] tensors, got shape {tuple(y.shape)}")
        y = check_tv_input(y, name)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{name} polls its device stopping flag from the host and cannot be captured into a graph")
        nd = y.dim() - 2
        restart = (self.restart or self.x2 is None or self.r2 is None or self.u2 is None or self.x2.shape != y.shape)
        if restart:
            x2 = y.clone()
            r2 = torch.zeros((*y.shape, nd), device=y.device, dtype=y.dtype)
            u2 = torch.zeros((*y.shape, nd * nd), device=y.device, dtype=y.dtype)
            self.restart = False
        else:
            x2, r2, u2 = (check_tv_input(t, name).clone() for t in (self.x2, self.r2, self.u2))
        f = 3 if nd == 3 else 1
        sigma = 1 / self.tau / (72 * f)                 # tgv.py:121-122
        lam = handle_ths(ths, y.shape[0], y.device)
        st = K.CPState(y, x2, r2, u2, lam * 0.1, lam * 0.15, self.tau, sigma, self.rho, self.crit)
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
        x2, r2, u2, self.n_iter, done = st.result()
        if done:
            self.has_converged = True
            if self.verbose:
                print("TGV prox reached convergence")
        elif self.verbose and self.n_iter == self.n_it_max and self.n_it_max > 0:
            print("The algorithm did not converge, stopped after " + str(self.n_iter) + " iterations.")
        self.x2 = x2.detach()
        self.r2 = r2.detach()
        self.u2 = u2.detach()
        return x2

    @staticmethod
    def nabla(x: torch.Tensor) -> torch.Tensor:
        """TV's forward differences (tgv.py:215-220)"""
        return TVDenoiser.nabla(x)

    @staticmethod
    def nabla_adjoint(x: torch.Tensor) -> torch.Tensor:
        """TV's adjoint differences (tgv.py:222-227)"""
        return TVDenoiser.nabla_adjoint(x)

    @staticmethod
    def epsilon(I: torch.Tensor) -> torch.Tensor:
        """backward differences of each component of a vector field, [*I.shape[:-1], nd^2], component i * nd + j along
        axis j, zero on the first face (tgv.py:229-271)"""
        if I.ndim not in [5, 6]:
            raise ValueError(f"Input tensor must be 5D or 6D, got {I.ndim}D")
        return K.epsilon(check_tv_input(I, "epsilon"))

    @staticmethod
    def epsilon_adjoint(G: torch.Tensor) -> torch.Tensor:
        """the exact adjoint of ``epsilon`` (tgv.py:272-310)"""
        if G.ndim not in [5, 6]:
            raise ValueError(f"Input tensor must be 5D or 6D, got {G.ndim}D")
        return K.epsilon_adjoint(check_tv_input(G, "epsilon_adjoint"))
