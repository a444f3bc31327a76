"""Data-fidelity terms (reference deepinv/optim/data_fidelity.py:26-338, 663-795; AmplitudeLoss: 757-773)."""
from __future__ import annotations

import torch

from ..physics.forward import LinearPhysics
from .distance import AmplitudeLossDistance, Distance, L1Distance, L2Distance, LogPoissonLikelihoodDistance, PoissonLikelihoodDistance
from .potential import Potential


class DataFidelity(Potential):
    r""":math:`f(x) = d(A(x), y)` (data_fidelity.py:26-160)."""

    def __init__(self, d=None):
        super().__init__()
        self.d = Distance(d=d)

    def fn(self, x, y, physics, *args, **kwargs):
        return self.d(physics.A(x), y, *args, **kwargs)

    def grad(self, x, y, physics, *args, **kwargs):
        return physics.A_vjp(x, self.d.grad(physics.A(x), y, *args, **kwargs))

    def grad_d(self, u, y, *args, **kwargs):
        return self.d.grad(u, y, *args, **kwargs)

    def prox_d(self, u, y, *args, **kwargs):
        return self.d.prox(u, y, *args, **kwargs)

    def prox_d_conjugate(self, u, y, *args, **kwargs):
        return self.d.prox_conjugate(u, y, *args, **kwargs)


class ZeroFidelity(DataFidelity):
    def fn(self, x, y, physics, *args, **kwargs):
        return torch.zeros(x.shape[0], device=x.device)

    def grad(self, x, y, physics, *args, **kwargs):
        return torch.zeros_like(x)

    def prox(self, x, y, physics, *args, gamma=1.0, **kwargs):
        return x


class L2(DataFidelity):
    r""":math:`\frac{1}{2\sigma^2}\|Ax-y\|^2` (data_fidelity.py:237-338)."""

    def __init__(self, sigma=1.0):
        super().__init__()
        self.d = L2Distance(sigma=sigma)
        self.norm = 1 / (sigma ** 2)

    def prox(self, x, y, physics, *args, gamma=1.0, **kwargs):
        return physics.prox_l2(x, y, self.norm * gamma)

    def grad(self, x, y, physics, *args, **kwargs):
        if isinstance(physics, LinearPhysics):
            return self.norm * (physics.A_adjoint_A(x) - physics.A_adjoint(y))
        return super().grad(x, y, physics, *args, **kwargs)


class PoissonLikelihood(DataFidelity):
    r""":math:`-y^\top\log(z+\beta) + 1^\top z` (data_fidelity.py:663-689); ``denormalize`` defaults to True here, to False in
    the distance, as in the reference."""

    def __init__(self, gain=1.0, bkg=0, denormalize: bool = True):
        super().__init__()
        self.d = PoissonLikelihoodDistance(gain=gain, bkg=bkg, denormalize=denormalize)
        self.bkg = bkg
        self.gain = gain
        self.normalize = denormalize


class L1(DataFidelity):
    r""":math:`\|Ax-y\|_1` (data_fidelity.py:692-754)."""

    def __init__(self):
        super().__init__()
        self.d = L1Distance()

    def prox(self, x, y, physics, *args, gamma=1.0, stepsize=None, crit_conv=1e-5, max_iter=100, **kwargs):
        """dual forward-backward iterations (no closed form for a general operator)"""
        norm_AtA = physics.compute_sqnorm(x)
        stepsize = 1.0 / norm_AtA if stepsize is None else stepsize
        u = x.clone()
        for it in range(max_iter):
            u_prev = u.clone()
            t = x - physics.A_adjoint(u)
            u_ = u + stepsize * physics.A(t)
            u = u_ - stepsize * self.d.prox(u_ / stepsize, y, gamma / stepsize)
            rel_crit = ((u - u_prev).norm()) / (u.norm() + 1e-12)
            if rel_crit < crit_conv and it > 2:
                break
        return t


class AmplitudeLoss(DataFidelity):
    r""":math:`\sum_i (\sqrt{|b_i x|^2} - \sqrt{y_i})^2` for :class:`deepinv_amd.physics.PhaseRetrieval` (data_fidelity.py:757-773).

    With :class:`deepinv_amd.physics.RandomPhaseRetrieval` or :class:`deepinv_amd.physics.StructuredRandomPhaseRetrieval` the
    gradient :math:`2 B^H (Bx \cdot (1 - \sqrt{y / (|Bx|^2 + \epsilon)}))` is two launches: the forward product with the residual
    factor as its epilogue, and the adjoint.  With :class:`deepinv_amd.physics.Ptychography` it is the operator's
    ``normal_epilogue``: forward, residual factor and adjoint per probe position inside one workgroup.  With any other physics
    it is the generic ``A_vjp`` route."""

    def __init__(self):
        super().__init__()
        self.d = AmplitudeLossDistance()

    def grad(self, x, y, physics, *args, epsilon: float = 1e-12, **kwargs):
        from ..hip import epilogue as hep
        from ..physics.phase_retrieval import fused_operator

        B = fused_operator(physics)
        if B is not None and isinstance(y, torch.Tensor) and y.dtype == torch.float32 and tuple(y.shape) == tuple(B.measurement_shape(x)):
            if hasattr(B, "normal_epilogue"):
                return 2 * B.normal_epilogue(x, hep.AMPLITUDE, y, epsilon)
            return 2 * physics.B_adjoint(B.apply_epilogue(x, hep.AMPLITUDE, y, epsilon))
        return super().grad(x, y, physics, *args, epsilon=epsilon, **kwargs)


class LogPoissonLikelihood(DataFidelity):
    r""":math:`N_0(1^\top e^{-\mu z} + \mu\, (e^{-\mu y})^\top z)` (data_fidelity.py:776-795); pairs with ``LogPoissonNoise``."""

    def __init__(self, N0=1024.0, mu=1 / 50.0):
        super().__init__()
        self.d = LogPoissonLikelihoodDistance(N0=N0, mu=mu)
        self.mu = mu
        self.N0 = N0
