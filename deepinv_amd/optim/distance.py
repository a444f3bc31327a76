"""Distances (reference deepinv/optim/distance.py:13-115, 196-395).

``grad`` / ``prox`` of the Poisson, L1 and log-Poisson distances are one launch of dinv_fidelity_pointwise (csrc/elementwise.hip) for
fp32 tensors on a HIP device; when an input records a gradient, or ``gamma`` is a Tensor, they are the reference's torch expressions, so
that autograd follows.  ``fn`` is the reference's expression on every device."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ..hip import elementwise as ew
from .potential import Potential


class Distance(Potential):
    def __init__(self, d=None):
        super().__init__(fn=d)

    def fn(self, x, y, *args, **kwargs):
        return self._fn(x, y, *args, **kwargs)

    def forward(self, x, y, *args, **kwargs):
        return self.fn(x, y, *args, **kwargs)


class L2Distance(Distance):
    r""":math:`\frac{1}{2\sigma^2}\|x-y\|^2` (distance.py:47-115)."""

    def __init__(self, sigma=1.0):
        super().__init__()
        self.norm = 1 / (sigma ** 2)

    def fn(self, x, y, *args, **kwargs):
        z = x - y
        return 0.5 * torch.linalg.vector_norm(z, ord=2, dim=tuple(range(1, z.dim()))) ** 2 * self.norm

    def grad(self, x, y, *args, **kwargs):
        return (x - y) * self.norm

    def prox(self, x, y, *args, gamma=1.0, **kwargs):
        return (x + self.norm * gamma * y) / (1 + gamma * self.norm)


class PoissonLikelihoodDistance(Distance):
    r""":math:`\sum_i y_i\log(y_i/x_i) + x_i - y_i` with gain and background (distance.py:196-263)."""

    def __init__(self, gain=1.0, bkg=0, denormalize: bool = False):
        super().__init__()
        self.bkg = bkg
        self.gain = gain
        self.denormalize = denormalize

    def fn(self, x, y, *args, **kwargs):
        if self.denormalize:
            y = y / self.gain
        # the first term is summed over the whole batch, as in the reference (distance.py:231-233)
        return (-y * torch.log(x / self.gain + self.bkg)).flatten().sum() + ((x / self.gain) + self.bkg - y).reshape(
            x.shape[0], -1).sum(dim=1)

    def grad(self, x, y, *args, **kwargs):
        if ew.fidelity_eligible(x, y, self.gain, self.bkg):
            return ew.fidelity_pointwise(ew.FID_POISSON_GRAD, x, y, self.gain, self.bkg, denormalize=self.denormalize)
        if self.denormalize:
            y = y / self.gain
        return self.gain * (1 - y / (x / self.gain + self.bkg))

    def prox(self, x, y, *args, gamma=1.0, **kwargs):
        if ew.fidelity_eligible(x, y, self.gain, gamma):
            return ew.fidelity_pointwise(ew.FID_POISSON_PROX, x, y, self.gain, gamma=gamma, denormalize=self.denormalize)
        if self.denormalize:
            y = y / self.gain
        out = x - (1 / (self.gain * gamma)) * ((x - (1 / (self.gain * gamma))).pow(2) + 4 * y / gamma).sqrt()
        return out / 2


class L1Distance(Distance):
    r""":math:`\|x-y\|_1` (distance.py:266-323)."""

    def __init__(self):
        super().__init__()

    def fn(self, x, y, *args, **kwargs):
        diff = x - y
        return torch.linalg.vector_norm(diff.view(diff.size(0), -1), ord=1, dim=1)

    def grad(self, x, y, *args, **kwargs):
        if ew.fidelity_eligible(x, y):
            return ew.fidelity_pointwise(ew.FID_L1_GRAD, x, y)
        return torch.sign(x - y)

    def prox(self, u, y, *args, gamma=1.0, **kwargs):
        if ew.fidelity_eligible(u, y, gamma):
            return ew.fidelity_pointwise(ew.FID_L1_PROX, u, y, gamma=gamma)
        return F.softshrink(u - y, lambd=gamma) + y


class AmplitudeLossDistance(Distance):
    r""":math:`\sum_i (\sqrt{u_i} - \sqrt{y_i})^2` for :class:`deepinv_amd.physics.PhaseRetrieval` (distance.py:326-369).  With a
    phase-retrieval operator of this package the gradient never exists as an array of its own: it is an epilogue of the forward
    launch (:meth:`deepinv_amd.optim.AmplitudeLoss.grad`)."""

    def __init__(self):
        super().__init__()

    def fn(self, u, y, *args, **kwargs):
        # the difference of two roots cancels where the fit is good, and the result is one number per batch entry: the roots, the
        # difference and the sum are taken in float64 and rounded once, so the loss carries the error of u alone
        x = torch.sqrt(u.double()) - torch.sqrt(y.double()) if u.dtype == torch.float32 else torch.sqrt(u) - torch.sqrt(y)
        return (torch.linalg.vector_norm(x, ord=2, dim=tuple(range(1, x.dim()))) ** 2).to(u.dtype)

    def grad(self, u, y, *args, epsilon: float = 1e-12, **kwargs):
        return 1 - torch.sqrt(y / (u + epsilon))


class LogPoissonLikelihoodDistance(Distance):
    r""":math:`N_0(1^\top e^{-\mu x} + \mu\, (e^{-\mu y})^\top x)` (distance.py:372-395); no closed-form prox."""

    def __init__(self, N0=1024.0, mu=1 / 50.0):
        super().__init__()
        self.mu = mu
        self.N0 = N0

    def fn(self, x, y, *args, **kwargs):
        out1 = torch.exp(-x * self.mu) * self.N0
        out2 = torch.exp(-y * self.mu) * self.N0 * (x * self.mu)
        return (out1 + out2).reshape(x.shape[0], -1).sum(dim=1)

    def grad(self, x, y, *args, **kwargs):
        """The reference differentiates ``fn`` by autograd (potential.py); outside autograd the same gradient is the analytic
        N0 mu (exp(-mu y) - exp(-mu x)) in one launch."""
        if ew.fidelity_eligible(x, y, self.N0, self.mu):
            return ew.fidelity_pointwise(ew.FID_LOGPOISSON_GRAD, x, y, self.N0, self.mu)
        return super().grad(x, y, *args, **kwargs)
