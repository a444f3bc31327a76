"""Priors (reference deepinv/optim/prior.py:22-109, 485-612)."""
from __future__ import annotations

import torch

from ..hip import tv as tv_kernels
from ..models.tv import TVDenoiser, TVL1Denoiser, check_tv_input
from .potential import Potential


class Prior(Potential):
    def __init__(self, g=None, *args, **kwargs):
        super().__init__(*args, fn=g, **kwargs)
        self.explicit_prior = self._fn is not None


class ZeroPrior(Prior):
    def __init__(self):
        super().__init__()
        self.explicit_prior = True

    def fn(self, x, *args, **kwargs):
        return torch.zeros(x.shape[0], device=x.device)

    def grad(self, x, *args, **kwargs):
        return torch.zeros_like(x)

    def prox(self, x, ths=1.0, gamma=1.0, *args, **kwargs):
        return x


class PnP(Prior):
    r"""Plug-and-play prior :math:`\operatorname{prox}_{\gamma g}(x) = D_\sigma(x)` (prior.py:86-109)."""

    def __init__(self, denoiser, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.denoiser = denoiser
        self.explicit_prior = False

    def prox(self, x, sigma_denoiser, *args, **kwargs):
        return self.denoiser(x, sigma_denoiser)


class TVPrior(Prior):
    r"""Total variation prior :math:`g(x) = \|Dx\|_{1,2}` (reference deepinv/optim/prior.py:485-582).

    ``fn`` is the per-sample sum of :math:`\|(Dx)_p\|_2` and ``grad`` the subgradient :math:`-\mathrm{div}(Dx/|Dx|)` with the
    zero element where :math:`|Dx| = 0`, each one launch of csrc/tv.hip; ``prox(x, gamma=...)`` is ``TVModel(x, ths=gamma)``,
    a :class:`~deepinv_amd.models.TVDenoiser` whose warm restart carries over between the outer iterations of a loop."""

    def __init__(self, def_crit=1e-8, n_it_max=1000, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.explicit_prior = True
        self.TVModel = TVDenoiser(crit=def_crit, n_it_max=n_it_max)

    def fn(self, x, *args, **kwargs):
        """prior.py:504-518"""
        return tv_kernels.fn(_tv_input(x), l1=False)

    def prox(self, x, *args, gamma=1.0, **kwargs):
        """prior.py:520-530"""
        return self.TVModel(x, ths=gamma)

    def nabla(self, x):
        return self.TVModel.nabla(x)

    def nabla_adjoint(self, x):
        return self.TVModel.nabla_adjoint(x)

    def grad(self, x, *args, **kwargs):
        """prior.py:550-582"""
        return tv_kernels.grad(_tv_input(x))


class TVL1Prior(TVPrior):
    r"""Anisotropic total variation prior :math:`g(x) = \|Dx\|_1` (reference deepinv/optim/prior.py:585-612): ``fn`` sums
    :math:`|Dx|` per sample and the prox is a :class:`~deepinv_amd.models.TVL1Denoiser`; ``grad`` is TVPrior's isotropic one,
    unchanged, as in the reference."""

    def __init__(self, def_crit=1e-8, n_it_max=1000, *args, **kwargs):
        super().__init__(def_crit=def_crit, n_it_max=n_it_max, *args, **kwargs)
        self.TVModel = TVL1Denoiser(crit=def_crit, n_it_max=n_it_max)

    def fn(self, x, *args, **kwargs):
        """prior.py:597-612"""
        return tv_kernels.fn(_tv_input(x), l1=True)


def _tv_input(x):
    x = check_tv_input(x, "TVPrior")
    if x.dim() not in (4, 5):
        raise ValueError(f"TVPrior takes [B,C,H,W] or [B,C,D,H,W] tensors, got shape {tuple(x.shape)}")
    return x
