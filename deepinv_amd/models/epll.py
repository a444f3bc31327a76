"""``EPLLDenoiser`` (reference deepinv/models/epll.py): EPLL with the identity as its operator.  Every half-quadratic step is three
launches of csrc/patch_gmm.hpp - classify, estimate, aggregate - with the image solve folded into the last one's epilogue."""
from __future__ import annotations

import torch

from ..optim.epll import EPLL, GaussianMixtureModel
from ..physics.forward import Denoising
from ..physics.noise import GaussianNoise
from .base import Denoiser


class EPLLDenoiser(Denoiser):
    r"""Expected Patch Log-Likelihood denoiser: :math:`\arg\min_x \|y-x\|^2 - \sum_i \log p(P_i x)` with a Gaussian-mixture patch
    prior.  Same signature as the reference, except that ``pretrained`` defaults to ``None`` and takes only the path of a ``.pt``
    state dict (this package fetches nothing from the network)."""

    def __init__(self, GMM: GaussianMixtureModel = None, n_components: int = 200, pretrained: str | None = None,
                 patch_size: int = 6, channels: int = 1, device=torch.device("cpu")):
        super().__init__()
        self.PatchGMM = EPLL(GMM, n_components, pretrained, patch_size, channels, device)
        self.denoising_operator = Denoising(GaussianNoise(0))

    def forward(self, x: torch.Tensor, sigma, betas=None, batch_size: int = -1) -> torch.Tensor:
        return self.PatchGMM(x, x_init=x.clone(), sigma=sigma, physics=self.denoising_operator, batch_size=batch_size, betas=betas)
