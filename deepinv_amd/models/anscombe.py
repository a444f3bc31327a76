"""Generalized Anscombe transform and the denoiser wrapper built on it (reference deepinv/models/anscombe.py): any Gaussian
denoiser of the package (DRUNet, DnCNN, TV, TGV) becomes a Poisson-Gaussian denoiser.  Plain tensor arithmetic around the wrapped
denoiser, which brings its own kernels."""
from __future__ import annotations

import torch

from .base import Denoiser


def check_nonnegative(value, name):
    # (the reference's one-line test cannot take a tensor of several elements; per-sample gains and sigmas are welcome here)
    if bool(torch.any(value < 0)) if isinstance(value, torch.Tensor) else value < 0:
        raise ValueError(f"{name} should be positive. Got {value}.")


def generalized_anscombe_transform(x, gain, sigma):
    r""":math:`h(y) = 2\sqrt{\gamma y + \tfrac38\gamma^2 + \sigma^2}` (anscombe.py:5-37): Poisson-Gaussian data with gain
    :math:`\gamma` becomes approximately Gaussian with standard deviation :math:`\gamma`."""
    check_nonnegative(gain, "gain")
    check_nonnegative(sigma, "sigma")
    aux = gain * x + 3.0 / 8 * gain ** 2 + sigma ** 2
    return 2.0 * aux.clamp_min(0).sqrt()


def inverse_generalized_anscombe_transform(x, gain, sigma):
    """the closed-form approximation of the exact unbiased inverse (anscombe.py:40-81)"""
    check_nonnegative(gain, "gain")
    check_nonnegative(sigma, "sigma")
    x = x / gain
    return gain * (1 / 4 * x ** 2 + 1 / 4 * (3 / 2) ** 0.5 * x ** (-1) - 11 / 8 * x ** (-2) + 5 / 8 * (3 / 2) ** 0.5 * x ** (-3)
                   - 1 / 8 - sigma ** 2 / gain ** 2)


def _per_sample(value, y):
    """float / tensor / list -> [B, 1, ..., 1] on y's device (the reference's Denoiser._handle_sigma, models/base.py:48-116)"""
    if isinstance(value, (float, int)):
        value = torch.tensor([float(value)] * y.size(0), dtype=y.dtype, device=y.device)
    elif isinstance(value, torch.Tensor):
        value = value.squeeze().to(dtype=y.dtype, device=y.device)
    elif isinstance(value, list):
        value = torch.tensor(value, dtype=y.dtype, device=y.device).squeeze()
    else:
        raise TypeError(f"Sigma must be a float, int, or torch.Tensor. Got {type(value)}.")
    if value.ndim == 0 or (value.ndim == 1 and value.size(0) == 1):
        value = value.reshape(1).expand(y.size(0))
    elif value.ndim != 1:
        raise ValueError(f"Sigma tensor has {value.ndim} dimensions, expected 0 or 1.")
    elif value.size(0) != y.size(0):
        raise ValueError(f"Sigma tensor size {value.size(0)} does not match batch size {y.size(0)}.")
    return value.view(-1, *([1] * (y.ndim - 1)))


class AnscombeDenoiser(Denoiser):
    """GAT, the wrapped Gaussian denoiser at noise level ``gain``, inverse GAT (anscombe.py:89-194); ``gain=None`` calls the
    wrapped denoiser directly."""

    def __init__(self, denoiser, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.denoiser = denoiser

    def forward(self, y, sigma, gain=None, *args, **kwargs):
        if gain is None:
            return self.denoiser(y, sigma, *args, **kwargs)
        sigma = _per_sample(sigma, y)
        gain = _per_sample(gain, y)
        z = generalized_anscombe_transform(y, gain, sigma)
        z_denoised = self.denoiser(z, *args, sigma=gain, **kwargs)
        return inverse_generalized_anscombe_transform(z_denoised, gain, sigma)
