"""Noise models applied by ``Physics.forward`` only (reference deepinv/physics/noise.py:11-330, 417-505, 548-650, 704-769).

Gaussian noise on a HIP device is one fused pass (csrc/random.hip: Philox4x32-10 + Box-Muller, y = x + sigma n), and so are the
Poisson, Poisson-Gaussian and log-Poisson models (dinv_poisson_noise: an exact Poisson sampler on the same counter stream); on
other devices, and for tensors that record a gradient, it is the reference's torch expression.
"""
from __future__ import annotations

import torch
import torch.nn as nn


class NoiseModel(nn.Module):
    def __init__(self, noise_model=None, rng: torch.Generator | None = None):
        super().__init__()
        self._fn = noise_model
        self.rng = rng

    def forward(self, x, seed: int | None = None, **kwargs):
        self.rng_manual_seed(seed)
        return x if self._fn is None else self._fn(x)

    def rng_manual_seed(self, seed: int | None = None):
        if seed is not None:
            if self.rng is None:
                raise ValueError("seed given but the noise model has no random generator (rng=None)")
            self.rng.manual_seed(seed)

    def randn_like(self, x, seed: int | None = None):
        self.rng_manual_seed(seed)
        return torch.empty_like(x).normal_(generator=self.rng)

    def rand_like(self, x, seed: int | None = None):
        self.rng_manual_seed(seed)
        return torch.empty_like(x).uniform_(generator=self.rng)

    def update_parameters(self, **kwargs):
        """a Tensor / float / int keyword replaces the same-named buffer (noise.py:111-124)"""
        for key, value in kwargs.items():
            if value is not None and hasattr(self, key) and isinstance(value, (torch.Tensor, float, int)):
                self.register_buffer(key, self._float_to_tensor(value))

    def _float_to_tensor(self, value):
        if value is None:
            return value
        if isinstance(value, (float, int)):
            return torch.tensor(value, dtype=torch.float32)
        if isinstance(value, torch.Tensor):
            return value
        raise ValueError(f"Unsupported type for noise level. Expected float, int, or torch.Tensor, got {type(value)}.")


def _infer_device(candidates, default=torch.device("cpu")):
    """the one device of the tensors / generators among `candidates` (noise.py:972-1000)"""
    devices = {c.device for c in candidates if isinstance(c, (torch.Tensor, torch.Generator))}
    if len(devices) > 1:
        raise RuntimeError(f"Input tensors and Generator should be on the same device. Found devices: {devices}.")
    return devices.pop() if devices else default


def _per_sample(p, x):
    """a parameter broadcast against x as the reference does: p[(...,) + (None,) * (x.dim() - 1)]"""
    return p[(...,) + (None,) * (x.dim() - 1)]


class ZeroNoise(NoiseModel):
    def forward(self, x, *args, **kwargs):
        return x


class GaussianNoise(NoiseModel):
    r""":math:`y = x + \sigma\epsilon`, :math:`\epsilon\sim\mathcal N(0,I)` (noise.py:197-330)."""

    def __init__(self, sigma=0.1, rng: torch.Generator | None = None):
        super().__init__(rng=rng)
        self.register_buffer("sigma", self._as_sigma(sigma), persistent=True)

    @staticmethod
    def _as_sigma(sigma):
        if isinstance(sigma, torch.Tensor):
            return sigma.detach().clone().float()
        return torch.tensor(float(sigma))

    def forward(self, x, sigma=None, seed=None, **kwargs):
        if sigma is not None:
            self.sigma = self._as_sigma(sigma).to(self.sigma.device)
        s = self.sigma.to(x.device)
        if x.is_cuda and x.dtype == torch.float32 and not (torch.is_grad_enabled() and x.requires_grad) \
                and (s.numel() == 1 or s.numel() == x.shape[0]):
            from ..hip import random as hrand

            self.rng_manual_seed(seed)
            return hrand.gaussian_noise(x, s, self.rng)
        if s.ndim > 0 and s.numel() > 1:
            s = s.reshape(-1, *([1] * (x.ndim - 1)))
        return x + self.randn_like(x, seed=seed) * s

    def update_parameters(self, sigma=None, **kwargs):
        if sigma is not None:
            self.sigma = self._as_sigma(sigma).to(self.sigma.device)


class PoissonNoise(NoiseModel):
    r""":math:`y = \mathcal P(x / \gamma)`, times :math:`\gamma` when ``normalize`` (noise.py:417-505)."""

    def __init__(self, gain=1.0, normalize: bool = True, clip_positive: bool = False, rng: torch.Generator | None = None):
        device = _infer_device([gain, rng])
        super().__init__(rng=rng)
        self.register_buffer("normalize", torch.tensor(normalize, dtype=torch.bool))
        self.clip_positive = clip_positive
        self.register_buffer("gain", self._float_to_tensor(gain).to(device))

    def forward(self, x, gain=None, seed: int | None = None, **kwargs):
        self.update_parameters(gain=gain, **kwargs)
        self.rng_manual_seed(seed)
        self.to(x.device)
        from ..hip import random as hrand

        if hrand.poisson_eligible(x, self.gain):
            y, bad = hrand.poisson_noise(x, hrand.POISSON, self.gain, normalize=self._normalize_on_host(),
                                         clip_positive=self.clip_positive, gen=self.rng)
            self._raise(bad, "Poisson")
            return y
        gain = _per_sample(self.gain, x)
        if self.clip_positive:
            z = torch.clip(x / gain, min=0.0)
        else:
            self._raise([bool(torch.any(x < 0)), bool(torch.any(gain <= 0))], "Poisson")
            z = x / gain
        y = torch.poisson(z, generator=self.rng)
        if self.normalize:
            y = y * gain
        return y

    def _normalize_on_host(self) -> bool:
        """the `normalize` buffer as a Python bool, read from the device once per value (the buffer follows the module across devices)"""
        t = self.normalize
        seen = getattr(self, "_normalize_seen", None)
        if seen is None or seen[0] is not t or seen[1] != t._version:
            seen = self._normalize_seen = (t, t._version, bool(t))
        return seen[2]

    @staticmethod
    def _raise(bad, name):
        """the reference's two checks, in its order (noise.py:492-498, 638-644)"""
        if bad is None:
            return
        if bad[1]:
            raise ValueError(f"{name} noise gain must be positive.")
        if bad[0]:
            raise ValueError(f"Input tensor for {name} noise must be non-negative.\n"
                             "Consider setting ``clip_positive=True`` to avoid this error.")


class PoissonGaussianNoise(NoiseModel):
    r""":math:`y = \gamma z + \epsilon`, :math:`z\sim\mathcal P(x / \gamma)`, :math:`\epsilon\sim\mathcal N(0, \sigma^2 I)`
    (noise.py:548-650); a gain below ``min_gain`` is raised to it."""

    def __init__(self, gain=1.0, sigma=0.1, clip_positive: bool = False, min_gain=1e-12, rng: torch.Generator | None = None):
        device = _infer_device([gain, sigma, rng])
        super().__init__(rng=rng)
        self.clip_positive = clip_positive
        self.min_gain = min_gain
        self.register_buffer("gain", self._float_to_tensor(gain).to(device))
        self.register_buffer("sigma", self._float_to_tensor(sigma).to(device))

    def forward(self, x, gain=None, sigma=None, seed: int | None = None, **kwargs):
        self.update_parameters(gain=gain, sigma=sigma, **kwargs)
        self.rng_manual_seed(seed)
        self.to(x.device)
        from ..hip import random as hrand

        if hrand.poisson_eligible(x, self.gain, self.sigma) and isinstance(self.min_gain, (int, float)):
            y, bad = hrand.poisson_noise(x, hrand.POISSON_GAUSSIAN, self.gain, self.sigma, clip_positive=self.clip_positive,
                                         min_gain=self.min_gain, gen=self.rng)
            PoissonNoise._raise(bad, "Poisson-Gaussian")
            return y
        gain = torch.clip(_per_sample(self.gain, x), min=self.min_gain)
        sigma = _per_sample(self.sigma, x)
        if self.clip_positive:
            y = torch.poisson(torch.clip(x / gain, min=0.0), generator=self.rng) * gain
        else:
            PoissonNoise._raise([bool(torch.any(x < 0)), bool(torch.any(gain <= 0))], "Poisson-Gaussian")
            y = torch.poisson(x / gain, generator=self.rng) * gain
        return y + self.randn_like(x) * sigma


class LogPoissonNoise(NoiseModel):
    r""":math:`y = -\frac{1}{\mu}\log\big(\mathcal P(N_0 e^{-\mu x}) / N_0\big)` (noise.py:704-769): low-dose CT."""

    def __init__(self, N0=1024.0, mu=1 / 50.0, rng: torch.Generator | None = None):
        device = _infer_device([N0, mu, rng])
        super().__init__(rng=rng)
        self.register_buffer("mu", self._float_to_tensor(mu).to(device))
        self.register_buffer("N0", self._float_to_tensor(N0).to(device))

    def forward(self, x, mu=None, N0=None, seed: int | None = None, **kwargs):
        self.update_parameters(mu=mu, N0=N0, **kwargs)
        self.rng_manual_seed(seed)
        self.to(x.device)
        from ..hip import random as hrand

        if self.N0.numel() == 1 and self.mu.numel() == 1 and hrand.poisson_eligible(x, self.N0, self.mu):
            return hrand.poisson_noise(x, hrand.POISSON_LOG, self.N0, self.mu, gen=self.rng)[0]
        n1 = torch.poisson(self.N0 * torch.exp(-x * self.mu), generator=self.rng)
        return -torch.log(n1 / self.N0) / self.mu
