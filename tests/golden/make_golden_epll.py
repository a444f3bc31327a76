#!/usr/bin/env python
"""Golden vectors for the Gaussian-mixture patch prior and EPLL from the REAL reference (deepinv v0.4.1, oracle/ref_shim.py),
float32 on the CPU: GaussianMixtureModel.component_log_likelihoods / forward / classify on a patch matrix, with and without the
covariance regularisation (deepinv/optim/utils.py:261-312), EPLLDenoiser on a grey batch of two noise levels and on a colour image
(deepinv/models/epll.py), and EPLL with a BlurFFT physics, whose image solve is the conjugate gradient (deepinv/optim/epll.py).
Every model is a random mixture at the scale of images in [0, 1] (QR of randn, eigenvalues 0.1 logspace(-1, 0) times a factor
per component, means 0.5 + 0.3 randn), stored as the reference's own state dict: with eigenvalues down to 1e-3 the reference's
own fp32 scores (inverse covariances) are off by 1e-3 and no input of these sizes keeps every classification clear of a flip.

Beside every output: the spread of the reference's own fp32 result against its fp64 one, and - over the classifications of all
half-quadratic steps - the smallest fp64 gap between the best and the second component score and the largest fp32-against-fp64
difference of one of those two scores.  The script asserts gap >= 100 x difference, so no golden sits on a classification flip.

    python tests/golden/make_golden_epll.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_shim import import_reference  # noqa: E402

dinv = import_reference()
from deepinv.models import EPLLDenoiser  # noqa: E402
from deepinv.optim import EPLL  # noqa: E402
from deepinv.optim.utils import GaussianMixtureModel  # noqa: E402

g = torch.Generator().manual_seed(2011)
out = {}


def random_gmm(K, d):
    Q = torch.linalg.qr(torch.randn(K, d, d, generator=g, dtype=torch.float64))[0]
    lam = 0.1 * torch.logspace(-1, 0, d, dtype=torch.float64)[None] * (0.5 + torch.rand(K, 1, generator=g, dtype=torch.float64))
    cov = Q @ torch.diag_embed(lam) @ Q.transpose(1, 2)
    m = GaussianMixtureModel(K, d)
    m.set_cov(cov.float())
    m.mu.data = (0.5 + 0.3 * torch.randn(K, d, generator=g)).float()
    m.set_weights(torch.rand(K, generator=g) + 0.1)
    return m


def double_of(m):
    m64 = GaussianMixtureModel(m.n_components, m.dimension).double()
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    return m64


def save_state(tag, m):
    sd = m.state_dict()
    out[f"{tag}_sd_keys"] = np.array(list(sd.keys()))
    for k, v in sd.items():
        out[f"{tag}_sd_{k}"] = v.numpy()


class Margins:
    """wraps classify of an fp64 mixture: records the smallest top-two gap and the largest fp32-against-fp64 difference of a top-two score"""

    def __init__(self, m32, m64):
        self.m32, self.m64, self.gap, self.diff = m32, m64, float("inf"), 0.0
        m64.classify = self

    def __call__(self, x, cov_regularization=False):
        if cov_regularization:
            self.m32.set_cov_reg(self.m64._covariance_regularization)
        s64 = self.m64.component_log_likelihoods(x, cov_regularization) + torch.log(self.m64._weights[None])
        s32 = self.m32.component_log_likelihoods(x.float(), cov_regularization) + torch.log(self.m32._weights[None])
        top, at = s64.topk(2, dim=1)
        self.gap = min(self.gap, float((top[:, 0] - top[:, 1]).min()))
        self.diff = max(self.diff, float((s32.double().gather(1, at) - top).abs().max()))      # of the two scores that decide
        return s64.argmax(1)

    def clear(self):
        return self.gap >= 100 * self.diff

    def save(self, tag):
        out[f"{tag}_gap"], out[f"{tag}_score_diff"] = np.float64(self.gap), np.float64(self.diff)
        print(tag, "smallest top-two gap", self.gap, "largest fp32 - fp64 score difference", self.diff)
        assert self.clear(), (tag, self.gap, self.diff)


# ------------------------------------------------------------------ the mixture on a patch matrix
ga = random_gmm(8, 16)
save_state("a", ga)
ga64 = double_of(ga)


def mixture_rows(m64, n, keep, reg):
    """`keep` of n rows drawn from the mixture itself: those whose fp64 top-two gap, with and without `reg`, is largest (a
    choice made from fp64 alone)"""
    k = torch.randint(0, m64.n_components, (n,), generator=g)
    L = torch.linalg.cholesky(m64._cov)
    x = (m64.mu[k] + torch.einsum("nij,nj->ni", L[k], torch.randn(n, m64.dimension, generator=g, dtype=torch.float64))).float().double()
    gaps = []
    for use in (False, True):
        m64.set_cov_reg(reg)
        top = (m64.component_log_likelihoods(x, use) + torch.log(m64._weights[None])).topk(2, dim=1).values
        gaps.append(top[:, 0] - top[:, 1])
    order = torch.minimum(*gaps).argsort(descending=True)[:keep]
    return x[order.sort().values].float()


X = mixture_rows(ga64, 96, 37, 0.05)
out["rows_x"] = X.numpy()
mg = Margins(ga, ga64)
for reg, tag in ((None, "rows"), (0.05, "rows_reg")):
    if reg is not None:
        ga.set_cov_reg(reg)
        ga64.set_cov_reg(reg)
        out["rows_reg"] = np.float64(reg)
    use = reg is not None
    cll, cll64 = ga.component_log_likelihoods(X, use), ga64.component_log_likelihoods(X.double(), use)
    cls = ga.classify(X, use)
    assert torch.equal(cls, ga64.classify(X.double(), use))
    out[f"{tag}_cll"], out[f"{tag}_cls"] = cll.numpy(), cls.numpy()
    out[f"{tag}_cll_spread"] = np.float64((cll.double() - cll64).abs().max())
    print(tag, "cll", tuple(cll.shape), "spread", out[f"{tag}_cll_spread"])
nll, nll64 = ga(X), ga64(X.double())
out["rows_nll"], out["rows_nll_spread"] = nll.numpy(), np.float64((nll.double() - nll64).abs().max())
print("nll spread", out["rows_nll_spread"])
mg.save("rows")


# ------------------------------------------------------------------ EPLLDenoiser and EPLL
def clear_input(tag, run64, shape):
    """the first of a sequence of seeded inputs whose fp64 run keeps every classification clear of a flip (Margins.clear): with a
    few thousand classifications per run, one in a few random inputs does"""
    for seed in range(200):
        gs = torch.Generator().manual_seed(seed)
        x = torch.rand(shape, generator=gs)
        mg, y, res64 = run64(x, gs)
        if mg.clear():
            out[f"{tag}_seed"] = np.int64(seed)
            return mg, y, res64
        print(tag, "seed", seed, "gap / difference", mg.gap / mg.diff)
    raise SystemExit(f"{tag}: no clear input among 200 seeds")


def denoise(tag, m, p, C, shape, sigma):
    def run64(x, gs):
        y = (x + sigma.view(-1, 1, 1, 1) * torch.randn(x.shape, generator=gs)).float()
        m64 = double_of(m)
        mg = Margins(double_of(m).float(), m64)
        return mg, y, EPLLDenoiser(GMM=m64, pretrained=None, patch_size=p, channels=C)(y.double(), sigma.double())

    mg, y, res64 = clear_input(tag, run64, shape)
    res = EPLLDenoiser(GMM=m, pretrained=None, patch_size=p, channels=C)(y, sigma)
    out[f"{tag}_y"], out[f"{tag}_sigma"], out[f"{tag}_out"] = y.numpy(), sigma.numpy(), res.numpy()
    out[f"{tag}_spread"] = np.float64((res.double() - res64).abs().max())
    print(tag, tuple(res.shape), "spread", out[f"{tag}_spread"], "range", float(res.min()), float(res.max()))
    mg.save(tag)


denoise("den_a", ga, 4, 1, (2, 1, 19, 22), torch.tensor([0.1, 0.05]))
gb = random_gmm(6, 27)
save_state("b", gb)
denoise("den_b", gb, 3, 3, (1, 3, 14, 17), torch.tensor([0.08]))

# EPLL with a circular Gaussian blur: the image solve is the conjugate gradient
filt = dinv.physics.blur.gaussian_blur(sigma=(1.0, 1.0))
physics = dinv.physics.BlurFFT(img_size=(1, 19, 22), filter=filt)
physics64 = dinv.physics.BlurFFT(img_size=(1, 19, 22), filter=filt.double())


def run64_blur(x, gs):
    y = (physics.A(x) + 0.05 * torch.randn(x.shape, generator=gs)).float()
    m64 = double_of(ga)
    mg = Margins(double_of(ga).float(), m64)
    return mg, y, EPLL(GMM=m64, pretrained=None, patch_size=4, channels=1)(y.double(), physics64, sigma=0.05)


mg, y, res64 = clear_input("blur", run64_blur, (1, 1, 19, 22))
res = EPLL(GMM=ga, pretrained=None, patch_size=4, channels=1)(y, physics, sigma=0.05)
out["blur_filter"], out["blur_y"], out["blur_sigma"], out["blur_out"] = filt.numpy(), y.numpy(), np.float64(0.05), res.numpy()
out["blur_spread"] = np.float64((res.double() - res64).abs().max())
print("blur", tuple(res.shape), "spread", out["blur_spread"])
mg.save("blur")

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "epll.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
