#!/usr/bin/env python
"""Golden vectors for the Poisson-family noise models, likelihoods and the Anscombe wrapper from the REAL reference (deepinv v0.4.1,
oracle/ref_shim.py), float32 on the CPU: fn / grad / prox of PoissonLikelihoodDistance, L1Distance and
LogPoissonLikelihoodDistance and of the fidelities built on them (over Denoising), the generalized Anscombe transform and its
inverse, AnscombeDenoiser around a closed-form denoiser, histograms of LogPoissonNoise and PoissonGaussianNoise samples (for a
two-sample test of the device sampler), and a PGD + PoissonLikelihood + TVPrior reconstruction on a 32 x 32 SinglePixelCamera.

    python tests/golden/make_golden_poisson.py
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_shim import import_reference  # noqa: E402

dinv = import_reference()
from deepinv.models.anscombe import (AnscombeDenoiser, generalized_anscombe_transform,  # noqa: E402
                                     inverse_generalized_anscombe_transform)
from deepinv.models.base import Denoiser  # noqa: E402
from deepinv.optim.distance import L1Distance, LogPoissonLikelihoodDistance, PoissonLikelihoodDistance  # noqa: E402
from deepinv.optim.prior import TVPrior  # noqa: E402
from deepinv.physics.singlepixel import SinglePixelCamera  # noqa: E402

g = torch.Generator().manual_seed(417)
out = {}

# ---- distances and fidelities on a small positive case
x = torch.rand(2, 1, 8, 8, generator=g) * 4 + 0.2
y = torch.poisson(x * 2, generator=g) / 2
out.update(x=x.numpy(), y=y.numpy())
GAIN, BKG, N0, MU = 0.5, 0.1, 1024.0, 1 / 50.0
out.update(gain=np.float64(GAIN), bkg=np.float64(BKG), N0=np.float64(N0), mu=np.float64(MU))
physics = dinv.physics.Denoising(dinv.physics.ZeroNoise())
for denorm in (False, True):
    d = PoissonLikelihoodDistance(gain=GAIN, bkg=BKG, denormalize=denorm)
    t = f"pl{int(denorm)}"
    out[f"{t}_fn"], out[f"{t}_grad"] = d.fn(x, y).numpy(), d.grad(x, y).numpy()
    out[f"{t}_prox"] = d.prox(x, y, gamma=0.7).numpy()
f = dinv.optim.PoissonLikelihood(gain=GAIN, bkg=BKG)                      # denormalize defaults to True here
assert f.d.denormalize is True and PoissonLikelihoodDistance().denormalize is False
out["plf_fn"], out["plf_grad"] = f.fn(x, y, physics).numpy(), f.grad(x, y, physics).numpy()
out["plf_prox_d"] = f.prox_d(x, y, gamma=1.3).numpy()
d = L1Distance()
out["l1_fn"], out["l1_grad"], out["l1_prox"] = d.fn(x, y).numpy(), d.grad(x, y).numpy(), d.prox(x, y, gamma=0.4).numpy()
f = dinv.optim.L1()
out["l1f_fn"], out["l1f_grad"] = f.fn(x, y, physics).numpy(), f.grad(x, y, physics).numpy()
d = LogPoissonLikelihoodDistance(N0=N0, mu=MU)
xl, yl = x * 40, y * 40
out["lp_fn"] = d.fn(xl, yl).numpy()
out["lp_grad"] = d.grad(xl.clone(), yl).detach().numpy()                 # autograd in the reference
f = dinv.optim.LogPoissonLikelihood(N0=N0, mu=MU)
out["lpf_fn"], out["lpf_grad"] = f.fn(xl, yl, physics).numpy(), f.grad(xl.clone(), yl, physics).detach().numpy()

# ---- Anscombe
# (the reference's check_nonnegative cannot take a tensor of more than one element, so its wrapper serves a batch of one: the
# per-sample values of a larger batch are recorded sample by sample)
sig_b, gain_b = [0.1, 0.3], [0.5, 0.2]
out["gat"] = generalized_anscombe_transform(y, 0.5, 0.1).numpy()
out["igat"] = inverse_generalized_anscombe_transform(torch.from_numpy(out["gat"]), 0.5, 0.1).numpy()


class Shrink(Denoiser):
    """a closed-form stand-in for a Gaussian denoiser"""

    def forward(self, u, sigma, **kwargs):
        return u / (1 + sigma * sigma)


out["ansc"] = torch.cat([AnscombeDenoiser(Shrink())(y[b:b + 1], 0.1, 0.5) for b in range(2)]).numpy()
out["ansc_b"] = torch.cat([AnscombeDenoiser(Shrink())(y[b:b + 1], sig_b[b], gain_b[b]) for b in range(2)]).numpy()
out["ansc_b_sigma"], out["ansc_b_gain"] = np.array(sig_b), np.array(gain_b)
out["ansc_none"] = AnscombeDenoiser(Shrink())(y, 0.2).numpy()

# ---- histograms of the reference's samplers (two-sample chi-square on the device side)
NS = 200_000
rng = torch.Generator().manual_seed(99)
yl = dinv.physics.LogPoissonNoise(N0=N0, mu=MU, rng=rng)(torch.full((NS,), 100.0))
k = torch.round(N0 * torch.exp(-MU * yl.double())).long()
out["hist_lp_x"], out["hist_lp_n"] = np.float64(100.0), np.int64(NS)
out["hist_lp_counts"] = torch.bincount(k, minlength=256)[:256].numpy().astype(np.int32)
assert int(k.max()) < 256
ypg = dinv.physics.PoissonGaussianNoise(gain=0.5, sigma=0.3, rng=rng)(torch.full((NS,), 3.0))
edges = np.linspace(-1.5, 10.5, 97)
out["hist_pg_x"], out["hist_pg_gain"], out["hist_pg_sigma"], out["hist_pg_n"] = np.float64(3.0), np.float64(0.5), np.float64(0.3), np.int64(NS)
out["hist_pg_edges"] = edges
out["hist_pg_counts"] = np.histogram(np.clip(ypg.numpy(), edges[0], edges[-1]), bins=edges)[0].astype(np.int32)

# ---- PGD + PoissonLikelihood(gain, bkg > 0) + TVPrior on a 32 x 32 sequency camera; the measurement is stored, nothing random is compared
xx, yy = torch.meshgrid(torch.linspace(-1, 1, 32), torch.linspace(-1, 1, 32), indexing="ij")
img = (0.2 + (xx ** 2 + yy ** 2 < 0.5).float() * 0.5 + ((xx.abs() < 0.3) & (yy.abs() < 0.6)).float() * 0.3).view(1, 1, 32, 32)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    p = SinglePixelCamera(m=400, img_size=(1, 32, 32))
PG_GAIN, PG_BKG = 0.02, 400.0
clean = p.A(img)
ym = dinv.physics.PoissonNoise(gain=PG_GAIN, normalize=True, clip_positive=True, rng=rng)(clean + PG_BKG * PG_GAIN) * p.mask
print("measurement range", float(clean.min()), float(clean.max()), "min rate", float((clean / PG_GAIN + PG_BKG).min()))
model = dinv.optim.PGD(prior=TVPrior(n_it_max=30), data_fidelity=dinv.optim.PoissonLikelihood(gain=PG_GAIN, bkg=PG_BKG),
                       stepsize=100.0, lambda_reg=0.01, max_iter=30, early_stop=False)
with torch.no_grad():
    rec = model(ym, p)
assert bool(torch.isfinite(rec).all())
out.update(pgd_y=ym.numpy(), pgd_rec=rec.numpy(), pgd_m=np.int64(400), pgd_gain=np.float64(PG_GAIN), pgd_bkg=np.float64(PG_BKG),
           pgd_img=img.numpy())
print("PGD + PoissonLikelihood + TVPrior: mse to the image", float(((rec - img) ** 2).mean()), "of A_dagger",
      float(((p.A_dagger(ym - PG_BKG * PG_GAIN * p.mask) - img) ** 2).mean()))

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "poisson.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
