#!/usr/bin/env python
"""Golden vectors for total variation from the REAL reference (deepinv v0.4.1, oracle/ref_shim.py), float32 on the CPU:
TVDenoiser (deepinv/models/tv.py:5-218) in 2-D and 3-D with a fixed iteration count (crit = 0) and with the early stop
(the iteration count at which the reference broke is recorded), a batch of two different images with per-sample ths, two
consecutive calls on one instance (warm restart), TVL1Denoiser (tv.py:221-240), TVPrior.fn / grad and TVL1Prior.fn
(deepinv/optim/prior.py:485-612), nabla / nabla_adjoint, and two PGD + TVPrior loops (BlurFFT deblurring as in
examples/optimization/demo_TV_minimisation.py, and single-coil MRI).

    python tests/golden/make_golden_tv.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_shim import import_reference  # noqa: E402

dinv = import_reference()
from deepinv.models.tv import TVDenoiser, TVL1Denoiser  # noqa: E402
from deepinv.optim.prior import TVL1Prior, TVPrior  # noqa: E402

g = torch.Generator().manual_seed(2024)
out = {}


def counted(den, *args, **kwargs):
    """den(*args) and the number of iterations it ran (one nabla call per iteration, tv.py:134)"""
    calls = [0]
    orig = TVDenoiser.nabla

    def nabla(x):
        calls[0] += 1
        return orig(x)

    den.nabla = nabla
    try:
        r = den(*args, **kwargs)
    finally:
        del den.nabla
    return r, calls[0]


def denoiser_case(tag, cls, y, ths, n_it_max, crit):
    den = cls(n_it_max=n_it_max, crit=crit)
    r, n = counted(den, y, ths=ths)
    out[f"{tag}_y"], out[f"{tag}_out"], out[f"{tag}_u2"] = y.numpy(), r.numpy(), den.u2.numpy()
    out[f"{tag}_ths"] = np.asarray(ths, dtype=np.float32)
    out[f"{tag}_nit"] = np.int64(n)
    out[f"{tag}_nitmax"], out[f"{tag}_crit"] = np.int64(n_it_max), np.float64(crit)
    print(tag, tuple(y.shape), "iterations", n)


# fixed iteration counts (crit = 0)
denoiser_case("fixed2d", TVDenoiser, torch.rand(2, 3, 20, 23, generator=g), [0.05, 0.2], 60, 0.0)
denoiser_case("fixed3d", TVDenoiser, torch.rand(1, 2, 6, 10, 9, generator=g), 0.1, 40, 0.0)
denoiser_case("l1fixed2d", TVL1Denoiser, torch.rand(2, 2, 16, 17, generator=g), [0.1, 0.03], 60, 0.0)
denoiser_case("l1fixed3d", TVL1Denoiser, torch.rand(1, 1, 5, 9, 8, generator=g), 0.05, 40, 0.0)
# the early stop (crit = 1e-5, the default)
denoiser_case("stop2d", TVDenoiser, torch.rand(1, 3, 24, 21, generator=g), 0.1, 1000, 1e-5)
denoiser_case("stop3d", TVDenoiser, torch.rand(1, 1, 6, 12, 11, generator=g), 0.1, 1000, 1e-5)
denoiser_case("l1stop2d", TVL1Denoiser, torch.rand(1, 2, 18, 19, generator=g), 0.05, 1000, 1e-5)
# a batch of two different images with per-sample ths: the batch norm of the stopping rule couples them
y0 = torch.rand(1, 1, 24, 24, generator=g)
y1 = torch.zeros(1, 1, 24, 24)
y1[..., 6:18, 6:18] = 1.0
y1 += 0.2 * torch.randn(1, 1, 24, 24, generator=g)
denoiser_case("batch", TVDenoiser, torch.cat([y0, y1]), [0.05, 0.3], 1000, 1e-5)
denoiser_case("batch_first", TVDenoiser, y0.clone(), [0.05], 1000, 1e-5)

# warm restart: two consecutive calls on one instance
den = TVDenoiser(n_it_max=50, crit=1e-5)
wy1 = torch.rand(2, 1, 19, 22, generator=g)
wy2 = (wy1 + 0.05 * torch.randn(2, 1, 19, 22, generator=g)).contiguous()
r1, n1 = counted(den, wy1, ths=0.1)
r2, n2 = counted(den, wy2, ths=0.1)
out.update(warm_y1=wy1.numpy(), warm_y2=wy2.numpy(), warm_out1=r1.numpy(), warm_out2=r2.numpy(), warm_u2=den.u2.numpy(),
           warm_nit=np.array([n1, n2], dtype=np.int64))
print("warm iterations", n1, n2)

# priors, finite differences
for tag, shape in (("2d", (2, 3, 15, 13)), ("3d", (2, 1, 5, 7, 6))):
    x = torch.randn(shape, generator=g)
    x[..., ::3, :] = 0.0                       # flat stretches: |Dx| = 0 somewhere (the zero subgradient branch)
    x[:, :, 1:3] = x[:, :, 1:2]
    v = torch.randn(*shape, len(shape) - 2, generator=g)
    out[f"prior{tag}_x"], out[f"prior{tag}_v"] = x.numpy(), v.numpy()
    out[f"prior{tag}_fn"] = TVPrior().fn(x).numpy()
    out[f"prior{tag}_grad"] = TVPrior().grad(x).numpy()
    out[f"prior{tag}_l1fn"] = TVL1Prior().fn(x).numpy()
    out[f"prior{tag}_l1grad"] = TVL1Prior().grad(x).numpy()
    out[f"prior{tag}_nabla"] = TVDenoiser.nabla(x).numpy()
    out[f"prior{tag}_nabla_adjoint"] = TVDenoiser.nabla_adjoint(v).numpy()

# PGD + TVPrior loops
x = torch.rand(1, 3, 64, 64, generator=g)
h = dinv.physics.functional.blur.gaussian_blur(sigma=(2.0, 2.0))
p = dinv.physics.BlurFFT(img_size=(3, 64, 64), filter=h)
y = p.A(x) + 0.02 * torch.randn(1, 3, 64, 64, generator=g)
model = dinv.optim.PGD(prior=TVPrior(n_it_max=100), data_fidelity=dinv.optim.L2(), stepsize=1.0, lambda_reg=0.05, max_iter=30,
                       early_stop=False)
with torch.no_grad():
    rec = model(y, p)
out.update(blur_filter=h.numpy(), blur_y=y.numpy(), blur_rec=rec.numpy())
print("blur PGD", float(rec.sum()))

xm = torch.rand(1, 2, 64, 64, generator=g)
mask = (torch.rand(64, 64, generator=g) < 0.4).float()
mask[28:36, :] = 1.0
pm = dinv.physics.MRI(mask=mask, img_size=(2, 64, 64))
ym = pm.A(xm)
model = dinv.optim.PGD(prior=TVPrior(n_it_max=100), data_fidelity=dinv.optim.L2(), stepsize=1.0, lambda_reg=0.02, max_iter=30,
                       early_stop=False)
with torch.no_grad():
    recm = model(ym, pm)
out.update(mri_mask=mask.numpy(), mri_y=ym.numpy(), mri_rec=recm.numpy())
print("MRI PGD", float(recm.sum()))

np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tv.npz"), **out)
