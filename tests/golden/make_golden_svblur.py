#!/usr/bin/env python
"""Golden vectors for SpaceVaryingBlur from the REAL reference (deepinv v0.4.1, oracle/ref_shim.py), float32 on the CPU:
SpaceVaryingBlur.A / A_adjoint (deepinv/physics/blur.py:740-868, functional/product_convolution.py) in the five padding modes,
with parameters from the reference's own generators (ProductConvolutionBlurGenerator over DiffractionBlurGenerator and
MotionBlurGenerator, deepinv/physics/generator/blur.py:1050-1177) and one random-parameter case with mixed broadcasting, and a
PGD + TVPrior loop on a generated reflect-padded operator together with the fp32-against-fp64 spread of the reference's own loop.

    python tests/golden/make_golden_svblur.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_shim import import_reference  # noqa: E402

dinv = import_reference()
from deepinv.optim.prior import TVPrior  # noqa: E402
from deepinv.physics.generator import (DiffractionBlurGenerator, MotionBlurGenerator,  # noqa: E402
                                       ProductConvolutionBlurGenerator)

MODES = ("valid", "circular", "reflect", "replicate", "constant")
g = torch.Generator().manual_seed(740)
out = {}


def operator_case(tag, x, filters, multipliers):
    out[f"{tag}_x"], out[f"{tag}_filters"], out[f"{tag}_multipliers"] = x.numpy(), filters.numpy(), multipliers.numpy()
    for mode in MODES:
        p = dinv.physics.SpaceVaryingBlur(filters=filters, multipliers=multipliers, padding=mode)
        y = p.A(x)
        v = torch.randn(y.shape, generator=g)
        xt = p.A_adjoint(v)
        lhs, rhs = float((y.double() * v.double()).sum()), float((x.double() * xt.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0), (tag, mode, lhs, rhs)
        out[f"{tag}_{mode}_y"], out[f"{tag}_{mode}_v"], out[f"{tag}_{mode}_adj"] = y.numpy(), v.numpy(), xt.numpy()
        print(tag, mode, tuple(y.shape), "dot", lhs, rhs)


# parameters from the reference's generators
gen = ProductConvolutionBlurGenerator(DiffractionBlurGenerator((7, 7), fc=0.25), img_size=(32, 24), n_eigen_psf=4)
params = gen.step(2, seed=1)
operator_case("diffraction", torch.randn(2, 1, 32, 24, generator=g), params["filters"].float().contiguous(),
              params["multipliers"].float().contiguous())
gen = ProductConvolutionBlurGenerator(MotionBlurGenerator((9, 9)), img_size=(32, 24), n_eigen_psf=5, spacing=(8, 6))
params = gen.step(1, seed=2)
operator_case("motion", torch.randn(1, 1, 32, 24, generator=g), params["filters"].float().contiguous(),
              params["multipliers"].float().contiguous())
# random parameters, mixed broadcasting: multipliers shared by the batch, filters shared by the channels
operator_case("mixed", torch.randn(2, 3, 20, 18, generator=g), torch.randn(2, 1, 3, 5, 4, generator=g),
              torch.randn(1, 3, 3, 20, 18, generator=g))

# PGD + TVPrior, 10 iterations on a generated reflect-padded operator (K = 5, 9 x 9 filters); the same loop in fp64 gives the
# spread of the reference's own arithmetic
gen = ProductConvolutionBlurGenerator(MotionBlurGenerator((9, 9)), img_size=(48, 40), n_eigen_psf=5)
params = gen.step(1, seed=3)
filters, multipliers = params["filters"].float().contiguous(), params["multipliers"].float().contiguous()
x = torch.zeros(1, 1, 48, 40)
x[..., 10:30, 8:25] = 1.0
x[..., 20:40, 18:34] += 0.5
x = x + 0.05 * torch.rand(1, 1, 48, 40, generator=g)
recs = {}
for dt in (torch.float32, torch.float64):
    p = dinv.physics.SpaceVaryingBlur(filters=filters.to(dt), multipliers=multipliers.to(dt), padding="reflect")
    if dt == torch.float32:
        y = p.A(x) + 0.01 * torch.randn(1, 1, 48, 40, generator=g)
    model = dinv.optim.PGD(prior=TVPrior(n_it_max=20), data_fidelity=dinv.optim.L2(), stepsize=1.0, lambda_reg=0.02, max_iter=10,
                           early_stop=False)
    with torch.no_grad():
        recs[dt] = model(y.to(dt), p)
spread = float((recs[torch.float32].double() - recs[torch.float64]).norm())
out.update(pgd_filters=filters.numpy(), pgd_multipliers=multipliers.numpy(), pgd_y=y.numpy(), pgd_rec=recs[torch.float32].numpy(),
           pgd_spread_l2=np.float64(spread), pgd_rec_norm=np.float64(float(recs[torch.float64].norm())))
print("PGD: |rec32 - rec64|_2 =", spread, "of |rec|_2 =", float(recs[torch.float64].norm()))

np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "svblur.npz"), **out)
