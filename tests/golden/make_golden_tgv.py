#!/usr/bin/env python
"""Golden vectors for total generalized variation from the REAL reference (deepinv v0.4.1, oracle/ref_shim.py), float32 on
the CPU: TGVDenoiser (deepinv/models/tgv.py:7-310) in 2-D and 3-D with a fixed iteration count (crit = 0) and with the
early stop (the iteration count at which the reference broke is recorded), two consecutive calls on one instance (warm
restart), epsilon / epsilon_adjoint, and a short PGD + PnP(TGVDenoiser) deblurring on BlurFFT.

Early-stop cases: crit is chosen from the reference's own rel_err sequence so that the stopping iteration's rel_err is at
least 2 % below crit and every earlier candidate's (index > 1) at least 2 % above it: a reordered fp32 sum cannot move
the count.

    python tests/golden/make_golden_tgv.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_shim import import_reference  # noqa: E402

dinv = import_reference()
from deepinv.models.tgv import TGVDenoiser  # noqa: E402

g = torch.Generator().manual_seed(2025)
out = {}


def counted(den, *args, record=None, **kwargs):
    """den(*args) and the number of iterations it ran: epsilon is called once per iteration when not verbose
    (tgv.py:152-156).  With `record`, the iterate x2 at the start of every iteration is appended to it."""
    calls = [0]
    orig_eps, orig_adj = TGVDenoiser.epsilon, TGVDenoiser.epsilon_adjoint

    def epsilon(v):
        calls[0] += 1
        return orig_eps(v)

    def epsilon_adjoint(u):
        if record is not None:
            record.append(den.x2.clone())
        return orig_adj(u)

    den.epsilon, den.epsilon_adjoint = epsilon, epsilon_adjoint
    try:
        r = den(*args, **kwargs)
    finally:
        del den.epsilon, den.epsilon_adjoint
    return r, calls[0]


def pick_crit(y, ths, target, n_probe=200):
    """a crit that stops the reference at iteration index `target` or later, with a 2 % margin on both sides"""
    den = TGVDenoiser(n_it_max=n_probe, crit=0.0)
    xs = []
    r, _ = counted(den, y, ths=ths, record=xs)
    xs.append(r.clone())
    rel = [float(torch.linalg.norm(xs[k].flatten() - xs[k + 1].flatten()) / (torch.linalg.norm(xs[k + 1].flatten()) + 1e-12))
           for k in range(n_probe)]
    for k in range(max(target, 2), n_probe):
        hi = min(rel[2:k], default=float("inf"))
        if rel[k] < hi / 1.05:
            crit = (rel[k] * hi) ** 0.5 if hi != float("inf") else rel[k] * 1.05
            assert rel[k] < crit / 1.02 and hi > crit * 1.02
            return crit, k + 1
    raise RuntimeError("no stopping index with a margin")


def denoiser_case(tag, y, ths, n_it_max, crit, nit_expected=None):
    den = TGVDenoiser(n_it_max=n_it_max, crit=crit)
    r, n = counted(den, y, ths=ths)
    if nit_expected is not None:
        assert n == nit_expected, (n, nit_expected)
    out[f"{tag}_y"], out[f"{tag}_out"] = y.numpy(), r.numpy()
    out[f"{tag}_r2"], out[f"{tag}_u2"] = den.r2.numpy(), den.u2.numpy()
    out[f"{tag}_ths"] = np.asarray(ths, dtype=np.float32)
    out[f"{tag}_nit"] = np.int64(n)
    out[f"{tag}_nitmax"], out[f"{tag}_crit"] = np.int64(n_it_max), np.float64(crit)
    out[f"{tag}_converged"] = np.bool_(den.has_converged)
    print(tag, tuple(y.shape), "crit", crit, "iterations", n)


# fixed iteration counts (crit = 0): an odd 2-D shape with a batch of two and per-sample ths, and a volume
denoiser_case("fixed2d", torch.rand(2, 3, 21, 23, generator=g), [0.05, 0.3], 40, 0.0)
denoiser_case("fixed3d", torch.rand(1, 2, 6, 9, 7, generator=g), 0.2, 30, 0.0)
# early stops at a crit with margin.  tau = 0.01 makes the steps small and rel_err oscillates between even and odd
# indices: it is lowest at index 2 for hundreds of iterations, so a stop comes either at index 2 or very late.
for tag, y, ths, target, n_probe in (
        ("stop2d", torch.rand(2, 3, 20, 23, generator=g), [0.1, 0.2], 2, 10),
        ("stop3d", torch.rand(1, 1, 6, 10, 9, generator=g), 0.2, 2, 10),
        ("stop2d_late", torch.rand(2, 1, 10, 11, generator=torch.Generator().manual_seed(3)), [0.1, 0.3], 3, 2600)):
    crit, nit = pick_crit(y, ths, target, n_probe)
    denoiser_case(tag, y, ths, 3000, crit, nit)

# warm restart: two consecutive calls on one instance
den = TGVDenoiser(n_it_max=25, crit=0.0)
wy1 = torch.rand(2, 1, 19, 22, generator=g)
wy2 = (wy1 + 0.05 * torch.randn(2, 1, 19, 22, generator=g)).contiguous()
r1, n1 = counted(den, wy1, ths=0.2)
r2, n2 = counted(den, wy2, ths=0.2)
out.update(warm_y1=wy1.numpy(), warm_y2=wy2.numpy(), warm_out1=r1.numpy(), warm_out2=r2.numpy(), warm_r2=den.r2.numpy(),
           warm_u2=den.u2.numpy(), warm_nit=np.array([n1, n2], dtype=np.int64))
print("warm iterations", n1, n2)

# epsilon / epsilon_adjoint
for tag, shape in (("2d", (2, 3, 15, 13)), ("3d", (2, 1, 5, 7, 6))):
    nd = len(shape) - 2
    v = torch.randn(*shape, nd, generator=g)
    u = torch.randn(*shape, nd * nd, generator=g)
    out[f"eps{tag}_v"], out[f"eps{tag}_u"] = v.numpy(), u.numpy()
    out[f"eps{tag}_eps"] = TGVDenoiser.epsilon(v).numpy()
    out[f"eps{tag}_adj"] = TGVDenoiser.epsilon_adjoint(u).numpy()

# PGD + PnP(TGVDenoiser) deblurring on a small BlurFFT (fixed inner counts: crit = 0)
x = torch.rand(1, 3, 32, 32, generator=g)
h = dinv.physics.functional.blur.gaussian_blur(sigma=(1.5, 1.5))
p = dinv.physics.BlurFFT(img_size=(3, 32, 32), filter=h)
y = p.A(x) + 0.02 * torch.randn(1, 3, 32, 32, generator=g)
model = dinv.optim.PGD(prior=dinv.optim.PnP(TGVDenoiser(n_it_max=30, crit=0.0)), data_fidelity=dinv.optim.L2(), stepsize=1.0,
                       g_param=0.1, max_iter=8, early_stop=False)
with torch.no_grad():
    rec = model(y, p)
out.update(pgd_filter=h.numpy(), pgd_y=y.numpy(), pgd_rec=rec.numpy())
print("PGD + PnP(TGV)", float(rec.sum()))

np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tgv.npz"), **out)
