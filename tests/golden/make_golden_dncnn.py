#!/usr/bin/env python
"""Golden vectors for DnCNN from the REAL reference (deepinv v0.4.1, oracle/ref_shim.py), float32 on the CPU:
deepinv.models.DnCNN (deepinv/models/dncnn.py) in colour at depth 20 / nf 64 on an even and an odd shape, grey, without bias,
with nf = 48 (the direct-kernel fallback) and nf = 8 / depth 3, with two channels; a 5-iteration PGD + PnP(DnCNN) on BlurFFT;
and one unfolded_builder("PGD") training step on MultiCoilMRI with PnP(DnCNN(2, 2, depth=7)) and trainable stepsize / g_param
(loss, gradients of every parameter and of the input; gradients larger than 4096 elements as a stride-7 sample plus their norm).
No weights are stored: the depth-20 colour weights come from a seed (tests/dncnn_weights.py: c20_state) and every other net is
cut out of them (derive).

    python tests/golden/make_golden_dncnn.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dncnn_weights import c20_state, derive, grad_sample  # noqa: E402
from oracle.ref_shim import import_reference  # noqa: E402

dinv = import_reference()
from deepinv.models.dncnn import DnCNN  # noqa: E402

g = torch.Generator().manual_seed(2025)
out = {}


c20 = DnCNN(pretrained=None, device="cpu")
SD = c20_state()
c20.load_state_dict(SD, strict=True)
c20.eval()


def net(C=3, depth=20, nf=64, bias=True):
    den = DnCNN(C, C, depth=depth, bias=bias, nf=nf, pretrained=None, device="cpu")
    den.load_state_dict(derive(SD, C, depth, nf, bias), strict=True)
    return den.eval()


def case(tag, den, shape):
    x = torch.rand(*shape, generator=g)
    with torch.no_grad():
        y = den(x)
    out[f"{tag}_x"], out[f"{tag}_y"] = x.numpy(), y.numpy()
    print(tag, shape, float(y.abs().mean()))


case("c20_even", c20, (2, 3, 64, 64))
case("c20_odd", c20, (1, 3, 37, 53))
case("gray", net(1, depth=5), (2, 1, 48, 40))
case("nobias", net(3, depth=5, bias=False), (2, 3, 32, 36))
case("nf48", net(3, depth=5, nf=48), (2, 3, 32, 32))
case("nf8", net(3, depth=3, nf=8), (2, 3, 24, 20))
case("ch2", net(2, depth=7), (2, 2, 40, 44))

# PGD + PnP(DnCNN) on BlurFFT, 5 iterations
pden = net(3, depth=6)
x = torch.rand(1, 3, 48, 48, generator=g)
h = dinv.physics.functional.blur.gaussian_blur(sigma=(1.5, 1.5))
p = dinv.physics.BlurFFT(img_size=(3, 48, 48), filter=h)
y = p.A(x) + 0.02 * torch.randn(1, 3, 48, 48, generator=g)
model = dinv.optim.PGD(prior=dinv.optim.PnP(pden), data_fidelity=dinv.optim.L2(), stepsize=1.0, g_param=0.05, max_iter=5,
                       early_stop=False)
with torch.no_grad():
    rec = model(y, p)
out.update(pgd_filter=h.numpy(), pgd_y=y.numpy(), pgd_rec=rec.numpy())
print("PGD", float(rec.sum()))

# unfolded PGD step on 2-D multi-coil MRI with a trainable DnCNN(2, 2, depth=7)
H = W = 32
coils = 4
xm = torch.rand(1, 2, H, W, generator=g)
maps = torch.randn(1, coils, H, W, dtype=torch.complex64, generator=g) / coils ** 0.5
mask = (torch.rand(H, W, generator=g) < 0.4).float()
mask[:, 12:20] = 1.0
pm = dinv.physics.MultiCoilMRI(mask=mask, coil_maps=maps, img_size=(2, H, W), device="cpu")
ym = pm.A(xm)
uden = net(2, depth=7).train()
model = dinv.unfolded.unfolded_builder("PGD", data_fidelity=dinv.optim.L2(), prior=dinv.optim.PnP(uden),
                                       params_algo={"stepsize": 0.8, "g_param": 0.05, "lambda": 1.0}, max_iter=3,
                                       trainable_params=["stepsize", "g_param"])
ym = ym.clone().requires_grad_()
recm = model(ym, pm)
loss = (recm - xm).pow(2).mean()
loss.backward()
out.update(unf_x=xm.numpy(), unf_maps=torch.view_as_real(maps).numpy(), unf_mask=mask.numpy(), unf_y=ym.detach().numpy(),
           unf_rec=recm.detach().numpy(), unf_loss=np.float64(loss.item()), unf_grad_y=ym.grad.numpy())
for n, q in model.named_parameters():      # (g_param gets none: DnCNN ignores the noise level)
    if q.grad is not None:
        out["unf_grad_" + n.replace(".", "_")] = grad_sample(q.grad).numpy()
        out["unf_gnorm_" + n.replace(".", "_")] = np.float64(q.grad.double().norm())
print("unfolded loss", float(loss), sorted(n for n, _ in model.named_parameters())[:3])

np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "dncnn.npz"), **out)
