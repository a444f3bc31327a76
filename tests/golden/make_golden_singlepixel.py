#!/usr/bin/env python
"""Golden vectors for SinglePixelCamera from the REAL reference (deepinv v0.4.1, oracle/ref_shim.py), float32 on the CPU
(deepinv/physics/singlepixel.py): the masks of the four orderings, every operator of the camera on seeded inputs, hadamard_1d /
hadamard_2d, the docstring example, a state dict, and a short HQS + TVPrior reconstruction.

Next to every float32 output `K` the file holds `K__err`: the reference's own float32 relative l2 error against a float64 run
of the same reference code on the same (float32-valued) inputs.  The GPU tests bound the kernels' error against float64
(recomputed by the test with dense Sylvester matrices, which keeps the file small) by twice this figure.

    python tests/golden/make_golden_singlepixel.py
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
from deepinv.physics.singlepixel import SinglePixelCamera, hadamard_1d, hadamard_2d  # noqa: E402

g = torch.Generator().manual_seed(2026)
out = {}
ORDERINGS = ("sequency", "cake_cutting", "zig_zag", "xy")


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm()) if float(b.double().norm()) > 0 else float(a.double().norm())


def put(key, f32, f64):
    out[key] = f32.numpy()
    out[key + "__err"] = np.float64(rel(f32, f64))
    print(f"{key:32s} {tuple(f32.shape)}  reference fp32 error {out[key + '__err']:.3e}")


# ---- masks: the four orderings at three sizes (uint8: they are binary), and the two ends of m for sequency
for img in ((1, 32, 32), (3, 64, 128), (1, 16, 16)):
    n = img[1] * img[2]
    tag = "x".join(map(str, img))
    for o in ORDERINGS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mask = SinglePixelCamera(m=n // 5, img_size=img, ordering=o).mask
        assert set(mask.unique().tolist()) <= {0.0, 1.0} and tuple(mask.shape) == (1, *img)
        out[f"mask_{tag}_{o}"] = mask.numpy().astype(np.uint8)
    for m in (1, 16, n):
        out[f"mask_{tag}_sequency_m{m}"] = SinglePixelCamera(m=m, img_size=img).mask.numpy().astype(np.uint8)


# ---- every operator on seeded inputs.  `sparse_y`: measurements supported on the mask, which keeps the large case small on disk
def operator_case(tag, img, m, ordering, B, ops, sparse_y=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p32 = SinglePixelCamera(m=m, img_size=img, ordering=ordering)
        p64 = SinglePixelCamera(m=m, img_size=img, ordering=ordering, dtype=torch.float64)
    x = torch.randn(B, *img, generator=g)
    y = torch.randn(B, *img, generator=g)
    if sparse_y:
        y = y * p32.mask
    out[f"{tag}_x"], out[f"{tag}_y"] = x.numpy(), y.numpy()
    out[f"{tag}_m"], out[f"{tag}_ordering"] = np.int64(m), np.array(ordering)
    table = {
        "A": lambda p, x, y: p.A(x),
        "A_adjoint": lambda p, x, y: p.A_adjoint(y),
        "A_adjoint_A": lambda p, x, y: p.A_adjoint_A(x),
        "A_A_adjoint": lambda p, x, y: p.A_A_adjoint(y),
        "prox_l2_g0.7": lambda p, x, y: p.prox_l2(x, y, 0.7),
        "prox_l2_g0.001": lambda p, x, y: p.prox_l2(x, y, 1e-3),
        "A_dagger": lambda p, x, y: p.A_dagger(y),
        "hadamard_1d": lambda p, x, y: hadamard_1d(x),
        "hadamard_1d_raw": lambda p, x, y: hadamard_1d(x, normalize=False),
        "hadamard_2d": lambda p, x, y: hadamard_2d(x),
    }
    for name in ops:
        put(f"{tag}_{name}", table[name](p32, x, y), table[name](p64, x.double(), y.double()))


ALL = ("A", "A_adjoint", "A_adjoint_A", "A_A_adjoint", "prox_l2_g0.7", "prox_l2_g0.001", "A_dagger", "hadamard_1d",
       "hadamard_1d_raw", "hadamard_2d")
operator_case("op32", (1, 32, 32), 16, "sequency", 2, ALL)
operator_case("op16_full", (1, 16, 16), 256, "sequency", 3, ALL)
operator_case("op16_one", (1, 16, 16), 1, "sequency", 2, ALL)
operator_case("op16_zigzag", (1, 16, 16), 40, "zig_zag", 2, ALL)
operator_case("op16_xy", (1, 16, 16), 40, "xy", 2, ALL)
operator_case("op16_cake", (1, 16, 16), 40, "cake_cutting", 2, ALL)
# the large rectangular multi-channel case: every operator of the camera.  Its three mask-independent transforms are left out
# for the size of the file alone (98 KB each); the (3, 16, 32) case below has them on a rectangular multi-channel input
operator_case("op64x128", (3, 64, 128), 900, "sequency", 1, ALL[:7], sparse_y=True)
operator_case("op16x32", (3, 16, 32), 100, "sequency", 1, ALL)


# ---- full-size shapes: only the reference's own error is stored; tests/test_singlepixel_gpu.py regenerates the inputs from the
# same seeds (full_size_inputs there is this function) and computes float64 itself
def full_size_inputs(shape):
    gen = torch.Generator().manual_seed(shape[-1] + shape[-2])
    x, y = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    mask = torch.rand(shape, generator=gen) * (torch.rand(shape, generator=gen) < 0.5)
    return x, y, mask


def err_case(tag, img, x, y, mask, m=100):
    """the reference's fp32 error against its own fp64 run for every operator, with `mask` passed through update_parameters"""
    p32 = SinglePixelCamera(m=m, img_size=img)
    p64 = SinglePixelCamera(m=m, img_size=img, dtype=torch.float64)
    if mask is not None:
        p32.update_parameters(mask=mask)
        p64.update_parameters(mask=mask.double())
    calls = {
        "A": lambda p, x, y: p.A(x), "A_adjoint": lambda p, x, y: p.A_adjoint(y), "A_adjoint_A": lambda p, x, y: p.A_adjoint_A(x),
        "A_A_adjoint": lambda p, x, y: p.A_A_adjoint(y), "prox_l2_g0.7": lambda p, x, y: p.prox_l2(x, y, 0.7),
        "prox_l2_g0.001": lambda p, x, y: p.prox_l2(x, y, 1e-3), "A_dagger": lambda p, x, y: p.A_dagger(y),
        "hadamard_1d": lambda p, x, y: hadamard_1d(x), "hadamard_1d_raw": lambda p, x, y: hadamard_1d(x, normalize=False),
        "hadamard_2d": lambda p, x, y: hadamard_2d(x), "pinv": lambda p, x, y: p.A_dagger(p.A(x)),
    }
    for name, fn in calls.items():
        out[f"{tag}_{name}__err"] = np.float64(rel(fn(p32, x, y), fn(p64, x.double(), y.double())))
        print(f"{tag:18s} {name:16s} reference fp32 error {out[f'{tag}_{name}__err']:.3e}")


for shape in ((2, 3, 128, 128), (2, 1, 512, 512), (1, 1, 1024, 1024), (2, 1, 128, 1024), (1, 2, 1024, 128)):
    err_case("fs_" + "x".join(map(str, shape)), shape[1:], *full_size_inputs(shape))

# a per-call [B, C, H, W] mask at a small size, and the full binary mask (m = H W: A_dagger(A(x)) = x) at two sizes
gen = torch.Generator().manual_seed(9)
px, pm = torch.randn(3, 1, 16, 16, generator=gen), torch.rand(3, 1, 16, 16, generator=gen)
err_case("percall", (1, 16, 16), px, SinglePixelCamera(m=30, img_size=(1, 16, 16)).A(px, mask=pm), pm, m=30)
for img in ((2, 16, 32), (1, 256, 128)):
    fx = torch.randn(2, *img, generator=torch.Generator().manual_seed(5))
    err_case("full_" + "x".join(map(str, img)), img, fx, fx, None, m=img[1] * img[2])

# ---- the docstring example (singlepixel.py:326-337)
torch.manual_seed(0)
x = torch.randn((1, 1, 32, 32))
physics = SinglePixelCamera(m=16, img_size=(1, 32, 32), fast=True)
out["doc_x"] = x.numpy()
out["doc_mask_sum"] = np.float64(torch.sum(physics.mask).item())
out["doc_y_corner"] = torch.round(physics(x)[:, :, :3, :3]).abs().numpy()
assert out["doc_mask_sum"] == 16.0 and out["doc_y_corner"].tolist() == [[[[1., 0., 1.], [0., 0., 0.], [0., 0., 0.]]]]

# ---- a state dict written by the reference
sd = SinglePixelCamera(m=100, img_size=(2, 16, 32), ordering="zig_zag").state_dict()
out["sd_keys"] = np.array(sorted(sd.keys()))
for k, v in sd.items():
    out[f"sd__{k}"] = v.numpy()
print("state dict keys", sorted(sd.keys()))

# ---- HQS + TVPrior on a 64 x 64 sequency camera with Gaussian noise (HQS goes through prox_l2)
from deepinv.optim.prior import TVPrior  # noqa: E402

xx, yy = torch.meshgrid(torch.linspace(-1, 1, 64), torch.linspace(-1, 1, 64), indexing="ij")
img = ((xx ** 2 + yy ** 2 < 0.5).float() * 0.6 + ((xx.abs() < 0.3) & (yy.abs() < 0.6)).float() * 0.4).view(1, 1, 64, 64)
p = SinglePixelCamera(m=1200, img_size=(1, 64, 64))
y = p.A(img) + 0.02 * torch.randn(1, 1, 64, 64, generator=g) * p.mask
model = dinv.optim.HQS(prior=TVPrior(n_it_max=40), data_fidelity=dinv.optim.L2(), stepsize=1.0, lambda_reg=0.05, max_iter=6,
                       early_stop=False)
with torch.no_grad():
    rec = model(y, p)
out.update(hqs_y=y.numpy(), hqs_rec=rec.numpy(), hqs_m=np.int64(1200))
print("HQS + TVPrior", float(rec.sum()), "psnr-ish", float(((rec - img) ** 2).mean()))

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "singlepixel.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
