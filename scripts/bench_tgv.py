#!/usr/bin/env python
"""Time the total-generalized-variation prox (TGVDenoiser, deepinv_amd/csrc/tgv.hip) against a plain PyTorch restatement of
the reference's loop (deepinv/models/tgv.py:148-171: the same tensor expressions and slice loops, with its host sync per
iteration) on the same GPU, and one 30-iteration PGD + PnP(TGVDenoiser) on BlurFFT [32,3,256,256].  One JSON line per shape:

    python scripts/bench_tgv.py [--iters 200] [--torch-iters 20]

us_per_it_*: wall time per inner iteration (crit = 0, so every iteration runs); gbps_fused: the byte model of DESIGN.md 3.9
((5 + 4 nd + 3 nd^2) * 4 bytes per pixel: 100 in 2-D, 176 in 3-D) over the fused time."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepinv_amd as dinv  # noqa: E402

SHAPES = [(32, 3, 256, 256), (8, 1, 512, 512), (1, 3, 64, 64), (2, 12, 16, 256, 256)]


def torch_nabla(x):
    nd = x.ndim - 2
    u = torch.zeros((*x.shape, nd), device=x.device, dtype=x.dtype)
    for i in range(nd):
        a, b = [slice(None)] * x.ndim, [slice(None)] * x.ndim
        a[i + 2], b[i + 2] = slice(None, -1), slice(1, None)
        u[(*a, i)] = x[tuple(b)] - x[tuple(a)]
    return u


def torch_nabla_adjoint(v):
    nd = v.ndim - 3
    u = torch.zeros(v.shape[:-1], device=v.device, dtype=v.dtype)
    for i in range(nd):
        a, b = [slice(None)] * u.ndim, [slice(None)] * u.ndim
        a[i + 2], b[i + 2] = slice(None, -1), slice(1, None)
        gs = [slice(None)] * v.ndim
        gs[-1], gs[i + 2] = i, slice(None, -1)
        u[tuple(a)] -= v[tuple(gs)]
        u[tuple(b)] += v[tuple(gs)]
    return u


def torch_epsilon(v):
    nd = v.ndim - 3
    out = torch.zeros((*v.shape[:-1], nd * nd), device=v.device, dtype=v.dtype)
    for i in range(nd):
        for j in range(nd):
            a, b = [slice(None)] * (v.ndim - 1), [slice(None)] * (v.ndim - 1)
            a[j + 2], b[j + 2] = slice(None, -1), slice(1, None)
            out[(*b, i * nd + j)] = v[(*b, i)] - v[(*a, i)]
    return out


def torch_epsilon_adjoint(u):
    nd = u.ndim - 3
    out = torch.zeros((*u.shape[:-1], nd), device=u.device, dtype=u.dtype)
    for i in range(nd):
        for j in range(nd):
            a, b = [slice(None)] * (u.ndim - 1), [slice(None)] * (u.ndim - 1)
            a[j + 2], b[j + 2] = slice(None, -1), slice(1, None)
            out[(*a, i)] -= u[(*b, i * nd + j)]
            out[(*b, i)] += u[(*b, i * nd + j)]
    return out


def torch_prox(y, lam, n_it, crit=0.0, tau=0.01, rho=1.99):
    nd = y.ndim - 2
    sigma = 1 / tau / (72 * (3 if nd == 3 else 1))
    l1, l2 = lam * 0.1, lam * 0.15
    one = torch.tensor([1.0], device=y.device)
    x2 = y.clone()
    r2 = torch.zeros((*y.shape, nd), device=y.device)
    u2 = torch.zeros((*y.shape, nd * nd), device=y.device)
    for it in range(n_it):
        x_prev = x2.clone()
        t = tau * torch_epsilon_adjoint(u2)
        x = (x2 - torch_nabla_adjoint(t) + tau * y) / (1 + tau)
        s = r2 + t
        r = s - s / torch.maximum(torch.sqrt(torch.sum(s ** 2, axis=-1)) / (tau * l1), one).unsqueeze(-1)
        v = u2 + sigma * torch_epsilon(torch_nabla(2 * x - x2) - (2 * r - r2))
        u = v / torch.maximum(torch.sqrt(torch.sum(v ** 2, axis=-1)) / l2, one).unsqueeze(-1)
        x2 = x2 + rho * (x - x2)
        r2 = r2 + rho * (r - r2)
        u2 = u2 + rho * (u - u2)
        rel = torch.linalg.norm(x_prev.flatten() - x2.flatten()) / (torch.linalg.norm(x2.flatten()) + 1e-12)
        if it > 1 and rel < crit:                     # the reference's host sync
            break
    return x2


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch-iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for shape in SHAPES:
        y = torch.rand(shape, generator=g).to(dev)
        nd = len(shape) - 2
        lam = torch.full((shape[0],) + (1,) * (len(shape) - 1), 0.1, device=dev)          # [B, 1, ..., 1] over the images
        den = dinv.models.TGVDenoiser(n_it_max=a.iters, crit=0.0)
        t_f = timed(lambda: den(y, 0.1)) / a.iters
        assert den.n_iter == a.iters
        t_t = timed(lambda: torch_prox(y, lam, a.torch_iters, crit=-1.0)) / a.torch_iters
        bpp = (5 + 4 * nd + 3 * nd * nd) * 4
        rec = {"shape": list(shape), "us_per_it_fused": round(t_f * 1e6, 2), "us_per_it_torch": round(t_t * 1e6, 2),
               "speedup": round(t_t / t_f, 2), "bytes_per_px": bpp, "gbps_fused": round(y.numel() * bpp / t_f / 1e9, 1),
               "iters": a.iters}
        print(json.dumps(rec), flush=True)
        del y, den
        torch.cuda.empty_cache()
    # 30 outer PGD iterations with PnP(TGVDenoiser(n_it_max=100)) (default crit, warm-restarted across outer iterations) on
    # BlurFFT deblurring
    x = torch.rand(32, 3, 256, 256, generator=g).to(dev)
    h = dinv.physics.functional.gaussian_blur(psf_size=(9, 9), sigma=(2.0, 2.0))
    p = dinv.physics.BlurFFT(img_size=(3, 256, 256), filter=h, device=dev)
    yb = p.A(x)
    den = dinv.models.TGVDenoiser(n_it_max=100)
    m = dinv.optim.PGD(prior=dinv.optim.PnP(den), data_fidelity=dinv.optim.L2(), stepsize=1.0, g_param=0.05, max_iter=30,
                       early_stop=False)
    with torch.no_grad():
        t_pgd = timed(lambda: m(yb, p), reps=1)
    print(json.dumps({"tgv_pgd_blurfft": [32, 3, 256, 256], "outer_iters": 30, "inner_n_it_max": 100, "seconds": round(t_pgd, 4),
                      "last_inner_iters": den.n_iter}), flush=True)


if __name__ == "__main__":
    main()
