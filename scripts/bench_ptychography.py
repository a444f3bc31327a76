#!/usr/bin/env python
"""Time the ptychography operators (the ptychography kernels of deepinv_amd/csrc/cstructured.hip) against the composed PyTorch
expression of the same computation on the same GPU, written here from the reference's code: the probe product, torch.fft.fft2 /
ifft2 over [B, n_img, H, W] and the sum over positions (deepinv/physics/phase_retrieval.py:376-395), with the pointwise stages as
torch ops (phase_retrieval.py:42-99, optim/distance.py:353-369, optim/phase_retrieval.py:174-179).  One JSON line per (shape,
call), also written to --out:

    python scripts/bench_ptychography.py [--reps 50] [--out profiles/ptychography_bench.jsonl]

Calls: A (|Bx|^2), B, B_adjoint, grad (AmplitudeLoss.grad) and spectral (one power iteration: the weighted normal operation, the
shift and the normalisation).  us_fused / us_torch: HIP-event time per call after three warm-up calls (--reps calls enqueued back
to back between two events, so the host side of a call is included whenever it is longer than the kernels); ratio = us_torch /
us_fused.  `groups` is the number of partial sums per image of the adjoint and the normal operation (1: one launch).

    python scripts/bench_ptychography.py --only-normal [--reps 20]

runs nothing but the normal operation of every shape, for a kernel trace of its own."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepinv_amd as dinv  # noqa: E402
from deepinv_amd.hip import cdense as hcd  # noqa: E402
from deepinv_amd.hip import ptycho as hpt  # noqa: E402
from deepinv_amd.physics.phase_retrieval import generate_shifts  # noqa: E402

SHAPES = (((1, 64, 64), 25, 1), ((1, 64, 64), 25, 32), ((1, 96, 96), 49, 8))     # (img_size, n_img, batch)
LAMB = 10.0


def timed_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-normal", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    lines = []
    al = dinv.optim.AmplitudeLoss()

    def record(rec, fused, ref):
        with torch.no_grad():
            want = ref()
            err = float(torch.linalg.vector_norm(fused() - want) / torch.linalg.vector_norm(want))
            assert err < 1e-4, (rec, err)
            t_f, t_t = timed_us(fused, a.reps), timed_us(ref, a.reps)
        rec.update(us_fused=round(t_f, 2), us_torch=round(t_t, 2), ratio=round(t_t / t_f, 2))
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    for img, n_img, batch in SHAPES:
        p = dinv.physics.Ptychography(img_size=img, shifts=generate_shifts(img, n_img=n_img), device=dev)
        P = p.B.probe

        def B(x):
            return torch.fft.fft2(P * x, norm="ortho")

        def Bt(y):
            return (P * torch.fft.ifft2(y, norm="ortho")).sum(dim=1).unsqueeze(1)      # a real probe: no conjugate to take

        x = torch.randn(batch, *img, dtype=torch.cfloat, generator=g).to(dev)
        yc = torch.randn(batch, n_img, *img[1:], dtype=torch.cfloat, generator=g).to(dev)
        y = p.A(torch.randn(batch, *img, dtype=torch.cfloat, generator=g).to(dev))
        T = dinv.optim.default_preprocessing(y / y.mean(), p)
        Tc = T.to(torch.cfloat)
        rec = {"operator": "Ptychography", "img_size": list(img), "n_img": n_img, "B": batch,
               "groups": hpt.groups(batch, n_img, img[1], img[2], hpt.NORMAL)}
        if a.only_normal:
            with torch.no_grad():
                for _ in range(a.reps):
                    p.B.normal_epilogue(x, hcd.AMPLITUDE, y)
            torch.cuda.synchronize()
            continue

        def spectral_fused():
            v = p.B.normal_epilogue(x, hcd.WEIGHT, T) + LAMB * x
            return v / torch.linalg.norm(v)

        def spectral_torch():
            v = Bt(Tc * B(x)) + LAMB * x
            return v / torch.linalg.norm(v)

        def grad_torch():
            z = B(x)
            return 2 * Bt(z * (1 - torch.sqrt(y / (z.abs().square() + 1e-12))))

        record(dict(rec, op="A"), lambda: p.A(x), lambda: B(x).abs().square())
        record(dict(rec, op="B"), lambda: p.B(x), lambda: B(x))
        record(dict(rec, op="B_adjoint"), lambda: p.B_adjoint(yc), lambda: Bt(yc))
        record(dict(rec, op="grad"), lambda: al.grad(x, y, p), grad_torch)
        record(dict(rec, op="spectral"), spectral_fused, spectral_torch)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
