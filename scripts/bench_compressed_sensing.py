#!/usr/bin/env python
"""Time StructuredRandom (deepinv_amd/csrc/dst.hip) and CompressedSensing (deepinv_amd/csrc/dense.hip) against a stock-PyTorch
expression of the same operator on the same GPU, written here from the reference's code: torch.fft.rfft of the odd extension
for dst1 (deepinv/physics/compressed_sensing.py:9-29) inside the pad / diagonal / transform / trim composition of
deepinv/physics/structured_random.py:172-202, and torch.matmul for the dense operator.  One JSON line per (operator, shape),
also written to --out when given:

    python scripts/bench_compressed_sensing.py [--reps 50] [--out profiles/compressed_sensing_bench.jsonl]

us_fused / us_torch: HIP-event time per call after three warm-up calls (--reps calls enqueued back to back between two events,
so the host side of a call is included whenever it is longer than the kernels); ratio = us_torch / us_fused."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepinv_amd as dinv  # noqa: E402
from deepinv_amd.physics.structured_random import padding, trimming  # noqa: E402

SR_SHAPES = [((1, 32, 32), (1, 32, 32)), ((3, 128, 128), (3, 128, 128)), ((3, 256, 256), (3, 128, 128))]
SR_LAYERS = (1, 2, 2.5)
CS_CASES = [((1, 32, 32), 256), ((1, 32, 32), 1024)]
BATCHES = (1, 32)


def torch_dst1(x):
    n = x.shape[-1]
    v = x.reshape(-1, n)
    z = torch.zeros(v.shape[0], 1, device=x.device)
    v = torch.view_as_real(torch.fft.rfft(torch.cat([z, v, z, -v.flip([1])], dim=1), norm="ortho"))
    return v[:, 1:-1, 1].reshape(x.shape)


def torch_structured(p):
    L, half = math.floor(p.n_layers), p.n_layers - math.floor(p.n_layers) == 0.5

    def A(x):
        if p.mode == "oversampling":
            x = padding(x, p.img_size, p.output_size)
        if half:
            x = torch_dst1(x)
        for i in range(L):
            x = torch_dst1(p.diagonals[i] * x)
        return trimming(x, p.img_size, p.output_size).contiguous() if p.mode == "undersampling" else x

    def At(y):
        if p.mode == "undersampling":
            y = padding(y, p.img_size, p.output_size)
        for i in range(L):
            y = p.diagonals[-i - 1] * torch_dst1(y)
        if half:
            y = torch_dst1(y)
        return trimming(y, p.img_size, p.output_size).contiguous() if p.mode == "oversampling" else y

    return A, At


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
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    lines = []

    def record(rec, fused, ref):
        with torch.no_grad():
            err = float((fused() - ref()).norm() / ref().norm())
            assert err < 1e-5, (rec, err)
            t_f, t_t = timed_us(fused, a.reps), timed_us(ref, a.reps)
        rec.update(us_fused=round(t_f, 2), us_torch=round(t_t, 2), ratio=round(t_t / t_f, 2))
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    for img, osz in SR_SHAPES:
        for nl in SR_LAYERS:
            p = dinv.physics.StructuredRandom(img, osz, n_layers=nl, device=dev, rng=torch.Generator(dev).manual_seed(1))
            A, At = torch_structured(p)
            for B in BATCHES:
                x, y = torch.randn(B, *img, generator=g).to(dev), torch.randn(B, *osz, generator=g).to(dev)
                base = {"operator": "StructuredRandom", "img_size": list(img), "output_size": list(osz), "n_layers": nl, "B": B}
                record(dict(base, op="A"), lambda: p.A(x), lambda: A(x))
                record(dict(base, op="A_adjoint"), lambda: p.A_adjoint(y), lambda: At(y))
    for img, m in CS_CASES:
        p = dinv.physics.CompressedSensing(m=m, img_size=img, device=dev, rng=torch.Generator(dev).manual_seed(1))
        for B in BATCHES:
            x, y = torch.randn(B, *img, generator=g).to(dev), torch.randn(B, m, generator=g).to(dev)
            base = {"operator": "CompressedSensing", "img_size": list(img), "m": m, "B": B}
            record(dict(base, op="A"), lambda: p.A(x), lambda: torch.matmul(x.reshape(B, -1), p._A.t()))
            record(dict(base, op="A_adjoint"), lambda: p.A_adjoint(y), lambda: torch.matmul(y, p._A).view(B, *img))
            record(dict(base, op="A_dagger"), lambda: p.A_dagger(y), lambda: torch.matmul(y, p._A_dagger.t()).view(B, *img))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
