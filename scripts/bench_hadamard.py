#!/usr/bin/env python
"""Time the operators of SinglePixelCamera (deepinv_amd/csrc/hadamard.hip) against a plain PyTorch restatement of the
reference's expressions on the same GPU (deepinv/physics/singlepixel.py:9-43 hadamard_1d / hadamard_2d: log2(n) rounds of
torch.cat over strided slices; deepinv/physics/forward.py:1080-1117, 1212-1234 for the operators).  One JSON line per
(shape, operator), also written to --out when given:

    python scripts/bench_hadamard.py [--reps 50] [--out profiles/hadamard_bench.jsonl] [--skip-torch]

us_fused / us_torch: HIP-event time per call after three warm-up calls (--reps calls enqueued back to back between two events, so
the host side of a call is included whenever it is longer than the kernels); bytes: the algorithmic minimum, one read of every input plane and
one write of the output (the mask is shared by the batch); gbps_fused = bytes / us_fused; ratio = us_torch / us_fused."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepinv_amd as dinv  # noqa: E402

SHAPES = [(32, 1, 64, 64), (32, 3, 128, 128), (8, 1, 512, 512), (4, 1, 1024, 1024)]


def aten_fwht_last_axis(v):
    """The launches the reference issues for one 1-D transform, written from the butterfly: log2(n) rounds, each one strided add,
    one strided subtract and one concatenation over [..., pairs, done] with the finished outputs on the trailing axis, then the
    1 / sqrt(n) division."""
    n = v.shape[-1]
    rounds = n.bit_length() - 1
    assert n == 1 << rounds
    t = v.reshape(*v.shape, 1)
    for _ in range(rounds):
        left, right = t[..., 0::2, :], t[..., 1::2, :]
        t = torch.cat([left + right, left - right], dim=-1)
    return t.reshape(v.shape) / math.sqrt(n)


def torch_h2(x):
    """rows, swap the axes, rows again, swap back: the two transposes stay views, as in the reference"""
    rows_done = aten_fwht_last_axis(x)
    cols_done = aten_fwht_last_axis(rows_done.transpose(-2, -1))
    return cols_done.transpose(-2, -1)


def torch_ops(mask):
    A = lambda x: mask * torch_h2(x)
    At = lambda y: torch_h2(mask * y)
    return {
        "A": lambda x, y: A(x),
        "A_adjoint": lambda x, y: At(y),
        "A_adjoint_A": lambda x, y: torch_h2(mask * mask * torch_h2(x)),
        "prox_l2": lambda x, y: torch_h2(torch_h2(At(y) + 1 / 0.7 * x) / (mask * mask + 1 / 0.7)),
    }


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
    ap.add_argument("--skip-torch", action="store_true", help="time the kernels alone (for a kernel trace of this script)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    lines = []
    for shape in SHAPES:
        B, C, H, W = shape
        p = dinv.physics.SinglePixelCamera(m=H * W // 4, img_size=(C, H, W), device=dev)
        x, y = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
        fused = {"A": lambda x, y: p.A(x), "A_adjoint": lambda x, y: p.A_adjoint(y), "A_adjoint_A": lambda x, y: p.A_adjoint_A(x),
                 "prox_l2": lambda x, y: p.prox_l2(x, y, 0.7)}
        ref = torch_ops(p.mask)
        with torch.no_grad():
            for op in fused:
                err = float((fused[op](x, y) - ref[op](x, y)).norm() / ref[op](x, y).norm())
                assert err < 1e-5, (op, err)
                t_f = timed_us(lambda: fused[op](x, y), a.reps)
                t_t = float("nan") if a.skip_torch else timed_us(lambda: ref[op](x, y), max(a.reps // 5, 3))
                nbytes = x.numel() * 4 * (3 if op == "prox_l2" else 2) + p.mask.numel() * 4
                rec = {"shape": list(shape), "op": op, "us_fused": round(t_f, 2), "us_torch": round(t_t, 2),
                       "bytes": nbytes, "gbps_fused": round(nbytes / t_f / 1e3, 1), "ratio": round(t_t / t_f, 1)}
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
        del x, y, p
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
