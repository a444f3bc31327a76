#!/usr/bin/env python
"""Time the Poisson-family noise kernel (deepinv_amd/csrc/random.hip: dinv_poisson_noise) and the pointwise likelihood kernel
(deepinv_amd/csrc/elementwise.hip: dinv_fidelity_pointwise) against the reference's torch expressions on the same GPU and inputs
(deepinv/physics/noise.py:473-505, 608-650, 752-769: torch.poisson and the elementwise ops around it; deepinv/optim/distance.py:235-263).
One JSON line per (shape, mode, rate), also written to --out when given:

    python scripts/bench_poisson.py [--reps 50] [--out profiles/poisson_bench.jsonl] [--skip-torch]

us_fused / us_torch: HIP-event time per call after three warm-up calls (--reps calls enqueued back to back between two events);
bytes: the algorithmic minimum, one read of x and one write of y (8 bytes per element; 12 for the likelihood kernel, which also
reads y); gbps_fused = bytes / us_fused; floor_fraction = gbps_fused / --peak-gbps (HBM peak); ratio = us_torch / us_fused.
The noise classes run with clip_positive=True on both sides: no flag, no host synchronisation (the reference's torch.any is not timed)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepinv_amd as dinv  # noqa: E402

SHAPES = [(8, 1, 725, 720), (32, 3, 256, 256), (32, 1, 128, 128)]
RATES = [1.0, 30.0, 1e4]
N0, MU = 1e4, 1 / 50.0


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


def torch_poisson(x, gain, rng):
    return torch.poisson(torch.clip(x / gain, min=0.0), generator=rng) * gain


def torch_poisson_gaussian(x, gain, sigma, rng):
    gain = torch.clip(gain, min=1e-12)
    y = torch.poisson(torch.clip(x / gain, min=0.0), generator=rng) * gain
    return y + torch.empty_like(x).normal_(generator=rng) * sigma


def torch_log_poisson(x, n0, mu, rng):
    return -torch.log(torch.poisson(n0 * torch.exp(-x * mu), generator=rng) / n0) / mu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--peak-gbps", type=float, default=8000.0, help="HBM peak of the device (MI355X: 8 TB/s)")
    ap.add_argument("--skip-torch", action="store_true", help="time the kernels alone (for a kernel trace of this script)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = torch.Generator(dev).manual_seed(0)
    lines = []

    def emit(rec, nbytes, t_f, t_t):
        rec.update(us_fused=round(t_f, 2), us_torch=round(t_t, 2), bytes=nbytes, gbps_fused=round(nbytes / t_f / 1e3, 1),
                   floor_fraction=round(nbytes / t_f / 1e3 / a.peak_gbps, 3), ratio=round(t_t / t_f, 2))
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    nan = float("nan")
    with torch.no_grad():
        for shape in SHAPES:
            gain = torch.tensor(0.5, device=dev)
            sigma = torch.tensor(0.1, device=dev)
            n0, mu = torch.tensor(N0, device=dev), torch.tensor(MU, device=dev)
            for lam in RATES:
                x = (0.75 + 0.5 * torch.rand(shape, generator=torch.Generator().manual_seed(1)).to(dev)) * (lam * 0.5)   # x / gain in [0.75, 1.25] lam
                nbytes = x.numel() * 8
                pn = dinv.physics.PoissonNoise(gain=gain, clip_positive=True, rng=rng)
                t_f = timed_us(lambda: pn(x), a.reps)
                t_t = nan if a.skip_torch else timed_us(lambda: torch_poisson(x, gain, rng), a.reps)
                emit({"shape": list(shape), "mode": "poisson", "rate": lam}, nbytes, t_f, t_t)
                pg = dinv.physics.PoissonGaussianNoise(gain=gain, sigma=sigma, clip_positive=True, rng=rng)
                t_f = timed_us(lambda: pg(x), a.reps)
                t_t = nan if a.skip_torch else timed_us(lambda: torch_poisson_gaussian(x, gain, sigma, rng), a.reps)
                emit({"shape": list(shape), "mode": "poisson_gaussian", "rate": lam}, nbytes, t_f, t_t)
                xl = -torch.log(x / 0.5 / N0) / MU               # N0 exp(-mu xl) = x / gain ~ lam
                lp = dinv.physics.LogPoissonNoise(N0=n0, mu=mu, rng=rng)
                t_f = timed_us(lambda: lp(xl), a.reps)
                t_t = nan if a.skip_torch else timed_us(lambda: torch_log_poisson(xl, n0, mu, rng), a.reps)
                emit({"shape": list(shape), "mode": "log_poisson", "rate": lam}, nbytes, t_f, t_t)
                del x, xl
        # the pointwise likelihood kernel: one grad and one prox row
        shape = (32, 3, 256, 256)
        x = torch.rand(shape, device=dev) * 4 + 0.1
        y = torch.poisson(x * 2) / 2
        d = dinv.optim.PoissonLikelihoodDistance(gain=0.5, bkg=0.1, denormalize=True)
        g_, b_ = 0.5, 0.1
        ref_grad = lambda: g_ * (1 - (y / g_) / (x / g_ + b_))
        ref_prox = lambda: (x - (1 / (g_ * 0.7)) * ((x - (1 / (g_ * 0.7))).pow(2) + 4 * (y / g_) / 0.7).sqrt()) / 2
        for name, fused, ref in (("poisson_grad", lambda: d.grad(x, y), ref_grad), ("poisson_prox", lambda: d.prox(x, y, gamma=0.7), ref_prox)):
            err = float((fused() - ref()).norm() / ref().norm())
            assert err < 1e-5, (name, err)
            t_f = timed_us(fused, a.reps)
            t_t = nan if a.skip_torch else timed_us(ref, a.reps)
            emit({"shape": list(shape), "mode": name, "rate": None}, x.numel() * 12, t_f, t_t)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
