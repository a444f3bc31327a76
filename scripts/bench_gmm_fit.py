#!/usr/bin/env python
"""Time one EM step of GaussianMixtureModel.fit on the fused kernels (csrc/patch_gmm.hpp POSTERIOR epilogue, csrc/gmm_moments.hpp)
against the same step written as the reference's expressions (deepinv/optim/utils.py:373-412) with PyTorch-ROCm operations on the
same GPU: per batch the centred [K, N, d] tensor and its bmm with the inverse covariances, logsumexp, the responsibilities, the
[K, N, d] product of responsibilities and rows, a K-fold tiled copy of the rows and their bmm; then the M-step formulas.  The
composition is the yardstick; its inverses and log-determinants are computed before the clock starts.

    python scripts/bench_gmm_fit.py [--windows 5] [--window-ms 300] [--out profiles/gmm_fit.json]

Shapes: 2^18 rows in batches of 2^16 at (K, d) = (200, 36), (200, 64) and (50, 108); a random mixture at the scale of image patches
(eigenvalues 0.01 logspace(-1, 0), means 0.5 + 0.05 randn), rows drawn from it.  Before any timing the two forms' new weights,
means and covariances are compared and the relative differences reported (the composition sums 2^18 raw fp32 products, so its
covariances carry the cancellation of C / w - mu mu^T; 1e-3 is flagged, not asserted).  Timing: device events around whole
steps (a fused step ends in its download and M-step on the host, a composed one in its M-step on the device), the two forms ALTERNATED window by window in one process, each window --window-ms long after a warm-up,
min / median / max over the windows.  A composed row that cannot allocate its tensors is reported as such.  Also timed alone, on
one batch with the responsibilities at hand: the posterior call (one launch) and the moments call (two launches: moments and
reduce), the latter with its useful FLOP (2 K N (d + 1)(d + 2) / 2) and executed FLOP (2 K N 1024 T (T + 1) / 2 over 2, T tiles of
32 per side of the upper triangle) against the 157.3 TFLOP/s fp32 matrix-core peak: the share of a call, not of a kernel."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepinv_amd as dinv  # noqa: E402
from deepinv_amd.hip import gmm as G  # noqa: E402

PEAK = 157.3e12
ROWS, BATCH = 1 << 18, 1 << 16
SHAPES = ((200, 36), (200, 64), (50, 108))


def random_mixture(K, d, gen):
    Q = torch.linalg.qr(torch.randn(K, d, d, generator=gen, dtype=torch.float64))[0]
    lam = 0.01 * torch.logspace(-1, 0, d, dtype=torch.float64)[None] * (0.5 + torch.rand(K, 1, generator=gen, dtype=torch.float64))
    cov = Q @ torch.diag_embed(lam) @ Q.transpose(1, 2)
    mu = 0.5 + 0.05 * torch.randn(K, d, generator=gen, dtype=torch.float64)
    w = torch.rand(K, generator=gen, dtype=torch.float64) + 0.1
    return w / w.sum(), mu, cov


def draw(mix, n, gen, device):
    """n rows of the mixture on the device, component by component (no [n, d, d] gather)"""
    w, mu, cov = mix
    k = torch.multinomial(w, n, replacement=True, generator=gen).to(device)
    L = torch.linalg.cholesky(cov).float().to(device)
    z = torch.randn(n, mu.shape[1], generator=gen).to(device)
    x = torch.empty_like(z)
    for j in range(w.numel()):
        sel = (k == j).nonzero()[:, 0]
        x[sel] = mu[j].float().to(device) + z[sel] @ L[j].T
    return x


def model_of(mix, device):
    w, mu, cov = mix
    m = dinv.optim.GaussianMixtureModel(w.numel(), mu.shape[1])
    m.set_cov(cov.float())
    m.mu.data = mu.float()
    m.set_weights(w.float())
    return m.to(device)


class Composed:
    """the reference's EM step as PyTorch operations on the device"""

    def __init__(self, m):
        cov = m._cov.detach().cpu().double()
        dev = m._cov.device
        self.K, self.d = m.n_components, m.dimension
        self.inv, self.logdet = torch.linalg.inv(cov).float().to(dev), torch.logdet(cov).float().to(dev)
        self.mu, self.logw = m.mu.detach(), torch.log(m._weights.detach())

    def step(self, batches, reg=1e-5):
        K, d = self.K, self.d
        mass = torch.zeros_like(self.logw)
        first = torch.zeros_like(self.mu)
        second = torch.zeros_like(self.inv)
        objective, n = 0, 0
        for x in batches:
            n += x.shape[0]
            centred = x[None, :, :] - self.mu[:, None, :]
            expo = torch.sum(torch.bmm(centred, self.inv) * centred, 2)
            ll = (-0.5 * self.logdet[:, None] - 0.5 * expo - 0.5 * d * math.log(2 * math.pi)).T + self.logw[None, :]
            lse = torch.logsumexp(ll, -1)
            objective = objective - torch.sum(lse)
            resp = torch.exp(ll - lse[:, None])
            mass += torch.sum(resp, 0)
            weighted = x[None, :, :] * resp.T[:, :, None]
            first += torch.sum(weighted, 1)
            second += torch.bmm(weighted.transpose(1, 2), x[None, :, :].tile(K, 1, 1))
        mass = torch.maximum(mass, torch.tensor(1e-5).to(mass))
        mu = first / mass[:, None]
        cov = second / mass[:, None, None] - torch.matmul(mu[:, :, None], mu[:, None, :])
        cov = cov + reg * torch.eye(d, device=cov.device)[None]
        return mass / n, mu, cov, objective / n


def window_us(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def reps_for(fn, window_ms):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    one = window_us(fn, 2)
    return max(2, int(window_ms * 1e3 / max(one, 1.0)))


def spread(ts):
    return {"min": round(min(ts), 1), "median": round(statistics.median(ts), 1), "max": round(max(ts), 1)}


def rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max())


def moments_flops(K, d, n):
    T = -(-(d + 1) // 32)
    return 2.0 * K * n * (d + 1) * (d + 2) / 2, 2.0 * K * n * 1024 * T * (T + 1) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gmm_fit.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    results = []
    with torch.no_grad():
        for K, d in SHAPES:
            mix = random_mixture(K, d, gen)
            batches = list(draw(mix, ROWS, gen, dev).split(BATCH))
            m = model_of(random_mixture(K, d, gen)[:1] + mix[1:], dev)       # the data's means and covariances, other weights
            fused = lambda: m._EM_step(batches, cov_regularization=1e-5)      # noqa: E731
            wf, muf, covf, objf = fused()
            rec = {"K": K, "d": d, "rows": ROWS, "batch": BATCH, "objective_fused": objf}
            comp = Composed(m)
            composed = lambda: comp.step(batches)                             # noqa: E731
            try:
                wc, muc, covc, objc = composed()
                torch.cuda.synchronize()
                rec["fused_against_composed"] = {"weights": float(f"{rel(wf, wc):.3g}"), "means": float(f"{rel(muf, muc):.3g}"),
                                                 "covariances": float(f"{rel(covf, covc):.3g}"),
                                                 "objective": float(f"{abs(objf - float(objc)):.3g}")}
                rec["agree_within_1e-3"] = max(rel(wf, wc), rel(muf, muc), rel(covf, covc)) < 1e-3
                can = True
            except torch.cuda.OutOfMemoryError as e:
                rec["composed"] = "cannot allocate: " + str(e).split(".")[0]
                can = False
                torch.cuda.empty_cache()
            rf = reps_for(fused, a.window_ms)
            rc = reps_for(composed, a.window_ms) if can else 0
            tf, tc = [], []
            for _ in range(a.windows):
                tf.append(window_us(fused, rf))
                if can:
                    tc.append(window_us(composed, rc))
            rec["us_fused_step"] = {**spread(tf), "reps": rf}
            if can:
                rec["us_composed_step"] = {**spread(tc), "reps": rc}
                rec["speedup_median"] = round(statistics.median(tc) / statistics.median(tf), 2)
                rec["clear_of_spread"] = min(tc) > max(tf) or min(tf) > max(tc)
            # the two calls of a batch alone
            x = batches[0]
            ops = m.operands(False)
            c = m.mu.detach().float().contiguous()
            beta, nll = G.posterior_rows(ops, x)
            acc = G.Moments.zeros(K, d, dev)
            post = lambda: G.posterior_rows(ops, x)                            # noqa: E731
            mom = lambda: G.accumulate_moments(acc, x, beta, c, nll)           # noqa: E731
            rp, rm = reps_for(post, a.window_ms), reps_for(mom, a.window_ms)
            tp, tm = [], []
            for _ in range(a.windows):
                tp.append(window_us(post, rp))
                tm.append(window_us(mom, rm))
            useful, executed = moments_flops(K, d, BATCH)
            med = statistics.median(tm)
            rec["us_posterior_call"] = {**spread(tp), "reps": rp}
            rec["us_moments_call"] = {**spread(tm), "reps": rm}
            rec["posterior_useful_TFLOP_per_s"] = round(2.0 * K * d * d * BATCH / statistics.median(tp) / 1e6, 2)
            rec["moments_useful_TFLOP_per_s"] = round(useful / med / 1e6, 2)
            rec["moments_executed_TFLOP_per_s"] = round(executed / med / 1e6, 2)
            rec["moments_executed_over_useful"] = round(executed / useful, 3)
            rec["moments_call_executed_share_of_mfma_peak"] = round(executed / (med * 1e-6) / PEAK, 4)
            rec["moments_call_useful_share_of_mfma_peak"] = round(useful / (med * 1e-6) / PEAK, 4)
            rec["moments_workspace_MB"] = round(G._l().dinv_gmm_moments_workspace_bytes(BATCH, K, d, 0) / 1e6, 1)
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del batches, comp
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump({"windows": a.windows, "window_ms": a.window_ms, "results": results}, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
