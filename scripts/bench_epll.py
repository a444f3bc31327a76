#!/usr/bin/env python
"""Time the EPLL half-quadratic step and the five-beta EPLLDenoiser on the fused kernels of csrc/patch_gmm.hpp against the
composition the reference runs, written with PyTorch-ROCm operations on the same GPU: the linear patch indices, the centred
[K, N, d] tensor and its bmm with the regularised inverse covariances, the argmax, the [N, d, d] gather of estimation matrices
and their bmm, two index_put_(accumulate=True) passes, the division and the closed-form image solve - image by image, as the
reference loops over a batch.  The composition is the yardstick; its regularised inverses, log-determinants and estimation
matrices are computed before the clock starts (the reference rebuilds them in every step), which only flatters it.

    python scripts/bench_epll.py [--windows 5] [--window-ms 300] [--out profiles/epll.json]

Shapes: [1, 1, 256, 256] and [8, 1, 256, 256] with K = 200, p = 6 (d = 36), and [1, 3, 256, 256] (d = 108); a random mixture at
the scale of images in [0, 1], sigma = 0.1.  Before any timing: on a 40 x 40 crop the fused step is checked against fp64 with the
counted bounds of tests/gmm_cases.py - every patch whose fp64 gap is clear of the score bound must get the fp64 class, and every
pixel of the step's output must lie within E_out of the fp64 result for the classes chosen (the fp64 truth of a whole 256 x 256
image, [N, K, d] doubles, is too large to hold, so the counted bounds are applied to the crop) - and at full size the fused and
the composed step must agree: at most 1 % of the patches classified differently (both are fp32; the composition's scores carry
the error of its inverse covariances) and the images within 1e-4 relative.  Timing: device events; the
two forms are ALTERNATED window by window in one process, each window --window-ms long after a warm-up, and the spread over the
windows is reported (min / median / max).  Reported per row: time, the executed and the useful FLOP of the product T = Wt P over
the step's time against the 157.3 TFLOP/s fp32 matrix-core peak (executed counts the padding: d rounded up to 4 rows per
component and to 2 per k step, the last row tile, patch tiles of 32), and the speed-up over the composition."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deepinv_amd as dinv  # noqa: E402
from deepinv_amd.hip import gmm as G  # noqa: E402

PEAK = 157.3e12
SIGMA = 0.1
BETAS = (1.0, 4.0, 8.0, 16.0, 32.0)


def random_gmm(K, d, gen, device):
    Q = torch.linalg.qr(torch.randn(K, d, d, generator=gen, dtype=torch.float64))[0]
    lam = 0.1 * torch.logspace(-1, 0, d, dtype=torch.float64)[None] * (0.5 + torch.rand(K, 1, generator=gen, dtype=torch.float64))
    m = dinv.optim.GaussianMixtureModel(K, d)
    m.set_cov((Q @ torch.diag_embed(lam) @ Q.transpose(1, 2)).float())
    m.mu.data = (0.5 + 0.3 * torch.randn(K, d, generator=gen)).float()
    m.set_weights(torch.rand(K, generator=gen) + 0.1)
    return m.to(device)


class Composed:
    """the reference's step as PyTorch operations, one image at a time"""

    def __init__(self, m, p, C, H, W, device):
        self.m, self.p, self.d = m, p, m.dimension
        ar = torch.arange
        one = (ar(C)[:, None, None] * H * W + ar(p)[None, :, None] * W + ar(p)[None, None, :]).reshape(-1)
        pos = (ar(H - p + 1)[:, None] * W + ar(W - p + 1)[None, :]).reshape(-1)
        self.idx = (pos[:, None] + one[None, :]).to(device)                       # [N, d] linear indices into one image
        self.logw = torch.log(m._weights)
        self.steps = {}

    def prepare(self, beta):
        """inverse, log-determinant and estimation matrices of Sigma + I / beta (fp64 on the host, outside the clock)"""
        if beta not in self.steps:
            r = float(torch.tensor(1.0 / beta, dtype=torch.float32))
            cov = self.m._cov.detach().cpu().double()
            reg = cov + r * torch.eye(self.d, dtype=torch.float64)
            inv = torch.linalg.inv(reg)
            dev = self.m._cov.device
            self.steps[beta] = (inv.float().to(dev), torch.logdet(reg).float().to(dev), torch.bmm(inv, cov).float().to(dev))
        return self.steps[beta]

    def classify(self, x1, beta):
        inv, logdet, _ = self.prepare(beta)
        patches = x1.reshape(-1)[self.idx]
        cx = patches[None] - self.m.mu[:, None, :]
        expo = (torch.bmm(cx, inv) * cx).sum(2)
        ll = (-0.5 * logdet[:, None] - 0.5 * expo - 0.5 * self.d * math.log(2 * math.pi)).T + self.logw[None]
        return patches, ll.argmax(1)

    def step(self, x, y, beta):
        a = beta * SIGMA ** 2
        est = self.prepare(beta)[2]
        outs = []
        for b in range(x.shape[0]):
            patches, k = self.classify(x[b], beta)
            z = torch.bmm(est[k], patches[:, :, None])[:, :, 0]
            flat, mult = torch.zeros_like(x[b]).reshape(-1), torch.zeros_like(x[b]).reshape(-1)
            mult.index_put_((self.idx.reshape(-1),), torch.ones_like(z).reshape(-1), accumulate=True)
            flat.index_put_((self.idx.reshape(-1),), z.reshape(-1), accumulate=True)
            outs.append(((y[b].reshape(-1) + a * (flat / mult)) / (1 + a)).view_as(x[b]))
        return torch.stack(outs)

    def denoise(self, y):
        x = y
        for c in BETAS:
            x = self.step(x, y, c / SIGMA ** 2)
        return x


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


def crop_check(m, p, C, x, beta):
    """the fused classes and the fused step's output on a 40 x 40 crop against fp64 with the counted bounds of tests/gmm_cases.py;
    returns (the share of patches inside the score bound, the worst output error over its bound)"""
    import gmm_cases as GC

    crop = x[:1, :, :40, :40].contiguous()
    case = GC.Case("image", m.n_components, C=C, p=p, B=1, H=40, W=40, r=(1.0 / beta,))
    ops = [t.float().double() for t in G.eigen_pack(m._cov.cpu(), m.mu.cpu(), m._weights.cpu())]
    r = torch.tensor([1.0 / beta], dtype=torch.float32)
    model = (*ops, r.double())
    tr = GC.truth(case, model, crop.cpu().double())
    E, _ = GC.score_bounds(case, model, tr)
    amb = GC.ambiguous(tr, E)
    k = G.scores_image(m.operands(True), crop, p, r, G.ARGMAX).cpu().long()
    wrong = (~amb) & (k != tr["scores"].argmax(1))
    assert not bool(wrong.any()), f"{int(wrong.sum())} clear patches of the crop are classified wrong"
    # the step's output for those classes, per pixel within the counted bound E_out (which contains E_z and E_x)
    a = torch.tensor([beta * SIGMA ** 2 / (1 + beta * SIGMA ** 2)], dtype=torch.float32)
    cb = torch.tensor([1 / (1 + beta * SIGMA ** 2)], dtype=torch.float32)
    out = G.epll_step(m.operands(True), crop, p, r, a.to(crop.device), cb.to(crop.device), crop).cpu().double()
    _, _, want, Eout = GC.step_truth(case, model, crop.cpu().double(), k, a.double(), cb.double(), crop.cpu().double())
    worst = float(((out - want).abs() / Eout).max())
    assert worst <= 1.0, f"a pixel of the crop's step is {worst:.3g} times its bound"
    return float(amb.double().mean()), worst


def flops(K, d, B, H, W, p):
    PH, PW = H - p + 1, W - p + 1
    useful = 2.0 * K * d * d * B * PH * PW
    tiles = -(-K * G.padded_dim(d) // 32)
    executed = 2.0 * tiles * 32 * ((d + 1) // 2 * 2) * 32 * (-(-PW // 32)) * PH * B
    return useful, executed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epll.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    K, p = 200, 6
    results = []
    with torch.no_grad():
        for B, C in ((1, 1), (8, 1), (1, 3)):
            H = W = 256
            d = C * p * p
            m = random_gmm(K, d, gen, dev)
            den = dinv.models.EPLLDenoiser(GMM=m, patch_size=p, channels=C, device=dev).to(dev)
            comp = Composed(m, p, C, H, W, dev)
            y = (torch.rand(B, C, H, W, generator=gen) + SIGMA * torch.randn(B, C, H, W, generator=gen)).to(dev)
            beta = 4.0 / SIGMA ** 2
            ambiguous, crop_worst = crop_check(m, p, C, y, beta)
            fused_step = lambda: den(y, SIGMA, betas=[beta])                      # noqa: E731
            comp_step = lambda: comp.step(y, y, beta)                             # noqa: E731
            fused_full = lambda: den(y, SIGMA)                                    # noqa: E731
            comp_full = lambda: comp.denoise(y)                                   # noqa: E731
            kf = G.scores_image(m.operands(True), y, p, torch.full((B,), 1.0 / beta), G.ARGMAX).long()
            kc = torch.cat([comp.classify(y[b], beta)[1] for b in range(B)])
            differ = float((kf != kc).double().mean())
            of, oc = fused_step(), comp_step()
            err = float((of.double() - oc.double()).norm() / oc.double().norm())
            assert differ <= 0.01 and err <= 1e-4, (B, C, differ, err)
            useful, executed = flops(K, d, B, H, W, p)
            for what, ff, fc, steps in (("step", fused_step, comp_step, 1), ("denoiser", fused_full, comp_full, len(BETAS))):
                rf, rc = reps_for(ff, a.window_ms), reps_for(fc, a.window_ms)
                tf, tc = [], []
                for _ in range(a.windows):
                    tf.append(window_us(ff, rf))
                    tc.append(window_us(fc, rc))
                med_f, med_c = statistics.median(tf), statistics.median(tc)
                rec = {"what": what, "x": [B, C, H, W], "K": K, "p": p, "d": d,
                       "patches_classified_differently": round(differ, 6), "step_relative_difference": float(f"{err:.3g}"),
                       "crop_ambiguous_share": round(ambiguous, 6), "crop_output_worst_over_bound": round(crop_worst, 4),
                       "us_fused": {"min": round(min(tf), 1), "median": round(med_f, 1), "max": round(max(tf), 1), "reps": rf},
                       "us_composed": {"min": round(min(tc), 1), "median": round(med_c, 1), "max": round(max(tc), 1), "reps": rc},
                       "speedup_median": round(med_c / med_f, 2), "clear_of_spread": min(tc) > max(tf),
                       "useful_TFLOP_per_s": round(steps * useful / med_f / 1e6, 2),
                       "executed_TFLOP_per_s": round(steps * executed / med_f / 1e6, 2),
                       "padding_share": round(1 - useful / executed, 4),
                       "executed_share_of_mfma_peak": round(steps * executed / (med_f * 1e-6) / PEAK, 4)}
                print(json.dumps(rec), flush=True)
                results.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump({"windows": a.windows, "window_ms": a.window_ms, "results": results}, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
