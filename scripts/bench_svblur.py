#!/usr/bin/env python
"""Time SpaceVaryingBlur's A and A^T as the fused launch (dinv_pconv2d / dinv_pconv2d_transpose, csrc/blur.hip) against the
composition the package offered before them on the same GPU: sum_k hip.conv._Conv(w_k x, h_k) (A) and sum_k w_k
hip.conv._ConvT(y, h_k) (A^T) with torch multiplies and adds - per k a multiply, a convolution launch and an accumulation.

    python scripts/bench_svblur.py [--windows 5] [--window-ms 300] [--out profiles/svblur.json]

Shapes: x [8, 3, 256, 256], reflect padding, K = 10; 7 x 7 filters (traffic-bound) and 31 x 31 (arithmetic-bound); multipliers
shared over the batch ([1, 3, K, H, W]) and per sample ([8, 3, K, H, W]).  Before any timing the fused and the composed outputs
are compared element by element within the counted bounds of tests/svblur_cases.py (both against each other: the sum of the two
bounds).  Timing: device events; per point the two forms are ALTERNATED window by window in one process, each window long enough
(--window-ms, after a warm-up) that it is a sizeable fraction of a second, and the spread over the windows is reported (min /
median / max).  Reported per point: time, bytes of the (K + 2) H W model over time, multiply-adds over time, and which of the two
bounds the fused kernel (the larger of bytes / 8 TB/s and FMAs / (157.3e12 / 2 per second))."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepinv_amd.hip import conv as hc  # noqa: E402

B, C, H, W, K = 8, 3, 256, 256, 10
MODE = "reflect"
PEAK_BYTES, PEAK_FMA = 8.0e12, 157.3e12 / 2
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


def composed_A(x, w, h):
    out = None
    for k in range(K):
        t = hc._Conv.apply(w[:, :, k] * x, h[:, :, k], MODE, 1)
        out = t if out is None else out + t
    return out


def composed_AT(y, w, h):
    out = None
    for k in range(K):
        t = w[:, :, k] * hc._ConvT.apply(y, h[:, :, k], MODE, 1, (H, W))
        out = t if out is None else out + t
    return out


def window_us(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def reps_for(fn, window_ms):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    one = window_us(fn, 3)
    return max(3, int(window_ms * 1e3 / max(one, 1.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_svblur.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    results = []
    with torch.no_grad():
        for f in (7, 31):
            for mb in (1, B):
                x = torch.randn(B, C, H, W, generator=g).to(dev)
                v = torch.randn(B, C, H, W, generator=g).to(dev)
                w = torch.randn(mb, C, K, H, W, generator=g).to(dev)
                h = (torch.randn(1, C, K, f, f, generator=g) / f).to(dev)
                hk = h.contiguous()
                for op, fused, comp, arg in (("A", hc._pconv_fwd, composed_A, x), ("A_adjoint", hc._pconv_adj, composed_AT, v)):
                    run_f = lambda: fused(arg, w, hk, MODE)            # noqa: E731
                    run_c = lambda: comp(arg, w, hk)                   # noqa: E731
                    # outputs agree within the counted bounds (fused: one chain; composed: per k a chain, a product, K - 1 additions)
                    yf, yc = run_f().double(), run_c().double()
                    wa, ha, aa = w.double().abs(), hk.double().abs(), arg.double().abs()
                    mag = composed_A(aa.float(), wa.float(), ha.float()).double() if op == "A" else \
                        composed_AT(aa.float(), wa.float(), ha.float()).double()
                    n_f, n_c = (K * f * f + 1, f * f + K) if op == "A" else (9 * f * f + K, 9 * f * f + K)
                    worst = float(((yf - yc).abs() / ((gamma(n_f) + gamma(n_c)) * mag * (1 + 1e-3))).max())
                    assert worst <= 1.0, (f, mb, op, worst)
                    rf, rc = reps_for(run_f, a.window_ms), reps_for(run_c, a.window_ms)
                    tf, tc = [], []
                    for _ in range(a.windows):
                        tf.append(window_us(run_f, rf))
                        tc.append(window_us(run_c, rc))
                    words = B * C * H * W * 2 + mb * C * K * H * W                  # x (or y) once, the result once, every multiplier once
                    fmas = B * C * H * W * K * f * f
                    med_f, med_c = statistics.median(tf), statistics.median(tc)
                    t_bytes, t_fma = words * 4 / PEAK_BYTES, fmas / PEAK_FMA
                    rec = {"op": op, "x": [B, C, H, W], "K": K, "filter": [f, f], "multipliers": [mb, C, K, H, W], "padding": MODE,
                           "agreement_worst_over_bound": round(worst, 4),
                           "us_fused": {"min": round(min(tf), 1), "median": round(med_f, 1), "max": round(max(tf), 1), "reps": rf},
                           "us_composed": {"min": round(min(tc), 1), "median": round(med_c, 1), "max": round(max(tc), 1), "reps": rc},
                           "speedup_median": round(med_c / med_f, 2),
                           "clear_of_spread": min(tc) > max(tf),
                           "model_GB_per_s_fused": round(words * 4 / med_f / 1e3, 1),
                           "GFMA_per_s_fused": round(fmas / med_f / 1e3, 1),
                           "bound": "bytes" if t_bytes > t_fma else "arithmetic",
                           "share_of_bound_fused": round(max(t_bytes, t_fma) / (med_f * 1e-6), 4)}
                    print(json.dumps(rec), flush=True)
                    results.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump({"windows": a.windows, "window_ms": a.window_ms, "results": results}, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()
