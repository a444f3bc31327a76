#!/usr/bin/env python
"""Time DnCNN (deepinv_amd.models.DnCNN: depth 20, nf 64, bias) against the same network as plain torch.nn in fp32 on
PyTorch-ROCm (MIOpen convolutions, TF32 off), with the same weights on the same GPU.  One JSON line per case, printed and
appended to --out:

    python scripts/bench_dncnn.py [--reps 10] [--out profiles/dncnn_bench.jsonl] [--skip-torch]

cases: inference at [32,2,320,320] (the cfg2 shape with DnCNN in DRUNet's place) and [32,3,256,256]; one training step
(forward + backward of every weight and bias) at [8,2,320,320].
flop_algorithmic: 2 * 9 * Cin * Cout per output pixel and layer (x3 for a training step: forward, data and weight gradients).
flop_executed: what the kernels issue - the direct kernels on the padded frame with zero-padded channels (head cin 8, couts in
32 / 64 tiles), the F(4x4,3x3) body at 36 multiplies per 4x4 tile instead of 144, the vector-ALU tail as algorithmic.
pct_fp32_mfma_peak: flop_algorithmic / time against the 157.3 TFLOP/s fp32 matrix peak (and the executed share)."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepinv_amd as dinv  # noqa: E402
from deepinv_amd.hip import drunet as K  # noqa: E402

PEAK = 157.3e12


class TorchDnCNN(nn.Module):
    """deepinv/models/dncnn.py forward as plain torch.nn (same state_dict keys)"""

    def __init__(self, C, depth, nf):
        super().__init__()
        self.in_conv = nn.Conv2d(C, nf, 3, 1, 1)
        self.conv_list = nn.ModuleList([nn.Conv2d(nf, nf, 3, 1, 1) for _ in range(depth - 2)])
        self.out_conv = nn.Conv2d(nf, C, 3, 1, 1)

    def forward(self, x):
        x1 = torch.relu(self.in_conv(x))
        for c in self.conv_list:
            x1 = torch.relu(c(x1))
        return self.out_conv(x1) + x


def flops(B, C, H, W, depth, nf, train):
    alg = 2.0 * 9 * B * H * W * (2 * C * nf + (depth - 2) * nf * nf)
    g = K.geom(B, H, W)
    head = 2.0 * 9 * 8 * 64 * g.np
    body = (2.0 * 36 * nf * nf * B * (H // 4) * (W // 4) if (H % 4 == 0 and W % 4 == 0 and nf % 64 == 0)
            else 2.0 * 9 * nf * nf * g.np)
    tail = 2.0 * 9 * nf * C * B * H * W
    if not train:
        return alg, head + (depth - 2) * body + tail
    # training: every layer forward on the direct kernel, its data gradient on the direct kernel, its weight gradient
    direct = 2.0 * 9 * g.np * (8 * 64 + (depth - 2) * nf * nf + nf * 32)
    return 3 * alg, 3 * direct


def gpu_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dncnn_bench.jsonl"))
    ap.add_argument("--skip-torch", action="store_true", help="time the HIP kernels only (profiler runs)")
    a = ap.parse_args()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda:0")
    depth, nf = 20, 64
    lines = []
    for kind, (B, C, H, W) in (("inference", (32, 2, 320, 320)), ("inference", (32, 3, 256, 256)), ("train_step", (8, 2, 320, 320))):
        torch.manual_seed(0)
        den = dinv.models.DnCNN(C, C, depth=depth, nf=nf).to(dev)
        ref = TorchDnCNN(C, depth, nf).to(dev)
        ref.load_state_dict(den.state_dict(), strict=True)
        x = torch.rand(B, C, H, W, device=dev)
        train = kind == "train_step"
        if train:
            gy = torch.randn(B, C, H, W, device=dev)

            def ours():
                den.zero_grad(set_to_none=True)
                den(x).backward(gy)

            def theirs_run():
                ref.zero_grad(set_to_none=True)
                ref(x).backward(gy)
        else:
            den.eval()

            def ours():
                with torch.no_grad():
                    den(x)

            def theirs_run():
                with torch.no_grad():
                    ref(x)
        t_hip = gpu_ms(ours, a.reps)
        t_torch = None if a.skip_torch else gpu_ms(theirs_run, a.reps)
        err = None
        if not a.skip_torch and not train:
            with torch.no_grad():
                yo, yr = den(x), ref(x)
            err = float((yo - yr).norm() / yr.norm())
        alg, exe = flops(B, C, H, W, depth, nf, train)
        rec = {"case": kind, "shape": [B, C, H, W], "depth": depth, "nf": nf, "ms_hip": round(t_hip, 3),
               "ms_torch_miopen": None if t_torch is None else round(t_torch, 3),
               "speedup_vs_torch": None if t_torch is None else round(t_torch / t_hip, 3),
               "flop_algorithmic": alg, "flop_executed": exe,
               "pct_fp32_mfma_peak_algorithmic": round(100 * alg / (t_hip * 1e-3) / PEAK, 2),
               "pct_fp32_mfma_peak_executed": round(100 * exe / (t_hip * 1e-3) / PEAK, 2),
               "rel_err_vs_torch": err, "reps": a.reps}
        if t_torch is not None:
            rec["pct_fp32_mfma_peak_torch_algorithmic"] = round(100 * alg / (t_torch * 1e-3) / PEAK, 2)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del den, ref, x
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
