#!/usr/bin/env python
"""Time the phase-retrieval operators (deepinv_amd/csrc/cdense.hip, cstructured.hip) against the composed PyTorch expression of
the same computation on the same GPU, written here from the reference's code: complex torch.matmul for the dense operator
(deepinv/physics/compressed_sensing.py:126-166), torch.fft.fft2 / ifft2 inside the pad / diagonal / transform / trim composition
of deepinv/physics/structured_random.py:172-202, and the pointwise stages as torch ops (phase_retrieval.py:42-99,
optim/distance.py:353-369, optim/phase_retrieval.py:174-179).  One JSON line per (operator, shape, call), also written to --out:

    python scripts/bench_phase_retrieval.py [--reps 50] [--out profiles/phase_retrieval_bench.jsonl]

Calls: A (|Bx|^2), B, B_adjoint, grad (AmplitudeLoss.grad: two products) and spectral (one power iteration: the weighted
forward, the adjoint, the shift and the normalisation).  us_fused / us_torch: HIP-event time per call after three warm-up calls
(--reps calls enqueued back to back between two events, so the host side of a call is included whenever it is longer than the
kernels); ratio = us_torch / us_fused.  The dense matrices are drawn here and put into the operator: its pseudo-inverse, an SVD
on the host at construction, is neither needed nor timed."""
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

IMG = (1, 64, 64)
DENSE_M = (4096, 8192)
SMALL = ((3, 8, 8), 48)     # K = 192 in 16-k slices at B = 1: the partial launch plus the reduce launch against one small matmul
STRUCT_OUT = ((1, 64, 64), (1, 90, 90))
BATCHES = (1, 32)
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


def torch_dense(p):
    A = p.B._A

    def B(x):
        return torch.matmul(x.reshape(x.shape[0], -1), A.t())

    def Bt(y):
        return torch.matmul(y.to(torch.cfloat), A.conj()).view(y.shape[0], *p.img_size)

    return B, Bt


def torch_structured(p):
    L, half = math.floor(p.n_layers), p.n_layers - math.floor(p.n_layers) == 0.5
    d = p.B.diagonals

    def B(x):
        if p.mode == "oversampling":
            x = padding(x, p.img_size, p.output_size)
        if half:
            x = torch.fft.fft2(x, norm="ortho")
        for i in range(L):
            x = torch.fft.fft2(d[i] * x, norm="ortho")
        return trimming(x, p.img_size, p.output_size) if p.mode == "undersampling" else x

    def Bt(y):
        y = y.to(torch.cfloat)
        if p.mode == "undersampling":
            y = padding(y, p.img_size, p.output_size)
        for i in range(L):
            y = torch.conj(d[-i - 1]) * torch.fft.ifft2(y, norm="ortho")
        if half:
            y = torch.fft.ifft2(y, norm="ortho")
        return trimming(y, p.img_size, p.output_size) if p.mode == "oversampling" else y

    return B, Bt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
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

    def bench(base, p, B, Bt, mshape, img=IMG):
        for batch in BATCHES:
            x = torch.randn(batch, *img, dtype=torch.cfloat, generator=g).to(dev)
            yc = torch.randn(batch, *mshape, dtype=torch.cfloat, generator=g).to(dev)
            y = p.A(torch.randn(batch, *img, dtype=torch.cfloat, generator=g).to(dev))
            T = dinv.optim.default_preprocessing(y / y.mean(), p)
            Tc = T.to(torch.cfloat)
            rec = dict(base, B=batch)

            def spectral_fused():
                v = p.B_adjoint(p.B.apply_epilogue(x, dinv.hip.cdense.WEIGHT, T)) + LAMB * x
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

    for img, m in [(IMG, m) for m in DENSE_M] + [SMALL]:
        n = img[0] * img[1] * img[2]
        p = dinv.physics.RandomPhaseRetrieval(m=8, img_size=img, device=dev)
        p.B._A = (torch.randn((m, n), dtype=torch.cfloat, generator=g) / math.sqrt(m)).to(dev)
        p.B._A_adjoint = p.B._A.conj().T
        bench({"operator": "RandomPhaseRetrieval", "img_size": list(img), "m": m}, p, *torch_dense(p), (m,), img)
        del p
        torch.cuda.empty_cache()
    for osz in STRUCT_OUT:
        p = dinv.physics.StructuredRandomPhaseRetrieval(IMG, osz, 2, device=dev)
        bench({"operator": "StructuredRandomPhaseRetrieval", "img_size": list(IMG), "output_size": list(osz), "n_layers": 2,
               "fused": bool(dinv.hip.cstructured.fits(osz[1], osz[2]))}, p, *torch_structured(p), osz)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
