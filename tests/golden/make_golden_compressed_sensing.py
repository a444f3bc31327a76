#!/usr/bin/env python
"""Golden vectors for dst1, StructuredRandom and CompressedSensing from the REAL reference (deepinv v0.4.1, oracle/ref_shim.py),
float32 on the CPU (deepinv/physics/compressed_sensing.py, structured_random.py).

Next to every float32 output `K` the file holds `K__err`: the reference's own float32 relative l2 error against a float64 run
of the same reference code on the same (float32-valued) inputs, diagonals and matrices.  The tests bound the kernels' error
against float64 by twice this figure.  Inputs, diagonals and state dicts are stored, so no test relies on an rng drawing the
same values twice.

    python tests/golden/make_golden_compressed_sensing.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_shim import import_reference  # noqa: E402

dinv = import_reference()
from deepinv.physics.compressed_sensing import CompressedSensing, dst1  # noqa: E402
from deepinv.physics.structured_random import StructuredRandom  # noqa: E402

g = torch.Generator().manual_seed(2027)
out = {}


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def put(key, f32, f64):
    assert f32.dtype == torch.float32 and f64.dtype == torch.float64, key
    out[key] = f32.numpy()
    out[key + "__err"] = np.float64(rel(f32, f64))
    print(f"{key:28s} {tuple(f32.shape)}  reference fp32 error {out[key + '__err']:.3e}")


# ---- dst1 on [3, n]
DST_N = (1, 2, 3, 12, 31, 32, 64, 127)
out["dst_n"] = np.array(DST_N)
for n in DST_N:
    x = torch.randn(3, n, generator=g)
    out[f"dst{n}_x"] = x.numpy()
    put(f"dst{n}_y", dst1(x), dst1(x.double()))

# ---- StructuredRandom: (tag, img_size, output_size, n_layers, input shape).  Diagonals differ in every channel, row and column:
# +-1 draws for the equisampling cases (the operator is orthogonal there), signed reals in 0.5 .. 1.5 for the others
SR = [("eq0.5", (2, 8, 12), (2, 8, 12), 0.5), ("eq1", (2, 8, 12), (2, 8, 12), 1), ("eq1.5", (2, 8, 12), (2, 8, 12), 1.5),
      ("eq3", (2, 8, 12), (2, 8, 12), 3), ("under2.5", (2, 8, 12), (2, 5, 7), 2.5), ("over1", (2, 8, 12), (2, 11, 15), 1),
      ("line2", (12,), (12,), 2)]
out["sr_tags"] = np.array([c[0] for c in SR])
for tag, img, osz, nl in SR:
    L = int(np.floor(nl))
    work = tuple(max(a, b) for a, b in zip(img, osz))
    sign = torch.where(torch.rand((L, *work), generator=g) > 0.5, -1.0, 1.0)
    diag = sign if tag.startswith("eq") else sign * (0.5 + torch.rand((L, *work), generator=g))
    B = 3 if len(img) == 1 else 2
    x = torch.randn(B, *img, generator=g)
    y = torch.randn(B, *osz, generator=g)
    p32 = StructuredRandom(img, osz, n_layers=nl, diagonals=[d for d in diag] if L else torch.zeros(0, *work))
    p64 = StructuredRandom(img, osz, n_layers=nl, diagonals=[d.double() for d in diag] if L else torch.zeros(0, *work).double())
    out[f"sr_{tag}_img"], out[f"sr_{tag}_out"], out[f"sr_{tag}_layers"] = np.array(img), np.array(osz), np.float64(nl)
    out[f"sr_{tag}_diag"], out[f"sr_{tag}_x"], out[f"sr_{tag}_y"] = diag.numpy(), x.numpy(), y.numpy()
    put(f"sr_{tag}_A", p32.A(x), p64.A(x.double()))
    put(f"sr_{tag}_At", p32.A_adjoint(y), p64.A_adjoint(y.double()))
    if tag.startswith("eq"):
        # orthogonality of the reference itself in float32
        out[f"sr_{tag}_ortho"] = np.float64(rel(p32.A_adjoint(p32.A(x)), x))
        print(f"sr_{tag}_ortho {out[f'sr_{tag}_ortho']:.3e}")

# the loop-level geometry of tests/test_compressed_sensing_gpu.py: only the reference's own error (the test draws its own inputs)
img, osz = (1, 32, 32), (1, 16, 16)
diag = torch.where(torch.rand((1, *img), generator=g) > 0.5, -1.0, 1.0)
x, y = torch.randn(2, *img, generator=g), torch.randn(2, *osz, generator=g)
p32, p64 = StructuredRandom(img, osz, diagonals=[diag[0]]), StructuredRandom(img, osz, diagonals=[diag[0].double()])
out["sr_loop_A__err"] = np.float64(rel(p32.A(x), p64.A(x.double())))
out["sr_loop_At__err"] = np.float64(rel(p32.A_adjoint(y), p64.A_adjoint(y.double())))
print("sr_loop", out["sr_loop_A__err"], out["sr_loop_At__err"])
# n = 1024 in one dimension, two rows, two layers
diag = torch.where(torch.rand((2, 1024), generator=g) > 0.5, -1.0, 1.0)
x = torch.randn(2, 1024, generator=g)
p32 = StructuredRandom((1024,), (1024,), n_layers=2, diagonals=[d for d in diag])
p64 = StructuredRandom((1024,), (1024,), n_layers=2, diagonals=[d.double() for d in diag])
out["sr_n1024_A__err"] = np.float64(rel(p32.A(x), p64.A(x.double())))
out["sr_n1024_At__err"] = np.float64(rel(p32.A_adjoint(x), p64.A_adjoint(x.double())))
print("sr_n1024", out["sr_n1024_A__err"], out["sr_n1024_At__err"])


# ---- CompressedSensing: the state dict of the reference and every operator at B = 1 and 3
def double_copy(p32, m, img, cw):
    """the same reference code in float64 on the same (float32-valued) matrices"""
    p64 = CompressedSensing(m=m, img_size=img, channelwise=cw, dtype=torch.float64)
    p64._A, p64._A_dagger, p64._A_adjoint = p32._A.double(), p32._A_dagger.double(), p32._A_adjoint.double()
    return p64


CS = [("cs48", 48, (3, 8, 8), False), ("cs20cw", 20, (3, 4, 4), True), ("cs80", 80, (1, 6, 6), False)]
out["cs_tags"] = np.array([c[0] for c in CS])
for tag, m, img, cw in CS:
    p32 = CompressedSensing(m=m, img_size=img, channelwise=cw, rng=torch.Generator().manual_seed(m))
    p64 = double_copy(p32, m, img, cw)
    sd = p32.state_dict()
    out[f"{tag}_keys"] = np.array(sorted(sd.keys()))
    for k, v in sd.items():
        out[f"{tag}_sd__{k}"] = v.contiguous().numpy()
    out[f"{tag}_m"], out[f"{tag}_img"], out[f"{tag}_cw"] = np.int64(m), np.array(img), np.bool_(cw)
    for B in (1, 3):
        x = torch.randn(B, *img, generator=g)
        y = torch.randn((B, img[0], m) if cw else (B, m), generator=g)
        out[f"{tag}_b{B}_x"], out[f"{tag}_b{B}_y"] = x.numpy(), y.numpy()
        put(f"{tag}_b{B}_A", p32.A(x), p64.A(x.double()))
        put(f"{tag}_b{B}_At", p32.A_adjoint(y), p64.A_adjoint(y.double()))
        put(f"{tag}_b{B}_Ad", p32.A_dagger(y), p64.A_dagger(y.double()))

# ---- the docstring example (compressed_sensing.py:75-81)
torch.manual_seed(0)
x = torch.randn(1, 1, 3, 3)
physics = CompressedSensing(m=10, img_size=(1, 3, 3), rng=torch.Generator("cpu"))
y = physics(x)
want = torch.tensor([[-1.7769, 0.6160, -0.8181, -0.5282, -1.2197, 0.9332, -0.1668, 1.5779, 0.6752, -1.5684]])
assert torch.allclose(y, want, atol=1e-4), y
out["doc_x"], out["doc_expected"] = x.numpy(), want.numpy()
for k, v in physics.state_dict().items():
    out[f"doc_sd__{k}"] = v.contiguous().numpy()
p64 = double_copy(physics, 10, (1, 3, 3), False)
put("doc_y", y, p64.A(x.double()))
out["doc_keys"] = np.array(sorted(physics.state_dict().keys()))
out["doc_m"], out["doc_img"], out["doc_cw"] = np.int64(10), np.array((1, 3, 3)), np.bool_(False)
for B in (1, 3):
    x = torch.randn(B, 1, 3, 3, generator=g)
    y = torch.randn(B, 10, generator=g)
    out[f"doc_b{B}_x"], out[f"doc_b{B}_y"] = x.numpy(), y.numpy()
    put(f"doc_b{B}_A", physics.A(x), p64.A(x.double()))
    put(f"doc_b{B}_At", physics.A_adjoint(y), p64.A_adjoint(y.double()))
    put(f"doc_b{B}_Ad", physics.A_dagger(y), p64.A_dagger(y.double()))

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "compressed_sensing.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
