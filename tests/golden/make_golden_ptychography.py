#!/usr/bin/env python
"""Golden vectors for ptychography from the REAL reference (deepinv v0.4.1, oracle/ref_shim.py), complex64 on the CPU
(Ptychography / PtychographyLinearOperator of deepinv/physics/phase_retrieval.py:317-539, AmplitudeLoss of optim/data_fidelity.py,
spectral_methods of optim/phase_retrieval.py).

Next to every output `K` the file holds `K__err`: the reference's own complex64 relative l2 error against the same reference code
run in complex128 on the same (complex64-valued) inputs and probe stack.  The tests bound the kernels' error against complex128 by
twice this figure and against the stored complex64 output by three times it.

The adjoint.  The reference's A_adjoint multiplies by the probe, not by its conjugate (phase_retrieval.py:395): the adjoint for
real probes only.  For the complex-probe case every stored output that involves B^H (B_adjoint, A_vjp, AmplitudeLoss.grad, the
spectral iterate) is computed by the reference's own A_adjoint with the `probe` buffer replaced by its conjugate for the duration
of that call: the true adjoint, by reference code.

Size.  The docstring case has 25 planes of 64 x 64 per image, which as complex64 is 0.8 MB per image and output.  For this case
only: the measurement-shaped inputs are stored as factors a[b, l] and u[h, w] whose product (one IEEE multiplication per element,
so the same bits everywhere) is the input, and of each output the file keeps `K` restricted to the planes / images named by
`K__sel`, while `K__err` is over the whole output.

    python tests/golden/make_golden_ptychography.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_shim import import_reference  # noqa: E402

dinv = import_reference()
from deepinv.optim.data_fidelity import AmplitudeLoss  # noqa: E402
from deepinv.optim.phase_retrieval import spectral_methods  # noqa: E402
from deepinv.physics.phase_retrieval import Ptychography, build_probe, generate_shifts  # noqa: E402

g = torch.Generator().manual_seed(2029)
out = {}
C64, C128 = torch.complex64, torch.complex128


def rel(a, b):
    a, b = up(a), up(b)
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


def up(t):
    return t.to(C128) if t.is_complex() else t.double()


def put(key, lo, hi, sel=None):
    """sel = (images, planes): index lists into the first two axes of the output kept in the file (None: all)"""
    assert lo.dtype in (C64, torch.float32) and hi.dtype in (C128, torch.float64), (key, lo.dtype, hi.dtype)
    out[key + "__err"] = np.float64(rel(lo, hi))
    if sel is not None:
        images, planes = sel
        out[key + "__sel_images"], out[key + "__sel_planes"] = np.array(images), np.array(planes)
        lo = lo[images][:, planes]
    out[key] = lo.contiguous().numpy()
    print(f"{key:24s} {tuple(lo.shape)}  reference complex64 error {out[key + '__err']:.3e}")


def crandn(*shape):
    return torch.randn(*shape, dtype=C64, generator=g)


def true_adjoint(p):
    """B_adjoint of p through the reference's A_adjoint on the conjugated probe buffer"""
    B, ref = p.B, p.B.A_adjoint

    def adjoint(y, **kwargs):
        probe = B.probe
        B.probe = probe.conj()
        try:
            return ref(y, **kwargs)
        finally:
            B.probe = probe

    B.A_adjoint = adjoint
    return p


def pair(img, probe, shifts):
    """(complex64 physics, the same reference code in complex128 on the same probe stack)"""
    p32, p64 = Ptychography(img_size=img, probe=probe, shifts=shifts), Ptychography(img_size=img, probe=probe, shifts=shifts)
    p64.B.probe = up(p32.B.probe)
    if p32.B.probe.is_complex():
        true_adjoint(p32), true_adjoint(p64)
    return p32, p64


def describe(tag, p32, img):
    sd = p32.state_dict()
    out[f"{tag}_keys"] = np.array(list(sd.keys()))
    for k, v in sd.items():
        out[f"{tag}_sd__{k}"] = v.numpy()
    out[f"{tag}_img"] = np.array(img)


def measurements(p32, img, B):
    """positive measurements with zeros, also on planes whose probe is zero"""
    y = p32.A(crandn(B, *img)) + 0.1 * torch.rand((B, p32.B.n_img, *img[1:]), generator=g)
    y.view(-1)[::5] = 0.0
    return y


def operators(key, p32, p64, x, yc, v, ymeas, image_sel=None, plane_sel=None):
    put(f"{key}_A", p32.A(x), p64.A(up(x)), plane_sel)
    put(f"{key}_B", p32.B(x), p64.B(up(x)), plane_sel)
    put(f"{key}_Bt", p32.B_adjoint(yc), p64.B_adjoint(up(yc)), image_sel)
    put(f"{key}_vjp", p32.A_vjp(x, v), p64.A_vjp(up(x), up(v)), image_sel)
    al = AmplitudeLoss()
    put(f"{key}_alfn", al.fn(x, ymeas, p32), al.fn(up(x), up(ymeas), p64))
    put(f"{key}_algrad", al.grad(x, ymeas, p32), al.grad(up(x), up(ymeas), p64), image_sel)


# ---------------------------------------------------------------- the docstring example and the defaults
img = (1, 64, 64)
p32, p64 = pair(img, None, None)
torch.manual_seed(0)
x = torch.randn(img, dtype=torch.cfloat)
y = p32(x)
assert y.shape == torch.Size([1, 25, 64, 64]) and p32.B.probe.dtype == torch.float32
describe("doc", p32, img)
for B, images, planes in ((1, [0], [12]), (3, [1], [7])):
    key = f"doc_b{B}"
    x = crandn(B, *img)
    fa, fu = crandn(B, 25, 1, 1), crandn(1, 1, 64, 64)
    va, vu = torch.randn((B, 25, 1, 1), generator=g), torch.randn((1, 1, 64, 64), generator=g)
    ya, yu = torch.rand((B, 25, 1, 1), generator=g) + 0.5, torch.rand((1, 1, 64, 64), generator=g)
    yu.view(-1)[::5] = 0.0
    for name, a, u in (("yc", fa, fu), ("v", va, vu), ("ymeas", ya, yu)):
        out[f"{key}_{name}__a"], out[f"{key}_{name}__u"] = a.numpy(), u.numpy()
    out[f"{key}_x"] = x.numpy()
    operators(key, p32, p64, x, fa * fu, va * vu, ya * yu, (images, [0]), (images, planes))

# ---------------------------------------------------------------- the small cases
CASES = [("p16", (1, 16, 16), 4, 5), ("p12x20", (1, 12, 20), 9, 4), ("p33x22", (1, 33, 22), 4, 6)]
C16_SHIFTS = torch.tensor([[0, 0], [3, -2], [-5, 4], [16, 0], [0, -7], [8, 8], [-3, -3], [2, 11], [-12, 1]], dtype=torch.int32)
out["tags"] = np.array([c[0] for c in CASES] + ["c16"])
physics = {}
for tag, img, n_img, radius in CASES:
    physics[tag] = (img, *pair(img, build_probe(img, type="disk", probe_radius=radius), generate_shifts(img, n_img=n_img)))
physics["c16"] = ((1, 16, 16), *pair((1, 16, 16), crandn(1, 16, 16), C16_SHIFTS))
for tag, (img, p32, p64) in physics.items():
    describe(tag, p32, img)
    L, B = p32.B.n_img, 2
    zero = [l for l in range(L) if not bool(p32.B.probe[0, l].abs().sum() > 0)]
    out[f"{tag}_zero_planes"] = np.array(zero, dtype=np.int64)
    print(tag, "probe", p32.B.probe.dtype, "planes whose probe is zero:", zero)
    x, yc, v = crandn(B, *img), crandn(B, L, *img[1:]), torch.randn((B, L, *img[1:]), generator=g)
    ymeas = measurements(p32, img, B)
    out[f"{tag}_x"], out[f"{tag}_yc"], out[f"{tag}_v"], out[f"{tag}_ymeas"] = x.numpy(), yc.numpy(), v.numpy(), ymeas.numpy()
    operators(tag, p32, p64, x, yc, v, ymeas)
assert list(out["p12x20_zero_planes"]) == [0, 2, 3, 5, 6, 8] and list(out["c16_zero_planes"]) == [3]

# ---------------------------------------------------------------- spectral iterations on the complex probe
N_SPEC = 10
out["spec_iters"] = np.int64(N_SPEC)
img, p32, p64 = physics["c16"]
x_true, x0 = crandn(2, *img), crandn(2, *img)
y = p32.A(x_true)
out["c16_spec_y"], out["c16_spec_x0"] = y.numpy(), x0.numpy()
put("c16_spec_x", spectral_methods(y, p32, x=x0, n_iter=N_SPEC, early_stop=False),
    spectral_methods(y.double(), p64, x=up(x0), n_iter=N_SPEC, early_stop=False))

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ptychography.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 1024 * 1024
