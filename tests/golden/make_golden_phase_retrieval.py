#!/usr/bin/env python
"""Golden vectors for phase retrieval from the REAL reference (deepinv v0.4.1, oracle/ref_shim.py), complex64 on the CPU
(deepinv/physics/phase_retrieval.py, optim/phase_retrieval.py, AmplitudeLoss of optim/data_fidelity.py).

Next to every output `K` the file holds `K__err`: the reference's own complex64 relative l2 error against the same reference
code run in complex128 on the same (complex64-valued) inputs, diagonals and matrices.  The tests bound the kernels' error
against complex128 by twice this figure and against the stored complex64 output by three times it.  Inputs, diagonals and state
dicts are stored, so no test relies on an rng drawing the same values twice.

    python tests/golden/make_golden_phase_retrieval.py
"""
import math
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_shim import import_reference  # noqa: E402

dinv = import_reference()
from deepinv.optim.data_fidelity import AmplitudeLoss  # noqa: E402
from deepinv.optim.phase_retrieval import spectral_methods  # noqa: E402
from deepinv.physics.phase_retrieval import PhaseRetrieval, RandomPhaseRetrieval, StructuredRandomPhaseRetrieval  # noqa: E402
from deepinv.physics.structured_random import StructuredRandom  # noqa: E402

g = torch.Generator().manual_seed(2028)
out = {}
C64, C128 = torch.complex64, torch.complex128


def rel(a, b):
    a, b = a.to(C128) if a.is_complex() else a.double(), b.to(C128) if b.is_complex() else b.double()
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


def put(key, lo, hi):
    assert lo.dtype in (C64, torch.float32) and hi.dtype in (C128, torch.float64), (key, lo.dtype, hi.dtype)
    out[key] = lo.contiguous().numpy()
    out[key + "__err"] = np.float64(rel(lo, hi))
    print(f"{key:28s} {tuple(lo.shape)}  reference complex64 error {out[key + '__err']:.3e}")


def crandn(*shape):
    return torch.randn(*shape, dtype=C64, generator=g)


def up(t):
    return t.to(C128) if t.is_complex() else t.double()


def operators(tag, p32, p64, x, yc, v, ymeas):
    """every operator of a phase-retrieval physics on stored inputs: x an image, yc a complex measurement-shaped array, v a real
    one (the vector of A_vjp), ymeas positive real measurements (the data of the amplitude loss)"""
    out[f"{tag}_x"], out[f"{tag}_yc"], out[f"{tag}_v"], out[f"{tag}_ymeas"] = x.numpy(), yc.numpy(), v.numpy(), ymeas.numpy()
    put(f"{tag}_A", p32.A(x), p64.A(up(x)))
    put(f"{tag}_B", p32.B(x), p64.B(up(x)))
    put(f"{tag}_Bt", p32.B_adjoint(yc), p64.B_adjoint(up(yc)))
    put(f"{tag}_Bd", p32.B_dagger(yc), p64.B_dagger(up(yc)))
    put(f"{tag}_vjp", p32.A_vjp(x, v), p64.A_vjp(up(x), up(v)))
    al = AmplitudeLoss()
    put(f"{tag}_alfn", al.fn(x, ymeas, p32), al.fn(up(x), up(ymeas), p64))
    put(f"{tag}_algrad", al.grad(x, ymeas, p32), al.grad(up(x), up(ymeas), p64))


# ---------------------------------------------------------------- RandomPhaseRetrieval
def random_double(p32, m, img, cw):
    """the same reference code in complex128 on the same (complex64-valued) matrices"""
    p64 = RandomPhaseRetrieval(m=m, img_size=img, channelwise=cw, dtype=C128)
    p64.B._A, p64.B._A_dagger, p64.B._A_adjoint = p32.B._A.to(C128), p32.B._A_dagger.to(C128), p32.B._A_adjoint.to(C128)
    return p64


def random_case(tag, p32, m, img, cw):
    p64 = random_double(p32, m, img, cw)
    sd = p32.state_dict()
    out[f"{tag}_keys"] = np.array(sorted(sd.keys()))
    for k, v in sd.items():
        out[f"{tag}_sd__{k}"] = v.resolve_conj().contiguous().numpy()
    out[f"{tag}_m"], out[f"{tag}_img"], out[f"{tag}_cw"] = np.int64(m), np.array(img), np.bool_(cw)
    for B in (1, 3):
        x = crandn(B, *img)
        mshape = (B, img[0], m) if cw else (B, m)
        yc, v = crandn(*mshape), torch.randn(mshape, generator=g)
        ymeas = p32.A(crandn(B, *img))
        operators(f"{tag}_b{B}", p32, p64, x, yc, v, ymeas)


# the docstring example (phase_retrieval.py:133-138)
torch.manual_seed(0)
x = torch.randn((1, 1, 3, 3), dtype=torch.cfloat)
physics = RandomPhaseRetrieval(m=6, img_size=(1, 3, 3), rng=torch.Generator("cpu"))
y = physics(x)
want = torch.tensor([[3.8405, 2.2588, 0.0146, 3.0864, 1.8075, 0.1518]])
assert torch.allclose(y, want, atol=1e-4), y
out["doc_x"], out["doc_expected"] = x.numpy(), want.numpy()
put("doc_y", y, random_double(physics, 6, (1, 3, 3), False).A(up(x)))
random_case("doc", physics, 6, (1, 3, 3), False)

RP = [("rp48", 48, (3, 8, 8), False), ("rp20cw", 20, (3, 4, 4), True), ("rp80", 80, (1, 6, 6), False)]
out["rp_tags"] = np.array(["doc"] + [c[0] for c in RP])
for tag, m, img, cw in RP:
    random_case(tag, RandomPhaseRetrieval(m=m, img_size=img, channelwise=cw, rng=torch.Generator().manual_seed(m)), m, img, cw)


# ---------------------------------------------------------------- StructuredRandomPhaseRetrieval
def structured_pair(img, osz, nl, shared=False):
    """(complex64 physics, complex128 physics on the same diagonals, the diagonals [L, C, H, W])"""
    L = math.floor(nl)
    if L == 0:
        # the reference's class stacks an empty list of diagonals and fails: its linear operator is built directly
        work = tuple(max(a, b) for a, b in zip(img, osz))

        def make(dtype):
            B = StructuredRandom(img, osz, n_layers=nl, transform_func=partial(torch.fft.fft2, norm="ortho"),
                                 transform_func_inv=partial(torch.fft.ifft2, norm="ortho"), diagonals=torch.zeros((0, *work), dtype=dtype))
            p = PhaseRetrieval(B)
            p.B_dagger = B.A_adjoint
            return p

        return make(C64), make(C128), torch.zeros((0, *work), dtype=C64)
    p32 = StructuredRandomPhaseRetrieval(img, osz, nl, shared_weights=shared)
    p64 = StructuredRandomPhaseRetrieval(img, osz, nl, shared_weights=shared, dtype=C128)
    assert p32.B.diagonals.dtype == C64
    p64.B.diagonals = p32.B.diagonals.to(C128)
    return p32, p64, p32.B.diagonals.clone()


SP = [("eq0.5", (1, 8, 12), (1, 8, 12), 0.5, False), ("eq1", (1, 8, 12), (1, 8, 12), 1, False),
      ("eq1.5", (1, 8, 12), (1, 8, 12), 1.5, False), ("eq3", (1, 8, 12), (1, 8, 12), 3, False),
      ("under2.5", (2, 8, 12), (2, 5, 7), 2.5, False), ("over1", (1, 8, 12), (1, 11, 15), 1, False),
      ("odd2", (1, 13, 7), (1, 13, 7), 2, False), ("shared2", (1, 8, 12), (1, 8, 12), 2, True),
      ("ch2", (2, 8, 12), (2, 8, 12), 1, False)]
out["sp_tags"] = np.array([c[0] for c in SP])
torch.manual_seed(77)       # the reference draws the phases from the default generator
for tag, img, osz, nl, shared in SP:
    p32, p64, diag = structured_pair(img, osz, nl, shared)
    key = f"sp_{tag}"
    out[f"{key}_img"], out[f"{key}_out"], out[f"{key}_layers"], out[f"{key}_shared"] = np.array(img), np.array(osz), np.float64(nl), np.bool_(shared)
    out[f"{key}_diag"] = diag.numpy()
    if shared:
        assert torch.equal(diag[0], diag[1])
    if tag == "ch2":
        assert not torch.equal(diag[0, 0], diag[0, 1])
    B = 2
    x, yc, v = crandn(B, *img), crandn(B, *osz), torch.randn((B, *osz), generator=g)
    ymeas = p32.A(crandn(B, *img))
    operators(key, p32, p64, x, yc, v, ymeas)
    if tag.startswith("eq") or tag in ("odd2", "shared2", "ch2"):
        out[f"{key}_unitary"] = np.float64(rel(p32.B_adjoint(p32.B(x)), x))
        print(f"{key}_unitary {out[f'{key}_unitary']:.3e}")


# ---------------------------------------------------------------- spectral methods and the loop
def criteria(y, p, x0, n_iter, lamb):
    """the early-stop criterion of spectral_methods at every iteration, with the reference's own operators"""
    from deepinv.optim.phase_retrieval import default_preprocessing
    x = x0
    diag_T = default_preprocessing(y / torch.mean(y), p).to(x)
    c = []
    for _ in range(n_iter):
        x_new = p.B_adjoint(diag_T * p.B(x)) + lamb * x
        x_new = x_new / torch.linalg.norm(x_new)
        c.append(float(torch.linalg.norm(x_new - x) / torch.linalg.norm(x)))
        x = x_new
    return c


def loop(y, p, x0, steps, stepsize):
    """spectral initialisation, then explicit gradient steps on the amplitude loss"""
    al = AmplitudeLoss()
    x = spectral_methods(y, p, x=x0, n_iter=30, early_stop=False)
    for _ in range(steps):
        x = x - stepsize * al.grad(x, y, p)
    return x


N_SPEC, STEPS, STEPSIZE = 30, 20, 0.2
out["spec_iters"], out["loop_steps"], out["loop_stepsize"] = np.int64(N_SPEC), np.int64(STEPS), np.float64(STEPSIZE)
torch.manual_seed(78)
p32 = RandomPhaseRetrieval(m=400, img_size=(1, 8, 8), rng=torch.Generator().manual_seed(400))
cases = [("spec_rand", p32, random_double(p32, 400, (1, 8, 8), False), (1, 8, 8), None)]
out["spec_rand_A"] = p32.B._A.numpy()       # the matrix alone: the loop uses neither the pseudo-inverse nor a second copy
s32, s64, sdiag = structured_pair((1, 16, 16), (1, 23, 23), 2)
out["spec_struct_diag"] = sdiag.numpy()
cases.append(("spec_struct", s32, s64, (1, 16, 16), sdiag))
for tag, q32, q64, img, _ in cases:
    x_true, x0 = crandn(2, *img), crandn(2, *img)
    y = q32.A(x_true)
    out[f"{tag}_y"], out[f"{tag}_x0"] = y.numpy(), x0.numpy()
    put(f"{tag}_x", spectral_methods(y, q32, x=x0, n_iter=N_SPEC, early_stop=False),
        spectral_methods(y.double(), q64, x=up(x0), n_iter=N_SPEC, early_stop=False))
    put(f"{tag}_loop", loop(y, q32, x0, STEPS, STEPSIZE), loop(y.double(), q64, up(x0), STEPS, STEPSIZE))
    if tag != "spec_rand":
        continue
    # early stop: an rtol that the criterion clears by a factor 1.5 on both sides of the stopping iteration, in both precisions
    found = None
    for lamb in (10.0, 3.0, 1.0, 0.3):
        c64, c128 = criteria(y, q32, x0, N_SPEC, lamb), criteria(y.double(), q64, up(x0), N_SPEC, lamb)
        for i in range(1, N_SPEC):
            hi = min(min(c64[:i]), min(c128[:i]))
            lo = max(c64[i], c128[i])
            if hi / lo >= 2.25 * 1.2:
                found = (lamb, i, math.sqrt(hi * lo), c64, c128)
                break
        if found:
            break
    assert found, "no iteration whose criterion drops by the needed factor"
    lamb, stop, rtol, c64, c128 = found
    for c in (c64, c128):
        assert all(v >= 1.5 * rtol for v in c[:stop]) and c[stop] * 1.5 <= rtol, (c[:stop + 1], rtol)
    print(f"early stop: lamb {lamb} stops at iteration {stop} with rtol {rtol:.3e}; criteria {c64[stop - 1]:.3e} -> {c64[stop]:.3e}")
    out["early_lamb"], out["early_rtol"], out["early_stop_iter"] = np.float64(lamb), np.float64(rtol), np.int64(stop)
    e32 = spectral_methods(y, q32, x=x0, n_iter=N_SPEC, lamb=lamb, early_stop=True, rtol=rtol)
    e64 = spectral_methods(y.double(), q64, x=up(x0), n_iter=N_SPEC, lamb=lamb, early_stop=True, rtol=rtol)
    # the stopped run returns the iterate BEFORE the one that met the criterion: it equals the run of `stop` iterations
    assert torch.equal(e32, spectral_methods(y, q32, x=x0, n_iter=stop, lamb=lamb, early_stop=False))
    put("early_x", e32, e64)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "phase_retrieval.npz")
np.savez_compressed(path, **out)
print(os.path.getsize(path), "bytes")
