"""dst1, StructuredRandom and CompressedSensing on the GPU through the public classes, against float64.

Bound: twice the reference's own fp32 error against its float64 run (``K__err`` of tests/golden/compressed_sensing.npz,
written by tests/golden/make_golden_compressed_sensing.py), the project's rule from the SinglePixelCamera tests.  Diagonals go in
through ``diagonals=`` and matrices through ``load_state_dict``: no test relies on an rng drawing the same values twice."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import dot_test, rel_err

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compressed_sensing.npz"))
SR_TAGS = [str(t) for t in GOLD["sr_tags"]]
CS_TAGS = [str(t) for t in GOLD["cs_tags"]] + ["doc"]       # the docstring example is a full case too


def T(a, dev):
    return torch.from_numpy(np.asarray(a)).to(dev)


def sine(n):
    j = torch.arange(1, n + 1, dtype=torch.float64)
    return -math.sqrt(2.0 / (n + 1)) * torch.sin(math.pi * j[:, None] * j[None, :] / (n + 1))


def sr_case(tag, dev):
    import deepinv_amd as dinv

    img, osz = tuple(int(v) for v in GOLD[f"sr_{tag}_img"]), tuple(int(v) for v in GOLD[f"sr_{tag}_out"])
    nl = float(GOLD[f"sr_{tag}_layers"])
    diag = T(GOLD[f"sr_{tag}_diag"], dev)
    p = dinv.physics.StructuredRandom(img, osz, n_layers=nl, diagonals=[d for d in diag] if len(diag) else None, device=dev)
    return p, T(GOLD[f"sr_{tag}_x"], dev), T(GOLD[f"sr_{tag}_y"], dev)


def sr_fp64(tag, x, adjoint):
    """float64 restatement: pad, the layers as dense sine matrices and diagonals, trim"""
    img, osz = tuple(int(v) for v in GOLD[f"sr_{tag}_img"]), tuple(int(v) for v in GOLD[f"sr_{tag}_out"])
    nl, diag = float(GOLD[f"sr_{tag}_layers"]), torch.from_numpy(GOLD[f"sr_{tag}_diag"]).double()
    L, half = math.floor(nl), nl - math.floor(nl) == 0.5
    x = x.detach().cpu().double()
    if len(img) == 3:
        a, b = (osz[1:], img[1:]) if adjoint else (img[1:], osz[1:])
        work = (max(a[0], b[0]), max(a[1], b[1]))
        top, left = math.ceil((work[0] - a[0]) / 2), math.ceil((work[1] - a[1]) / 2)
        x = torch.nn.functional.pad(x, (left, work[1] - a[1] - left, top, work[0] - a[0] - top))
    S = sine(x.shape[-1])
    if not adjoint:
        x = x @ S if half else x
        for i in range(L):
            x = (diag[i] * x) @ S
    else:
        for i in range(L):
            x = diag[L - 1 - i] * (x @ S)
        x = x @ S if half else x
    if len(img) == 3:
        top, left = math.ceil((work[0] - b[0]) / 2), math.ceil((work[1] - b[1]) / 2)
        x = x[..., top:top + b[0], left:left + b[1]]
    return x


def cs_case(tag, dev):
    import deepinv_amd as dinv

    m, img, cw = int(GOLD[f"{tag}_m"]), tuple(int(v) for v in GOLD[f"{tag}_img"]), bool(GOLD[f"{tag}_cw"])
    p = dinv.physics.CompressedSensing(m=m, img_size=img, channelwise=cw, device=dev, rng=torch.Generator(dev))
    p.load_state_dict({k: torch.from_numpy(GOLD[f"{tag}_sd__{k}"]) for k in p.state_dict()})
    return p


# ---------------------------------------------------------------- golden outputs
@pytest.mark.parametrize("n", [int(n) for n in GOLD["dst_n"]])
def test_dst1_golden(n, dev):
    import deepinv_amd as dinv

    x = T(GOLD[f"dst{n}_x"], dev)
    got = dinv.physics.functional.dst1(x)
    e = rel_err(got, x.cpu().double() @ sine(n))
    print(f"dst1 n={n}: {e:.3e} (reference {float(GOLD[f'dst{n}_y__err']):.3e})")
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert e <= 2 * float(GOLD[f"dst{n}_y__err"])
    # any leading shape
    assert torch.equal(dinv.physics.functional.dst1(x.view(3, 1, 1, n)).view(3, n), got)


@pytest.mark.parametrize("tag", SR_TAGS)
def test_structured_random_golden(tag, dev):
    p, x, y = sr_case(tag, dev)
    for key, inp, adjoint in ((f"sr_{tag}_A", x, False), (f"sr_{tag}_At", y, True)):
        got = p.A_adjoint(inp) if adjoint else p.A(inp)
        assert tuple(got.shape) == tuple(GOLD[key].shape)
        e = rel_err(got, sr_fp64(tag, inp, adjoint))
        print(f"{key}: {e:.3e} (reference {float(GOLD[key + '__err']):.3e})")
        assert e <= 2 * float(GOLD[key + "__err"])
        assert rel_err(got, torch.from_numpy(GOLD[key])) <= 3 * float(GOLD[key + "__err"])      # each side's own error
    d = dot_test(p, x, y)
    print(f"{tag} dot test {d:.2e}")
    assert d <= 1e-5
    if tag.startswith("eq"):
        o = rel_err(p.A_adjoint(p.A(x)), x)
        print(f"{tag} orthogonality {o:.3e} (reference {float(GOLD[f'sr_{tag}_ortho']):.3e})")
        assert o <= 2 * float(GOLD[f"sr_{tag}_ortho"])


@pytest.mark.parametrize("tag", CS_TAGS)
def test_compressed_sensing_golden(tag, dev):
    p = cs_case(tag, dev)
    A64, Ad64 = torch.from_numpy(GOLD[f"{tag}_sd___A"]).double(), torch.from_numpy(GOLD[f"{tag}_sd___A_dagger"]).double()
    for B in (1, 3):
        x, y = T(GOLD[f"{tag}_b{B}_x"], dev), T(GOLD[f"{tag}_b{B}_y"], dev)
        rows = (lambda t: t.cpu().double().reshape(-1, t.shape[-1])) if p.channelwise else (lambda t: t.cpu().double().reshape(B, -1))
        xr = x.cpu().double().reshape(B * x.shape[1], -1) if p.channelwise else x.cpu().double().reshape(B, -1)
        for key, got, want in ((f"{tag}_b{B}_A", p.A(x), xr @ A64.t()), (f"{tag}_b{B}_At", p.A_adjoint(y), rows(y) @ A64),
                               (f"{tag}_b{B}_Ad", p.A_dagger(y), rows(y) @ Ad64.t())):
            assert tuple(got.shape) == tuple(GOLD[key].shape)
            e = rel_err(got.reshape(want.shape), want)
            print(f"{key}: {e:.3e} (reference {float(GOLD[key + '__err']):.3e})")
            assert e <= 2 * float(GOLD[key + "__err"])
        d = dot_test(p, x, y)
        assert d <= 1e-5, d
    assert torch.equal(p.A(x), p.A(x))


def test_docstring_example(dev):
    import deepinv_amd as dinv

    p = dinv.physics.CompressedSensing(m=10, img_size=(1, 3, 3), device=dev, rng=torch.Generator(dev))
    p.load_state_dict({k: torch.from_numpy(GOLD[f"doc_sd__{k}"]) for k in p.state_dict()})
    y = p(T(GOLD["doc_x"], dev))
    assert torch.allclose(y.cpu(), torch.from_numpy(GOLD["doc_expected"]), atol=1e-4)
    want = torch.from_numpy(GOLD["doc_x"]).double().reshape(1, 9) @ torch.from_numpy(GOLD["doc_sd___A"]).double().t()
    assert rel_err(y, want) <= 2 * float(GOLD["doc_y__err"])


# ---------------------------------------------------------------- autograd
def test_autograd_is_the_adjoint_kernel(dev):
    g = torch.Generator().manual_seed(3)
    for tag in ("eq1.5", "under2.5", "over1", "line2"):
        p, x, y = sr_case(tag, dev)
        x = x.clone().requires_grad_()
        (p.A(x) * y).sum().backward()
        assert torch.equal(x.grad, p.A_adjoint(y)), tag
        y = y.clone().requires_grad_()
        (p.A_adjoint(y) * x.detach()).sum().backward()
        assert torch.equal(y.grad, p.A(x.detach())), tag
    for tag in CS_TAGS:
        p = cs_case(tag, dev)
        x, v = T(GOLD[f"{tag}_b3_x"], dev).requires_grad_(), T(GOLD[f"{tag}_b3_y"], dev)
        (p.A(x) * v).sum().backward()
        assert torch.equal(x.grad, p.A_adjoint(v)), tag
        v = v.clone().requires_grad_()
        (p.A_dagger(v) * x.detach()).sum().backward()
        assert v.grad.shape == v.shape and torch.isfinite(v.grad).all()
    import deepinv_amd as dinv

    z = torch.randn(4, 31, generator=g).to(dev).requires_grad_()
    w = torch.randn(4, 31, generator=g).to(dev)
    (dinv.physics.functional.dst1(z) * w).sum().backward()
    assert torch.equal(z.grad, dinv.physics.functional.dst1(w))


# ---------------------------------------------------------------- operators drawn here
def test_default_diagonals(dev):
    import deepinv_amd as dinv

    mk = lambda seed: dinv.physics.StructuredRandom((3, 32, 32), (3, 32, 32), n_layers=2, device=dev,
                                                    rng=torch.Generator(dev).manual_seed(seed))
    p = mk(5)
    d = p.diagonals
    assert d.device.type == "cuda" and tuple(d.shape) == (2, 3, 32, 32) and bool((d.abs() == 1).all())
    assert abs(float(d.mean())) <= 5 / math.sqrt(d.numel())          # +-1 draws: standard error 1 / sqrt(N)
    assert torch.equal(mk(5).diagonals, d) and not torch.equal(mk(6).diagonals, d)


def test_own_pseudo_inverse(dev):
    import deepinv_amd as dinv

    p = dinv.physics.CompressedSensing(m=80, img_size=(1, 6, 6), device=dev, rng=torch.Generator(dev).manual_seed(1))
    assert p._A_adjoint.data_ptr() == p._A.data_ptr()
    x = torch.randn(3, 1, 6, 6, generator=torch.Generator().manual_seed(2)).to(dev)
    A64 = p._A.cpu().double()
    want = (x.cpu().double().reshape(3, 36) @ A64.t()) @ torch.linalg.pinv(A64).t()
    e = rel_err(p.A_dagger(p.A(x)).reshape(3, 36), want)
    print(f"A_dagger(A(x)): {e:.3e} (bound {2 * float(GOLD['cs80_b3_Ad__err']):.3e})")
    assert e <= 2 * float(GOLD["cs80_b3_Ad__err"])


# ---------------------------------------------------------------- the operator in the loops
def test_cg_dagger_and_pgd_tv_loop(dev):
    """StructuredRandom((1, 32, 32) -> (1, 16, 16)) in LinearPhysics.A_dagger (CG) and 5 iterations of PGD + TVPrior, against the
    same loops over a dense float64 matrix of the operator built here (its products rounded to fp32, so the rest of the loop is
    the same code).  Bound: twice the reference's fp32 error of this geometry, times the iteration count."""
    import deepinv_amd as dinv

    g = torch.Generator().manual_seed(11)
    diag = torch.where(torch.rand(1, 1, 32, 32, generator=g) > 0.5, -1.0, 1.0)
    p = dinv.physics.StructuredRandom((1, 32, 32), (1, 16, 16), diagonals=[diag[0].to(dev)], device=dev)
    full = (diag[0].double() * torch.eye(1024, dtype=torch.float64).view(1024, 1, 32, 32)) @ sine(32)
    M = full[..., 8:24, 8:24].reshape(1024, 256).t().contiguous().to(dev)                      # [256, 1024]
    dense = dinv.physics.LinearPhysics(A=lambda x, **kw: (x.double().reshape(x.shape[0], -1) @ M.t()).float().view(-1, 1, 16, 16),
                                       A_adjoint=lambda y, **kw: (y.double().reshape(y.shape[0], -1) @ M).float().view(-1, 1, 32, 32),
                                       img_size=(1, 32, 32), device=dev)
    xx, yy = torch.meshgrid(torch.linspace(-1, 1, 32), torch.linspace(-1, 1, 32), indexing="ij")
    img = ((xx ** 2 + yy ** 2 < 0.5).float() * 0.6 + 0.2).view(1, 1, 32, 32).repeat(2, 1, 1, 1).to(dev)
    y = p.A(img)
    err = 2 * max(float(GOLD["sr_loop_A__err"]), float(GOLD["sr_loop_At__err"]))
    with torch.no_grad():
        a, b = p.A_dagger(y, max_iter=5, tol=0.0), dense.A_dagger(y, max_iter=5, tol=0.0)
        e = rel_err(a, b)
        print(f"CG A_dagger: {e:.3e} (bound {5 * err:.3e})")
        assert e <= 5 * err
        mk = lambda: dinv.optim.PGD(prior=dinv.optim.TVPrior(n_it_max=20), data_fidelity=dinv.optim.L2(), stepsize=1.0,
                                    lambda_reg=0.02, max_iter=5, early_stop=False)
        a, b = mk()(y, p), mk()(y, dense)
        e = rel_err(a, b)
        print(f"PGD + TVPrior: {e:.3e} (bound {5 * err:.3e})")
        assert e <= 5 * err


def test_n1024_and_the_lds_limit(dev):
    import deepinv_amd as dinv
    from deepinv_amd.hip import dst as hd

    g = torch.Generator().manual_seed(7)
    diag = torch.where(torch.rand(2, 1024, generator=g) > 0.5, -1.0, 1.0)
    x = torch.randn(2, 1024, generator=g)
    p = dinv.physics.StructuredRandom((1024,), (1024,), n_layers=2, diagonals=[d.to(dev) for d in diag], device=dev)
    S = sine(1024)
    want = (diag[1].double() * ((diag[0].double() * x.double()) @ S)) @ S
    e = rel_err(p.A(x.to(dev)), want)
    print(f"n = 1024: {e:.3e} (reference {float(GOLD['sr_n1024_A__err']):.3e})")
    assert e <= 2 * float(GOLD["sr_n1024_A__err"])
    with pytest.raises(NotImplementedError, match=str(hd.MAX_N)):
        dinv.physics.functional.dst1(torch.zeros(1, hd.MAX_N + 1, device=dev))
    # the largest row runs.  P = 5850 = 13 5 5 3 3 2: each stage of radix r adds at most (r + 3) u and the scale 2 u (the derivation
    # in tests/test_emu_dst.py), 51 u per transform, two transforms for the involution
    big = dinv.physics.functional.dst1(torch.ones(2, hd.MAX_N, device=dev))
    assert rel_err(dinv.physics.functional.dst1(big), torch.ones(2, hd.MAX_N)) <= 2 * 51 * 2.0 ** -24
