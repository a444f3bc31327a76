"""Total variation on the MI355X (deepinv_amd/csrc/tv.hip through deepinv_amd.models.TVDenoiser / TVL1Denoiser and
deepinv_amd.optim.TVPrior / TVL1Prior) against the real reference's outputs (tests/golden/make_golden_tv.py) and, at the
project's full sizes, against the float64 PyTorch restatement of deepinv/models/tv.py:86-218 in tests/variational_cases.py."""
import os

import numpy as np
import pytest
import torch

import variational_cases as VC
from conftest import rel_err
from variational_cases import r_nabla, r_nabla_adjoint

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(G, "tv.npz"))
    return {k: d[k] for k in d.files}


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------- float64 restatement (tv.py:86-218): tests/variational_cases.py
def r_tv_prox(y, lam, n_it):
    """n_it isotropic iterations from the cold start"""
    return VC.r_tv_prox(y, lam, y.clone(), torch.zeros((*y.shape, y.ndim - 2), dtype=y.dtype, device=y.device), n_it, 0.0, False)[:2]


# ---------------------------------------------------------------- parity with the reference
CASES = [("fixed2d", False), ("fixed3d", False), ("l1fixed2d", True), ("l1fixed3d", True), ("stop2d", False), ("stop3d", False),
         ("l1stop2d", True), ("batch", False), ("batch_first", False)]


@pytest.mark.parametrize("tag,l1", CASES)
def test_denoiser_golden(gold, dev, tag, l1):
    """one prox call (tv.py:86-152): x2 at 1e-5, the stored dual u2, and the same iteration count as the reference's break"""
    import deepinv_amd as dinv

    cls = dinv.models.TVL1Denoiser if l1 else dinv.models.TVDenoiser
    den = cls(n_it_max=int(gold[f"{tag}_nitmax"]), crit=float(gold[f"{tag}_crit"]))
    ths = gold[f"{tag}_ths"]
    ths = float(ths) if ths.ndim == 0 else ths.tolist()
    y = T(gold[f"{tag}_y"], dev)
    out = den(y, ths)
    assert den.n_iter == int(gold[f"{tag}_nit"])
    assert rel_err(out, T(gold[f"{tag}_out"], dev)) < 1e-5
    assert rel_err(den.u2, T(gold[f"{tag}_u2"], dev)) < 1e-4
    assert den.x2.data_ptr() == out.data_ptr() and den.u2.shape == (*y.shape, y.ndim - 2)


def test_one_sample_keeps_the_batch_iterating(gold):
    """the stopping rule is a batch norm: the fixture's second image delays the stop of the first (and both match)"""
    assert int(gold["batch_nit"]) != int(gold["batch_first_nit"])


def test_warm_restart_golden(gold, dev):
    """tv.py:104-117: the second call on an instance starts from the first call's x2 / u2"""
    import deepinv_amd as dinv

    den = dinv.models.TVDenoiser(n_it_max=50, crit=1e-5)
    o1 = den(T(gold["warm_y1"], dev), 0.1)
    assert rel_err(o1, T(gold["warm_out1"], dev)) < 1e-5
    o2 = den(T(gold["warm_y2"], dev), 0.1)
    assert den.n_iter == int(gold["warm_nit"][1])
    assert rel_err(o2, T(gold["warm_out2"], dev)) < 1e-5
    assert rel_err(den.u2, T(gold["warm_u2"], dev)) < 1e-4
    fresh = dinv.models.TVDenoiser(n_it_max=50, crit=1e-5)(T(gold["warm_y2"], dev), 0.1)
    assert rel_err(fresh, o2) > 1e-4                                    # a cold start gives another answer


@pytest.mark.parametrize("tag", ["2d", "3d"])
def test_prior_and_differences_golden(gold, dev, tag):
    import deepinv_amd as dinv

    x, v = T(gold[f"prior{tag}_x"], dev), T(gold[f"prior{tag}_v"], dev)
    p, p1 = dinv.optim.TVPrior(), dinv.optim.prior.TVL1Prior()
    assert p.explicit_prior and p1.explicit_prior
    assert rel_err(p.fn(x), T(gold[f"prior{tag}_fn"], dev)) < 1e-5
    assert rel_err(p(x), T(gold[f"prior{tag}_fn"], dev)) < 1e-5
    assert rel_err(p.grad(x), T(gold[f"prior{tag}_grad"], dev)) < 1e-5
    assert rel_err(p1.fn(x), T(gold[f"prior{tag}_l1fn"], dev)) < 1e-5
    assert rel_err(p1.grad(x), T(gold[f"prior{tag}_l1grad"], dev)) < 1e-5
    assert rel_err(p.nabla(x), T(gold[f"prior{tag}_nabla"], dev)) < 1e-6
    assert rel_err(dinv.models.TVDenoiser.nabla_adjoint(v), T(gold[f"prior{tag}_nabla_adjoint"], dev)) < 1e-6


def test_pgd_tv_blurfft_golden(gold, dev):
    """reference PGD + TVPrior on BlurFFT deblurring (examples/optimization/demo_TV_minimisation.py), 30 outer iterations"""
    import deepinv_amd as dinv

    h = T(gold["blur_filter"], dev)
    p = dinv.physics.BlurFFT(img_size=(3, 64, 64), filter=h, device=dev)
    m = dinv.optim.PGD(prior=dinv.optim.TVPrior(n_it_max=100), data_fidelity=dinv.optim.L2(), stepsize=1.0, lambda_reg=0.05,
                       max_iter=30, early_stop=False)
    with torch.no_grad():
        rec = m(T(gold["blur_y"], dev), p)
    assert rel_err(rec, T(gold["blur_rec"], dev)) < 1e-4


def test_pgd_tv_mri_golden(gold, dev):
    """compressed-sensing MRI: reference PGD + TVPrior on single-coil MRI, 30 outer iterations"""
    import deepinv_amd as dinv

    p = dinv.physics.MRI(mask=T(gold["mri_mask"], dev), img_size=(2, 64, 64), device=dev)
    m = dinv.optim.PGD(prior=dinv.optim.TVPrior(n_it_max=100), data_fidelity=dinv.optim.L2(), stepsize=1.0, lambda_reg=0.02,
                       max_iter=30, early_stop=False)
    with torch.no_grad():
        rec = m(T(gold["mri_y"], dev), p)
    assert rel_err(rec, T(gold["mri_rec"], dev)) < 1e-4


# ---------------------------------------------------------------- full sizes
FULL = [(32, 3, 256, 256), (8, 1, 512, 512), (2, 12, 16, 256, 256)]


@pytest.mark.parametrize("shape", FULL)
def test_full_size_against_fp64(dev, shape):
    """the largest shapes of the project's configurations, per-sample ths, 20 iterations at crit = 0"""
    import deepinv_amd as dinv

    g = torch.Generator().manual_seed(1)
    y = torch.rand(shape, generator=g).to(dev)
    lam = torch.linspace(0.02, 0.2, shape[0])
    den = dinv.models.TVDenoiser(n_it_max=20, crit=0.0)
    out = den(y, lam.to(dev))
    assert den.n_iter == 20
    rx, ru = r_tv_prox(y.double(), lam.double().to(dev), 20)
    assert rel_err(out, rx) < 1e-5
    assert rel_err(den.u2, ru) < 1e-4


@pytest.mark.parametrize("shape", [(4, 3, 256, 256), (2, 3, 16, 64, 64)])
def test_adjoint(dev, shape):
    """<nabla x, v> = <x, nabla^T v>"""
    import deepinv_amd as dinv

    g = torch.Generator().manual_seed(2)
    x = torch.randn(shape, generator=g).to(dev)
    v = torch.randn(*shape, len(shape) - 2, generator=g).to(dev)
    D = dinv.models.TVDenoiser
    gx, av = D.nabla(x), D.nabla_adjoint(v)
    lhs, rhs = (gx.double() * v.double()).sum(), (x.double() * av.double()).sum()
    assert float((lhs - rhs).abs() / (gx.double().norm() * v.double().norm())) < 1e-6
    assert rel_err(gx, r_nabla(x.double())) < 1e-6 and rel_err(av, r_nabla_adjoint(v.double())) < 1e-6


def test_repeated_call_bit_identical(dev):
    """fixed-order reductions: the same state gives the same bits and the same stop"""
    import deepinv_amd as dinv

    y = torch.rand(4, 3, 96, 80, generator=torch.Generator().manual_seed(3)).to(dev)
    a, b = dinv.models.TVDenoiser(), dinv.models.TVDenoiser()
    oa, ob = a(y, [0.05, 0.1, 0.2, 0.3]), b(y, [0.05, 0.1, 0.2, 0.3])
    assert a.n_iter == b.n_iter < 1000 and torch.equal(oa, ob) and torch.equal(a.u2, b.u2)


def test_pnp_tvdenoiser_in_pgd(dev):
    """PnP(TVDenoiser()) in the product's PGD gives the iterates of TVPrior with the same threshold"""
    import deepinv_amd as dinv

    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 3, 64, 64, generator=g).to(dev)
    h = dinv.physics.functional.gaussian_blur(psf_size=(9, 9), sigma=(2.0, 2.0))
    p = dinv.physics.BlurFFT(img_size=(3, 64, 64), filter=h, device=dev)
    y = p.A(x)
    m1 = dinv.optim.PGD(data_fidelity=dinv.optim.L2(), prior=dinv.optim.PnP(dinv.models.TVDenoiser(n_it_max=100, crit=1e-8)),
                        stepsize=1.0, g_param=0.05, max_iter=10)
    m2 = dinv.optim.PGD(data_fidelity=dinv.optim.L2(), prior=dinv.optim.TVPrior(n_it_max=100), stepsize=1.0, lambda_reg=0.05,
                        max_iter=10)
    with torch.no_grad():
        r1, r2 = m1(y, p), m2(y, p)
    assert rel_err(r1, r2) < 1e-6
    assert rel_err(r1, y) > 1e-3


def test_stream_capture_refused(dev):
    import deepinv_amd as dinv

    y = torch.rand(1, 1, 32, 32, device=dev)
    den = dinv.models.TVDenoiser(n_it_max=10)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="captured"):
        with torch.cuda.graph(graph):
            den(y, 0.1)
