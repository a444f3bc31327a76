"""Total generalized variation on the MI355X (deepinv_amd/csrc/tgv.hip through deepinv_amd.models.TGVDenoiser) against the
real reference's outputs (tests/golden/make_golden_tgv.py) and, at full size, against the float64 PyTorch restatement of
deepinv/models/tgv.py:93-310 in tests/variational_cases.py."""
import os

import numpy as np
import pytest
import torch

import variational_cases as VC
from conftest import rel_err
from variational_cases import r_epsilon, r_epsilon_adjoint

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(G, "tgv.npz"))
    return {k: d[k] for k in d.files}


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ths_of(a):
    return float(a) if a.ndim == 0 else a.tolist()


# ---------------------------------------------------------------- float64 restatement (tgv.py:93-310): tests/variational_cases.py
def r_tgv_prox(y, lam, n_it):
    """n_it iterations from the cold start"""
    nd = y.ndim - 2
    r2 = torch.zeros((*y.shape, nd), dtype=y.dtype, device=y.device)
    u2 = torch.zeros((*y.shape, nd * nd), dtype=y.dtype, device=y.device)
    return VC.r_tgv_prox(y, lam, y.clone(), r2, u2, n_it, 0.0)[:3]


# ---------------------------------------------------------------- parity with the reference
# (tag, bound on u2): the dual amplifies rounding (sigma = 1.39 in 2-D); about 4x what the emulated kernels reach
CASES = [("fixed2d", 1e-4), ("fixed3d", 1e-4), ("stop2d", 1e-4), ("stop3d", 1e-4), ("stop2d_late", 1e-3)]


@pytest.mark.parametrize("tag,ubound", CASES)
def test_denoiser_golden(gold, dev, tag, ubound):
    """one prox call (tgv.py:93-214): x2 and r2 at 1e-5, u2, and the same iteration count as the reference's break"""
    import deepinv_amd as dinv

    den = dinv.models.TGVDenoiser(n_it_max=int(gold[f"{tag}_nitmax"]), crit=float(gold[f"{tag}_crit"]))
    y = T(gold[f"{tag}_y"], dev)
    out = den(y, ths_of(gold[f"{tag}_ths"]))
    assert den.n_iter == int(gold[f"{tag}_nit"])
    assert den.has_converged == bool(gold[f"{tag}_converged"])
    assert rel_err(out, T(gold[f"{tag}_out"], dev)) < 1e-5
    assert rel_err(den.r2, T(gold[f"{tag}_r2"], dev)) < 1e-5
    assert rel_err(den.u2, T(gold[f"{tag}_u2"], dev)) < ubound
    nd = y.ndim - 2
    assert den.x2.data_ptr() == out.data_ptr() and den.r2.shape == (*y.shape, nd) and den.u2.shape == (*y.shape, nd * nd)


def test_warm_restart_golden(gold, dev):
    """tgv.py:107-119: the second call on an instance starts from the first call's x2 / r2 / u2"""
    import deepinv_amd as dinv

    den = dinv.models.TGVDenoiser(n_it_max=25, crit=0.0)
    o1 = den(T(gold["warm_y1"], dev), 0.2)
    assert rel_err(o1, T(gold["warm_out1"], dev)) < 1e-5
    o2 = den(T(gold["warm_y2"], dev), 0.2)
    assert den.n_iter == int(gold["warm_nit"][1])
    assert rel_err(o2, T(gold["warm_out2"], dev)) < 1e-5
    assert rel_err(den.r2, T(gold["warm_r2"], dev)) < 1e-5
    assert rel_err(den.u2, T(gold["warm_u2"], dev)) < 1e-4
    fresh = dinv.models.TGVDenoiser(n_it_max=25, crit=0.0)(T(gold["warm_y2"], dev), 0.2)
    assert rel_err(fresh, o2) > 1e-4                                    # a cold start gives another answer


@pytest.mark.parametrize("tag", ["2d", "3d"])
def test_epsilon_golden(gold, dev, tag):
    import deepinv_amd as dinv

    D = dinv.models.TGVDenoiser
    assert rel_err(D.epsilon(T(gold[f"eps{tag}_v"], dev)), T(gold[f"eps{tag}_eps"], dev)) < 1e-6
    assert rel_err(D.epsilon_adjoint(T(gold[f"eps{tag}_u"], dev)), T(gold[f"eps{tag}_adj"], dev)) < 1e-6


def test_pgd_pnp_tgv_golden(gold, dev):
    """reference PGD + PnP(TGVDenoiser) on BlurFFT deblurring, 8 outer iterations of 30 inner ones (warm-restarted)"""
    import deepinv_amd as dinv

    p = dinv.physics.BlurFFT(img_size=(3, 32, 32), filter=T(gold["pgd_filter"], dev), device=dev)
    m = dinv.optim.PGD(prior=dinv.optim.PnP(dinv.models.TGVDenoiser(n_it_max=30, crit=0.0)), data_fidelity=dinv.optim.L2(),
                       stepsize=1.0, g_param=0.1, max_iter=8, early_stop=False)
    with torch.no_grad():
        rec = m(T(gold["pgd_y"], dev), p)
    assert rel_err(rec, T(gold["pgd_rec"], dev)) < 1e-5


def test_pnp_tgv_in_hqs(dev):
    """PnP(TGVDenoiser()) works unchanged in HQS: the prior's prox is the TGV prox"""
    import deepinv_amd as dinv

    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 3, 48, 48, generator=g).to(dev)
    h = dinv.physics.functional.gaussian_blur(psf_size=(9, 9), sigma=(2.0, 2.0))
    p = dinv.physics.BlurFFT(img_size=(3, 48, 48), filter=h, device=dev)
    y = p.A(x)
    m = dinv.optim.HQS(data_fidelity=dinv.optim.L2(), prior=dinv.optim.PnP(dinv.models.TGVDenoiser(n_it_max=20)),
                       stepsize=1.0, g_param=0.05, max_iter=5)
    with torch.no_grad():
        rec = m(y, p)
    assert torch.isfinite(rec).all() and rel_err(rec, y) > 1e-3


# ---------------------------------------------------------------- full sizes
FULL = [(32, 3, 256, 256), (2, 2, 16, 64, 64)]


@pytest.mark.parametrize("shape", FULL)
def test_full_size_against_fp64(dev, shape):
    """per-sample ths, 20 iterations at crit = 0"""
    import deepinv_amd as dinv

    g = torch.Generator().manual_seed(1)
    y = torch.rand(shape, generator=g).to(dev)
    lam = torch.linspace(0.05, 0.4, shape[0])
    den = dinv.models.TGVDenoiser(n_it_max=20, crit=0.0)
    out = den(y, lam.to(dev))
    assert den.n_iter == 20 and not den.has_converged
    rx, rr, ru = r_tgv_prox(y.double(), lam.double().to(dev), 20)
    assert rel_err(out, rx) < 1e-5
    assert rel_err(den.r2, rr) < 1e-4
    assert rel_err(den.u2, ru) < 1e-4


@pytest.mark.parametrize("shape", [(4, 3, 256, 256), (2, 3, 16, 64, 64)])
def test_adjoint(dev, shape):
    """<eps v, u> = <v, eps^T u>, and both against the restatement"""
    import deepinv_amd as dinv

    g = torch.Generator().manual_seed(2)
    nd = len(shape) - 2
    v = torch.randn(*shape, nd, generator=g).to(dev)
    u = torch.randn(*shape, nd * nd, generator=g).to(dev)
    D = dinv.models.TGVDenoiser
    ev, au = D.epsilon(v), D.epsilon_adjoint(u)
    lhs, rhs = (ev.double() * u.double()).sum(), (v.double() * au.double()).sum()
    assert float((lhs - rhs).abs() / (ev.double().norm() * u.double().norm())) < 1e-6
    assert rel_err(ev, r_epsilon(v.double())) < 1e-6 and rel_err(au, r_epsilon_adjoint(u.double())) < 1e-6


def test_repeated_call_bit_identical(dev):
    """fixed-order reductions: the same input gives the same bits, on one instance (after a restart) and on two"""
    import deepinv_amd as dinv

    y = torch.rand(4, 3, 96, 80, generator=torch.Generator().manual_seed(3)).to(dev)
    ths = [0.05, 0.1, 0.2, 0.3]
    a, b = dinv.models.TGVDenoiser(n_it_max=60, crit=0.0), dinv.models.TGVDenoiser(n_it_max=60, crit=0.0)
    oa, ob = a(y, ths).clone(), b(y, ths)
    assert torch.equal(oa, ob) and torch.equal(a.r2, b.r2) and torch.equal(a.u2, b.u2)
    a.restart = True
    assert torch.equal(a(y, ths), ob) and torch.equal(a.u2, b.u2)
    c, d = dinv.models.TGVDenoiser(crit=1e-3), dinv.models.TGVDenoiser(crit=1e-3)
    assert torch.equal(c(y, ths), d(y, ths)) and c.n_iter == d.n_iter == 3 and c.has_converged


def test_verbose_messages(dev, capsys):
    import deepinv_amd as dinv

    y = torch.rand(1, 1, 24, 24, generator=torch.Generator().manual_seed(5)).to(dev)
    dinv.models.TGVDenoiser(verbose=True, n_it_max=5, crit=0.0)(y, 0.1)
    assert "did not converge, stopped after 5 iterations" in capsys.readouterr().out
    dinv.models.TGVDenoiser(verbose=True, crit=1.0)(y, 0.1)
    assert "TGV prox reached convergence" in capsys.readouterr().out


def test_stream_capture_refused(dev):
    import deepinv_amd as dinv

    y = torch.rand(1, 1, 32, 32, device=dev)
    den = dinv.models.TGVDenoiser(n_it_max=10)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="captured"):
        with torch.cuda.graph(graph):
            den(y, 0.1)
