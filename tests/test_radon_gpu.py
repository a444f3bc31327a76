"""Every Radon kernel path of csrc/radon.hip and csrc/radon_tiled.hip on the MI355X against fp64 on the CPU: the whole case table
of tests/radon_cases.py through the C entry points on guarded buffers - including what the host emulation cannot run: config 3
(512^2, 720 angles), the kw = 4 plan at G = 1449, G = 4096 (the last tiled size) and 4097 (gather only), the pack kernels past
65535 blocks and the ramp filter's CT = 2 / CT = 1 lengths with many columns and its direct kernel at the 64 KiB limit - then the
same paths through the Python layer (deepinv_amd.hip.radon, Tomography): normalisation by the device norm scalar (tiled) and
div_ (gather), autograd, views, more than 65535 images per call and empty batches."""

import pytest
import torch

import radon_cases as K

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def runner():
    from deepinv_amd import hip
    from deepinv_amd.hip import radon as hr

    return K.Runner(hr._l(), DEV, lambda: hip.stream_ptr(DEV), fft_plan=lambda n: (hip.fft_plan(n, DEV)[0], hip.fft_plan_host_table(n)))


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.id)
def test_radon_path(runner, case):
    errs = K.run_case(runner, case)
    print(f"{case.id}: " + ", ".join(f"{op} {e:.3g}" for op, e in errs.items()))


def test_empty_batch_entry_points(runner):
    K.run_empty(runner)


def _tables_match(geo, tab):
    """the device tables of hip.radon.RadonGeometry are the ones the fp64 references read"""
    assert torch.equal(geo.cs.cpu(), tab.cs) and torch.equal(geo.xn.cpu(), tab.xn) and torch.equal(geo.ixtab.cpu(), tab.ixtab)
    assert (geo.G, geo.pad_before) == (tab.G, tab.pad)


def _fwd_ratio(y, x, tab, scale):
    yr, M, T = K.ref_forward(tab, x.reshape(-1, tab.W, tab.W).cpu())
    return K.worst_ratio(y.reshape(yr.shape), yr * scale, K._par_measure(tab, M, T) * abs(scale))


def _adj_ratio(xa, v, tab, scale):
    xr, m, T = K.ref_adjoint(tab, v.reshape(-1, tab.G, tab.A).cpu())
    return K.worst_ratio(xa.reshape(xr.shape), xr * scale, K._adj_measure(tab, m, T) * abs(scale))


@pytest.mark.parametrize("tiled", [True, False], ids=["tiled", "gather"])
@pytest.mark.parametrize("W,nang,circle", [(64, 45, False), (50, 30, True)])
def test_normalised_tomography_autograd_and_views(W, nang, circle, tiled, monkeypatch):
    """Tomography(normalize=True): the tiled kernels divide by the device norm scalar, the gather kernels are followed by div_;
    both within their bounds against fp64 / ||A||, autograd through either is the other operator bit for bit, and offset or
    non-contiguous inputs give the bits of their contiguous copies"""
    import deepinv_amd as dinv
    from deepinv_amd.hip import radon as hr

    monkeypatch.setattr(hr, "ENABLE_TILED", tiled)
    g = torch.Generator().manual_seed(W + nang)
    torch.manual_seed(1)
    phys = dinv.physics.Tomography(angles=nang, img_width=W, circle=circle, normalize=True, device=DEV)
    nrm = float(phys.operator_norm)
    assert nrm > 1.0
    tab = K.RadonGeom(phys.angles.cpu(), W, circle)
    _tables_match(phys._geometry(DEV), tab)
    base = torch.randn(2 * W * W + 3, generator=g)
    x = base.to(DEV)[3:].view(2, 1, W, W)
    assert x.storage_offset() == 3
    y = phys.A(x)
    assert torch.equal(y, phys.A(x.clone()))
    assert torch.equal(phys.A(x.transpose(-1, -2)), phys.A(x.transpose(-1, -2).contiguous()))
    key = "fwd_tiled" if tiled else "fwd_gather"
    # the gather path divides after the kernel (div_): one more rounding, inside u G M
    assert _fwd_ratio(y, x, tab, 1.0 / nrm) <= K.BOUNDS[key]
    v = torch.randn(tuple(y.shape), generator=g).to(DEV)
    xa = phys.A_adjoint(v)
    assert _adj_ratio(xa, v, tab, 1.0 / nrm) <= K.BOUNDS["adj_tiled" if tiled else "adj_gather"]
    vt = v.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not vt.is_contiguous() and torch.equal(phys.A_adjoint(vt), xa)
    xg = x.clone().requires_grad_(True)
    (phys.A(xg) * v).sum().backward()
    assert torch.equal(xg.grad, xa)
    vg = v.clone().requires_grad_(True)
    (phys.A_adjoint(vg) * x).sum().backward()
    assert torch.equal(vg.grad, phys.A(x))


def test_forced_tiled_forward_through_the_module(monkeypatch):
    """FORCE_TILED: the kw = 2 plan of 512^2 with 180 angles (production takes the gather kernel there) runs the tiled forward
    with 128-thread workgroups; both forwards agree with fp64 on a subset of angles"""
    from deepinv_amd.hip import radon as hr

    ang = torch.tensor(K.uniform(180))
    geo = hr.RadonGeometry(ang, 512, False, DEV)
    assert geo.plan.kw == 2
    tab = K.RadonGeom(ang, 512, False)
    _tables_match(geo, tab)
    x = torch.randn(3, 1, 512, 512, generator=torch.Generator().manual_seed(5))
    y_gather = hr.radon_forward(x.to(DEV), geo)
    monkeypatch.setattr(hr, "FORCE_TILED", True)
    y_tiled = hr.radon_forward(x.to(DEV), geo)
    sub = [0, 45, 89, 90, 91, 135, 179, 33]
    yr, M, T = K.ref_forward(tab, x[:, 0], sub)
    bound = K._par_measure(tab, M, T)
    assert K.worst_ratio(y_tiled.cpu()[:, 0][:, :, sub], yr, bound) <= K.BOUNDS["fwd_tiled"]
    assert K.worst_ratio(y_gather.cpu()[:, 0][:, :, sub], yr, bound) <= K.BOUNDS["fwd_gather"]


def test_more_than_65535_images_per_call():
    """ramp_filter and iradon_backproject cut the batch at 65535 images per launch: 65537 images at W = 2, every element
    against fp64, and the images on both sides of the cut equal to the same images filtered alone"""
    from deepinv_amd.hip import radon as hr

    n, A = 65537, 3
    geo = hr.RadonGeometry(torch.tensor([10., 70., 135.]), 2, False, DEV)
    tab = K.RadonGeom(torch.tensor([10., 70., 135.]), 2, False)
    _tables_match(geo, tab)
    y = torch.randn(n, 1, geo.G, A, generator=torch.Generator().manual_seed(9))
    yd = y.to(DEV)
    out = hr.ramp_filter(yd)
    e = K.ramp_fft_ratio(out[:, 0], y[:, 0], K.ramp_padded(geo.G))
    print(f"65537 images: ramp {e:.3g}")
    assert e <= K.BOUNDS["ramp_fft"]
    for s in (65534, 65535):
        assert torch.equal(out[s:s + 2], hr.ramp_filter(yd[s:s + 2].clone()))
    bp = hr.iradon_backproject(yd, geo)
    xr, m, T = K.ref_backproject(tab, y[:, 0])
    assert K.worst_ratio(bp.cpu()[:, 0], xr, K.U * A * m + K.ulp(tab.G) * T) <= K.BOUNDS["backproject"]
    assert torch.equal(bp[65534:65536], hr.iradon_backproject(yd[65534:65536].clone(), geo))


def test_empty_batches_through_the_module():
    import deepinv_amd as dinv
    from deepinv_amd.hip import radon as hr

    phys = dinv.physics.Tomography(angles=12, img_width=20, normalize=False, device=DEV)
    y = phys.A(torch.zeros(0, 1, 20, 20, device=DEV))
    assert y.shape[0] == 0 and phys.A_adjoint(y).shape == (0, 1, 20, 20)
    assert hr.ramp_filter(torch.zeros(0, 2, 29, 12, device=DEV)).shape == (0, 2, 29, 12)
    geo = hr.RadonGeometry(torch.tensor(K.uniform(12)), 20, False, DEV)
    assert hr.iradon_backproject(torch.zeros(0, 1, geo.G, 12, device=DEV), geo).shape == (0, 1, 20, 20)
