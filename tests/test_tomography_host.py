"""The Python layer of the Radon operators (deepinv_amd/hip/radon.py) on the host emulation of the kernel sources
(tests/emu_backend.py): which kernels every route launches (read off the emulation's launch log, against
radon_cases.expected_launches), the autograd of the three operator pairs bit for bit, where the operator norm divides, the
errors and the empty batch, and its ctypes prototypes against include/deepinv_amd.h."""
import ctypes
import os
import re

import pytest
import torch

import emu_lib as E
import radon_cases as K
from emu_backend import emu_backend

from deepinv_amd.hip import radon as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "deepinv_amd.h")
W, ANGLES, B, C = 12, K.uniform(8), 1, 2            # G = 17: two 16-pixel tiles per side, NB = 2
FAN_W, FAN_ANGLES = 16, K.uniform(10, 360.0)        # the geometry of fan-W16-det20-aboveG-n1 (radon_cases)
NORM = 13.5


def _case(**kw):
    """the radon_cases entry whose dispatch the Python layer must reproduce"""
    return K.Case("host", "par", True, W=W, angles=ANGLES, n_img=B * C, **kw)


def _data(seed=5):
    g = torch.Generator().manual_seed(seed)
    geo = K.RadonGeom(ANGLES, W, False)
    return torch.randn(B, C, W, W, generator=g), torch.randn(B, C, geo.G, geo.A, generator=g)


def _geometry(plan=False):
    """RadonGeometry on the host (inside emu_backend): no plan unless asked for, as on a CPU device"""
    geo = R.RadonGeometry(torch.tensor(ANGLES), W, False, "cpu")
    assert geo.plan is None and geo.plan_dev is None
    if plan:
        geo.build_plan()
    return geo


def _fan_geometry():
    return R.FanGeometry(torch.tensor(FAN_ANGLES), FAN_W, False, "cpu", K.FAN_A)


def _logged(fn):
    """(result of fn(), the instantiations and block sizes it launched)"""
    l = E.lib()
    l.dinv_emu_launch_log_reset()
    out = fn()
    return out, [l.dinv_emu_launch_log_instance(i).decode() for i in range(l.dinv_emu_launch_log_count())]


@pytest.fixture
def ramp_cache(monkeypatch):
    """the ramp tables built on the host stay out of the cache the device tables live in"""
    monkeypatch.setattr(R, "_ramp_cache", {})


# ------------------------------------------------------------------ launch list per route
def test_gather_routes(monkeypatch):
    monkeypatch.setattr(R, "ENABLE_TILED", False)
    x, v = _data()
    case = _case(gather=True)
    with emu_backend():
        geo = _geometry(plan=True)         # a plan does not bring the tiled forward back
        y, launched = _logged(lambda: R.radon_forward(x, geo))
        assert launched == K.expected_launches(case, "fwd")
        xt, launched = _logged(lambda: R.radon_adjoint(v, geo))
        assert launched == K.expected_launches(case, "adj")
    assert torch.equal(y, E.radon_forward_gather(x, E.RadonGeom(ANGLES, W, False)))
    assert xt.shape == x.shape


def test_tiled_adjoint_and_gather_forward_without_a_plan():
    x, v = _data()
    case = _case(gather=False)
    with emu_backend():
        geo = _geometry()
        xt, launched = _logged(lambda: R.radon_adjoint(v, geo))
        assert launched == K.expected_launches(case, "adj") == ["radon_pack_sino2<2> x256", "radon_adj_tiled_kernel<2> x256"]
        _, launched = _logged(lambda: R.radon_forward(x, geo))
        assert launched == K.expected_launches(_case(gather=True), "fwd")
    assert torch.equal(xt, E.radon_adjoint_tiled(v, E.RadonGeom(ANGLES, W, False)))


def test_tiled_forward_with_a_plan(monkeypatch):
    x, _ = _data()
    with emu_backend():
        geo = _geometry(plan=True)
        kw = geo.plan.kw
        assert kw in (1, 2, 4, 8) and geo.plan_dev.numel() == geo.plan.blob_words
        if kw < 4:
            _, launched = _logged(lambda: R.radon_forward(x, geo))          # too few angles per workgroup: the gather kernel
            assert launched == K.expected_launches(_case(), "fwd", kw) == K.expected_launches(_case(gather=True), "fwd")
            monkeypatch.setattr(R, "FORCE_TILED", True)
        case = _case(force_tiled=kw < 4)
        assert K.forward_is_tiled(case, kw)
        y, launched = _logged(lambda: R.radon_forward(x, geo))
        assert launched == K.expected_launches(case, "fwd", kw)
    ref, pl = E.radon_forward_tiled(x, E.RadonGeom(ANGLES, W, False))
    assert pl.kw == kw and torch.equal(y, ref)


def test_fan_routes():
    g = torch.Generator().manual_seed(6)
    case = K.Case("host-fan", "fan", True, W=FAN_W, angles=FAN_ANGLES, n_img=1, fan=K.FAN_A)
    with emu_backend():
        geo = _fan_geometry()
        assert geo.plan is None and geo.n_det == 20 and geo.xm.shape == (geo.G,)
        x, v = torch.randn(1, 1, FAN_W, FAN_W, generator=g), torch.randn(1, 1, geo.n_det, geo.A, generator=g)
        y, launched = _logged(lambda: R.fan_forward(x, geo))
        assert launched == K.expected_launches(case, "fan_fwd")
        xt, launched = _logged(lambda: R.fan_adjoint(v, geo))
        assert launched == K.expected_launches(case, "fan_adj")
    egeo = E.FanGeom(FAN_ANGLES, FAN_W, False, K.FAN_A)
    assert torch.equal(y, E.radon_fan_forward(x, egeo)) and torch.equal(xt, E.radon_fan_adjoint(v, egeo))


def test_backprojection_route():
    _, v = _data()
    with emu_backend():
        geo = _geometry()
        out, launched = _logged(lambda: R.iradon_backproject(v, geo, 0.5))
    assert launched == K.expected_launches(K.Case("host-bp", "bp", True, W=W, angles=ANGLES, n_img=B * C), "bp")
    assert out.shape == (B, C, W, W) and torch.isfinite(out).all()


@pytest.mark.parametrize("direct", [False, True], ids=["fft", "direct"])
def test_ramp_routes(monkeypatch, ramp_cache, direct):
    _, v = _data()
    monkeypatch.setattr(R, "ENABLE_RAMP_FFT", not direct)
    case = K.Case("host-ramp", "ramp", True, n_img=B * C, N=v.shape[-2], A_ramp=v.shape[-1], direct=direct)
    with emu_backend():
        out, launched = _logged(lambda: R.ramp_filter(v))
    assert launched == K.expected_launches(case, "ramp") == ["ramp_kernel x256" if direct else "ramp_fft_kernel x256"]
    ref = K.ref_ramp(v.view(B * C, *v.shape[-2:])).view(v.shape)
    assert float((out.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


# ------------------------------------------------------------------ autograd: each side's backward is the other, bit for bit
def _pairs():
    """(name, geometry factory, forward, adjoint) of the three operator pairs through the public functions"""
    return [("exact", _geometry, lambda t, g: R.radon_forward(t, g), lambda t, g: R.radon_adjoint(t, g)),
            ("exact-norm", _geometry, lambda t, g: R.radon_forward(t, g, torch.tensor([NORM])),
             lambda t, g: R.radon_adjoint(t, g, torch.tensor([NORM]))),
            ("interpolating", _geometry, lambda t, g: R.apply_radon(t, g, 0.37, False), lambda t, g: R.apply_radon(t, g, 0.37, True)),
            ("fan", _fan_geometry, lambda t, g: R.fan_forward(t, g), lambda t, g: R.fan_adjoint(t, g))]


@pytest.mark.parametrize("name,make,fwd,adj", _pairs(), ids=[p[0] for p in _pairs()])
def test_backward_of_each_side_is_the_other(name, make, fwd, adj):
    g = torch.Generator().manual_seed(8)
    with emu_backend():
        geo = make()
        n_det = geo.n_det if name == "fan" else geo.G
        x = torch.randn(1, 2, geo.W, geo.W, generator=g)
        v = torch.randn(1, 2, n_det, geo.A, generator=g)
        xg = x.clone().requires_grad_()
        (fwd(xg, geo) * v).sum().backward()
        assert torch.equal(xg.grad, adj(v, geo))
        vg = v.clone().requires_grad_()
        (adj(vg, geo) * x).sum().backward()
        assert torch.equal(vg.grad, fwd(x, geo))


def test_double_backward_of_the_exact_pair_is_the_forward_again():
    x, v = _data()
    w = torch.randn(x.shape, generator=torch.Generator().manual_seed(9))
    with emu_backend():
        geo = _geometry()
        xg, vg = x.clone().requires_grad_(), v.clone().requires_grad_()
        (grad_x,) = torch.autograd.grad((R.radon_forward(xg, geo) * vg).sum(), xg, create_graph=True)   # = adjoint(vg)
        (grad_v,) = torch.autograd.grad((grad_x * w).sum(), vg)                                         # = forward(w)
        assert torch.equal(grad_x.detach(), R.radon_adjoint(v, geo)) and torch.equal(grad_v, R.radon_forward(w, geo))


# ------------------------------------------------------------------ where the operator norm divides
def test_tiled_routes_divide_by_the_norm_in_the_kernel(monkeypatch):
    x, v = _data()
    norm = torch.tensor([NORM])
    egeo = E.RadonGeom(ANGLES, W, False)
    with emu_backend():
        geo = _geometry(plan=True)
        monkeypatch.setattr(R, "FORCE_TILED", geo.plan.kw < 4)
        y, launched = _logged(lambda: R.radon_forward(x, geo, norm))
        assert [k.split("<")[0] for k in launched][:2] == ["radon_pack_image2", "radon_fwd_tiled_kernel"]
        xt, launched = _logged(lambda: R.radon_adjoint(v, geo, norm))
        assert launched == K.expected_launches(_case(), "adj")
        plain = R.radon_forward(x, geo)
    assert torch.equal(y, E.radon_forward_tiled(x, egeo, norm=norm)[0])
    assert torch.equal(xt, E.radon_adjoint_tiled(v, egeo, norm=norm))
    assert torch.equal(y, plain / norm) and not torch.equal(y, plain)     # the kernel's v / norm is the same IEEE division
    with emu_backend(), pytest.raises(RuntimeError, match="float32 scalar on the operator's device"):
        R.radon_forward(x, geo, norm.double())


def test_gather_routes_divide_after_the_kernel(monkeypatch):
    x, v = _data()
    norm = torch.tensor([NORM])
    monkeypatch.setattr(R, "ENABLE_TILED", False)
    with emu_backend():
        geo, fan = _geometry(), _fan_geometry()
        xf = torch.randn(1, 1, FAN_W, FAN_W, generator=torch.Generator().manual_seed(3))
        for op, t, g in ((R.radon_forward, x, geo), (R.radon_adjoint, v, geo), (R.fan_forward, xf, fan)):
            plain, launched_plain = _logged(lambda: op(t, g))
            scaled, launched = _logged(lambda: op(t, g, norm))
            assert launched == launched_plain and torch.equal(scaled, plain.clone().div_(norm))
        yf = R.fan_forward(xf, fan)
        assert torch.equal(R.fan_adjoint(yf, fan, norm), R.fan_adjoint(yf, fan).div_(norm))


# ------------------------------------------------------------------ errors and edge cases
def test_sinogram_shape_errors_keep_their_messages():
    with emu_backend():
        geo, fan = _geometry(), _fan_geometry()
        bad = torch.zeros(1, 2, geo.G + 1, geo.A)
        msg = f"sinogram of shape {tuple(bad.shape)} does not match the operator ({geo.G} detectors, {geo.A} angles)"
        with pytest.raises(ValueError, match=re.escape(msg)):
            R.radon_adjoint(bad, geo)
        with pytest.raises(ValueError, match=re.escape(msg)):
            R.iradon_backproject(bad, geo)
        bad = torch.zeros(1, 1, fan.n_det, fan.A + 2)
        msg = f"sinogram of shape {tuple(bad.shape)} does not match the operator ({fan.n_det} detector pixels, {fan.A} angles)"
        with pytest.raises(ValueError, match=re.escape(msg)):
            R.fan_adjoint(bad, fan)


@pytest.mark.parametrize("tiled", [True, False], ids=["tiled", "gather"])
def test_empty_batch_on_every_route(monkeypatch, ramp_cache, tiled):
    monkeypatch.setattr(R, "ENABLE_TILED", tiled)
    monkeypatch.setattr(R, "FORCE_TILED", tiled)
    monkeypatch.setattr(R, "ENABLE_RAMP_FFT", tiled)
    with emu_backend():
        geo, fan = _geometry(plan=True), _fan_geometry()
        x0, y0 = torch.zeros(0, 3, W, W), torch.zeros(0, 3, geo.G, geo.A)
        _, launched = _logged(lambda: [
            _same(R.radon_forward(x0, geo).shape, y0.shape), _same(R.radon_adjoint(y0, geo).shape, x0.shape),
            _same(R.apply_radon(x0, geo, 2.0, False).shape, y0.shape), _same(R.apply_radon(y0, geo, 2.0, True).shape, x0.shape),
            _same(R.iradon_backproject(y0, geo).shape, x0.shape), _same(R.ramp_filter(y0).shape, y0.shape),
            _same(R.fan_forward(torch.zeros(0, 1, FAN_W, FAN_W), fan).shape, (0, 1, fan.n_det, fan.A)),
            _same(R.fan_adjoint(torch.zeros(0, 1, fan.n_det, fan.A), fan).shape, (0, 1, FAN_W, FAN_W))])
    assert launched == []


def _same(a, b):
    assert tuple(a) == tuple(b), (a, b)


def test_chunks_of_65535_images():
    assert list(R._chunks(65537)) == [(0, 65535), (65535, 65537)]
    assert list(R._chunks(0)) == []
    assert list(R._chunks(65535)) == [(0, 65535)] and list(R._chunks(1)) == [(0, 1)]


# ------------------------------------------------------------------ declarations
def test_every_radon_entry_point_has_its_prototype():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {name: [p.strip() for p in params.split(",")] for name, params in
              re.findall(r"\b(dinv_radon_[a-z0-9_]+)\s*\(([^)]*)\)", src)}
    assert {"dinv_radon_forward", "dinv_radon_adjoint", "dinv_radon_forward_tiled", "dinv_radon_adjoint_tiled", "dinv_radon_fan_forward",
            "dinv_radon_fan_adjoint", "dinv_radon_backproject", "dinv_radon_ramp", "dinv_radon_ramp_fft", "dinv_radon_plan_init",
            "dinv_radon_workspace_bytes", "dinv_radon_tiled_workspace_bytes", "dinv_radon_fan_workspace_bytes"} <= set(protos)
    fresh = ctypes.CDLL(E.lib()._name)        # hip/radon.py owns these symbols: its _declare alone sets them
    R._declare(fresh)
    for name, params in protos.items():
        argtypes = getattr(fresh, name).argtypes
        assert argtypes is not None, f"{name}: no argtypes"
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for ({', '.join(params)})"
        for at, p in zip(argtypes, params):
            if p.split()[-1] == "ws_bytes":
                assert at is ctypes.c_size_t, f"{name}: ws_bytes declared as {at}"
        if name.endswith("_bytes"):
            assert getattr(fresh, name).restype is ctypes.c_size_t, name
