"""SpaceVaryingBlur without a device and without the emulation: the built gfx950 library exports the two entry points, the Python
layer validates shapes and dtypes before it reaches a kernel, CPU tensors are refused (there is no CPU fallback), and the two
buffers round-trip through a state dict."""
import ctypes
import os

import pytest
import torch

import deepinv_amd as dinv
from deepinv_amd.hip import HipExtensionError
from deepinv_amd.physics import functional as dF


def _params(B=1, C=1, K=2, H=8, W=9, fh=3, fw=3):
    g = torch.Generator().manual_seed(3)
    return torch.randn(B, C, K, fh, fw, generator=g), torch.randn(B, C, K, H, W, generator=g)


def test_library_exports_the_entry_points():
    path = os.path.join(os.path.dirname(os.path.abspath(dinv.__file__)), "libdeepinv_amd.so")
    lib = ctypes.CDLL(path)
    for name in ("dinv_pconv2d", "dinv_pconv2d_transpose"):
        assert hasattr(lib, name), name


def test_class_is_exported_with_the_reference_buffers():
    h, w = _params()
    p = dinv.physics.SpaceVaryingBlur(filters=h, multipliers=w, padding="reflect")
    assert isinstance(p, dinv.physics.LinearPhysics) and p.padding == "reflect" and p.use_fft is False
    assert set(p.state_dict()) >= {"filters", "multipliers"}
    assert torch.equal(p.filters, h) and torch.equal(p.multipliers, w)
    empty = dinv.physics.SpaceVaryingBlur()
    assert empty.filters is None and empty.multipliers is None and empty.padding == "valid"


def test_state_dict_round_trip():
    h, w = _params()
    p = dinv.physics.SpaceVaryingBlur(filters=h, multipliers=w)
    q = dinv.physics.SpaceVaryingBlur(filters=torch.zeros_like(h), multipliers=torch.zeros_like(w))
    q.load_state_dict(p.state_dict())
    assert torch.equal(q.filters, h) and torch.equal(q.multipliers, w)


def test_cpu_tensors_raise():
    h, w = _params()
    x = torch.randn(1, 1, 8, 9)
    p = dinv.physics.SpaceVaryingBlur(filters=h, multipliers=w, padding="circular")
    for fn in (lambda: p.A(x), lambda: p.A_adjoint(x), lambda: dF.product_convolution2d(x, w, h), lambda: dF.multiplier(x, w[:, :, 0]),
               lambda: dF.multiplier_adjoint(x, w[:, :, 0]), lambda: dF.product_convolution2d_adjoint(x, w, h, "circular", use_fft=True)):
        with pytest.raises(RuntimeError):
            fn()
    assert issubclass(HipExtensionError, RuntimeError)


def test_shapes_and_dtypes_are_validated_before_any_kernel():
    h, w = _params()
    x = torch.randn(1, 1, 8, 9)
    p = dinv.physics.SpaceVaryingBlur(filters=h, multipliers=w, padding="reflect")
    with pytest.raises(ValueError, match="2-D only"):
        p.A(torch.randn(1, 1, 4, 8, 9))
    with pytest.raises(ValueError, match="2-D only"):
        p.A_adjoint(torch.randn(1, 1, 4, 8, 9))
    with pytest.raises(ValueError, match="complex"):
        dF.product_convolution2d(x, w.to(torch.complex64), h)
    with pytest.raises(ValueError, match="complex"):
        dF.multiplier(x, w[:, :, 0].to(torch.complex64))
    with pytest.raises(ValueError, match="complex"):
        dF.multiplier_adjoint(x, w[:, :, 0].to(torch.complex64))
    with pytest.raises(ValueError, match="same number of dimension"):
        dF.multiplier(x, w)
    with pytest.raises(ValueError, match="K = "):
        dF.product_convolution2d(x, w, h[:, :, :1])
    with pytest.raises(ValueError, match="K = "):
        dF.product_convolution2d_adjoint(x, w, h[:, :, :1])
    with pytest.raises(ValueError, match="not implemented"):
        dF.product_convolution2d(x, w, h, padding="mirror")
    with pytest.raises(ValueError, match="not implemented"):
        p.A(x, padding="mirror")
    with pytest.raises(ValueError, match="5D"):
        dF.product_convolution2d(x, w[:, :, 0], h)
    with pytest.raises(ValueError, match="needs both"):
        dinv.physics.SpaceVaryingBlur(filters=h).A(x)


def test_broadcast_dims_are_validated():
    """dims that do not broadcast are a ValueError of the wrapper (checked before the library is asked anything on the device
    path; here through the checker itself, which needs no device)"""
    from deepinv_amd.hip import conv as hc

    h, w = _params(B=3)
    with pytest.raises(ValueError, match="do not broadcast"):
        hc._pconv_desc(2, 1, (8, 9), w, h[:1], "reflect")
    with pytest.raises(ValueError, match="do not broadcast"):
        hc._pconv_desc(2, 1, (8, 9), w[:1], h, "reflect")
    with pytest.raises(ValueError, match="do not match the image size"):
        hc._pconv_desc(1, 1, (8, 8), w[:1], h[:1], "reflect")
