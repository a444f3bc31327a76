"""Every dispatch path of the FFT engine (csrc/fft_launch.hpp) on the MI355X against complex128 torch.fft on the CPU: the whole
case table of tests/fft_cases.py through the C entry points (dinv_fft_c2c_axis, dinv_rfft2, dinv_irfft2, dinv_blurfft_apply) on
guarded buffers - including the cases the host emulation cannot run: more than kMaxGrid tiles (grid-stride loops), the wave
kernel's persistent round with the next tile's loads prefetched, and its missing-LDS-ordering failure mode, which only hardware
shows - then the Python layer (deepinv_amd.hip.fft.fftn / ifftn and deepinv_amd.hip.conv.rfft2 / irfft2) on views, every norm,
and autograd."""
import pytest
import torch

import fft_cases as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def runner():
    from deepinv_amd import hip
    from deepinv_amd.hip import conv

    return F.Runner(conv._l(), DEV, lambda n: hip.fft_plan(n, DEV), lambda: hip.stream_ptr(DEV))


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_fft_path(runner, case):
    F.run_case(runner, case)


# ------------------------------------------------------------------ the Python layer
# Bound: these chain up to three passes (wave / static / generic rows, static / generic columns).  The same calls over the emulated
# kernels (deepinv_amd.hip.fft through tests/emu_backend.py) gave a worst per-line error of 3.7e-7 for fftn / ifftn over this table
# and 3.7e-7 for the gradients: about 4x that.
PY_BOUND = 1.5e-6


def _fftn_ref(x, dims, inverse, centered, norm):
    x = x.cpu().to(torch.complex128)
    if centered:
        x = torch.fft.ifftshift(x, dim=dims)
    y = (torch.fft.ifftn if inverse else torch.fft.fftn)(x, dim=dims, norm=norm)
    if centered:
        y = torch.fft.fftshift(y, dim=dims)
    return y


def _randc(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))


@pytest.mark.parametrize("shape", [(2, 320, 320), (2, 257, 320), (8, 64, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dims", [(-2, -1), (-3, -2, -1), (-3,)], ids=lambda d: "d" + "".join(str(-i) for i in d))
@pytest.mark.parametrize("norm", ["ortho", "backward", "forward"])
@pytest.mark.parametrize("centered", [False, True], ids=["plain", "centred"])
def test_hip_fftn_ifftn(shape, dims, norm, centered):
    from deepinv_amd.hip import fft as hf

    x = _randc(shape, sum(shape) + len(dims)).to(torch.complex64)
    xd = x.to(DEV)
    for inverse, fn in ((False, hf.fftn), (True, hf.ifftn)):
        out = fn(xd, dim=dims, norm=norm, centered=centered)
        assert out.dtype == torch.complex64 and out.shape == x.shape
        err = F.worst_line_error(out, _fftn_ref(x, dims, inverse, centered, norm))
        assert err < PY_BOUND, (inverse, err)
        assert torch.equal(xd.cpu(), x), "fftn modified its input"


@pytest.mark.parametrize("centered", [False, True], ids=["plain", "centred"])
def test_hip_fftn_on_views(centered):
    """a transposed (non-contiguous) input and a view at a storage offset give what their contiguous copies give"""
    from deepinv_amd.hip import fft as hf

    base = _randc((3, 64, 257), 5).to(torch.complex64).to(DEV)
    views = {"transposed": base.transpose(-1, -2),                                    # 3 x 257 x 64, strides (., 1, 257)
             "offset": base.reshape(-1)[7:7 + 2 * 320 * 17].view(2, 320, 17)}        # storage offset 7 complex
    for name, v in views.items():
        assert not v.is_contiguous() or v.storage_offset() > 0, name
        out = hf.fftn(v, dim=(-2, -1), norm="ortho", centered=centered)
        err = F.worst_line_error(out, _fftn_ref(v, (-2, -1), False, centered, "ortho"))
        assert err < PY_BOUND, (name, err)
        assert torch.equal(out.cpu(), hf.fftn(v.contiguous(), dim=(-2, -1), norm="ortho", centered=centered).cpu()), name


@pytest.mark.parametrize("dims,norm,centered", [((-2, -1), "ortho", True), ((-3, -2, -1), "backward", False),
                                                ((-3,), "forward", True)])
def test_hip_fftn_backward_matches_cpu_autograd(dims, norm, centered):
    from deepinv_amd.hip import fft as hf

    x = _randc((2, 257, 320), 11).to(torch.complex64)
    g = _randc((2, 257, 320), 12).to(torch.complex64)
    for inverse, fn in ((False, hf.fftn), (True, hf.ifftn)):
        xd = x.to(DEV).requires_grad_(True)
        (gx,) = torch.autograd.grad(fn(xd, dim=dims, norm=norm, centered=centered), xd, g.to(DEV))
        xr = x.to(torch.complex128).requires_grad_(True)
        (gr,) = torch.autograd.grad(_fftn_ref(xr, dims, inverse, centered, norm), xr, g.to(torch.complex128))
        err = F.worst_line_error(gx, gr)
        assert err < PY_BOUND, (inverse, err)


@pytest.mark.parametrize("norm", ["ortho", "backward", "forward"])
def test_hip_rfft2_irfft2_on_offset_views(norm):
    """deepinv_amd.hip.conv.rfft2 / irfft2 of views at a storage offset (data not 16-byte aligned) against torch.fft in fp64"""
    from deepinv_amd.hip import conv as hc

    H, W = 320, 256
    g = torch.Generator().manual_seed(3)
    base = torch.randn(2 * H * W + 5, generator=g)
    x = base[1:1 + 2 * H * W].view(2, H, W)                       # 4-byte storage offset
    xd = base.to(DEV)[1:1 + 2 * H * W].view(2, H, W)
    assert xd.storage_offset() == 1
    spec = hc.rfft2(xd, norm=norm)
    ref = torch.fft.rfft2(x.double(), norm=norm)
    assert F.worst_line_error(spec, ref) < F.BOUNDS["rfft2"]
    sbase = _randc((2 * H * (W // 2 + 1) + 3,), 4).to(torch.complex64)
    s = sbase[3:].view(2, H, W // 2 + 1)                            # 24-byte storage offset, arbitrary imaginary DC / Nyquist
    sd = sbase.to(DEV)[3:].view(2, H, W // 2 + 1)
    back = hc.irfft2(sd, s=(H, W), norm=norm)
    ref = torch.fft.irfft2(s.to(torch.complex128), s=(H, W), norm=norm)
    assert F.worst_line_error(back, ref) < F.BOUNDS["irfft2"]
