"""Ptychography on the GPU through the public classes: the cases and bounds of tests/ptychography_cases.py (the golden vectors of
the real reference and complex128 restatements), which tests/test_emu_ptychography.py runs on the host emulation."""
import ctypes

import pytest
import torch

import phase_retrieval_cases as PC
import ptychography_cases as PT
from ptychography_cases import C128, GOLD, cdot, crel, up

import deepinv_amd as dinv
from deepinv_amd.hip import cdense as hcd
from deepinv_amd.hip import ptycho as hpt
from deepinv_amd.physics.phase_retrieval import generate_shifts

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", PT.TAGS)
def test_golden_operators(tag, dev):
    p, r = PT.physics(tag, dev)
    x, yc, _, _ = PT.run_operators(tag, p, r, dev)
    assert cdot(p.B, x, yc) <= 1e-5                                 # with the conjugate: also for the complex probe of c16
    assert torch.equal(p.B(x), p.B(x))


@pytest.mark.parametrize("tag", PT.TAGS)
def test_autograd(tag, dev):
    p, r = PT.physics(tag, dev)
    PT.run_autograd(tag, p, r, dev, GOLD[f"{tag}_zero_planes"])


@pytest.mark.parametrize("tag", PT.TAGS)
def test_epilogues_and_normal(tag, dev):
    p, r = PT.physics(tag, dev)
    x = PT.gold(f"{tag}_x", dev)
    PC.run_epilogues(p, r, x, float(GOLD[f"{tag}_B__err"]), dev)
    PT.run_normal(tag, p, r, dev)


@pytest.mark.parametrize("tag", ["p12x20", "c16"])
def test_zero_probe_planes(tag, dev):
    p, _ = PT.physics(tag, dev)
    PT.run_zero_planes(tag, p, dev)


def test_complex_probe_adjoint_and_spectral(dev):
    """the adjoint conjugates the probe: the stored B_adjoint is the reference's A_adjoint on the conjugated buffer, and the
    reference's own (unconjugated) product is not the adjoint of B"""
    p, r = PT.physics("c16", dev)
    assert p.B.probe.dtype == torch.complex64
    _, yc, _, _ = PT.inputs("c16", dev)
    plain = (up(p.B.probe) * torch.fft.ifft2(up(yc), norm="ortho")).sum(dim=1, keepdim=True)
    assert crel(p.B_adjoint(yc), plain) > 0.1
    PT.run_spectral("c16", p, r, dev)


def test_group_forms(dev):
    """forced groups of 1, 2, 3 (ragged: 3 + 1) and 4 positions on p16: within the bounds, bit-identical from call to call, and
    the single-group, the split and the ragged form all occur"""
    p, r = PT.physics("p16", dev)
    seen = set()
    for G in (1, 2, 3, 4):
        n = PT.probe_groups(p, 2, hpt.ADJOINT, G)
        assert n == PT.probe_groups(p, 2, hpt.NORMAL, G) == -(-4 // G)
        seen.add("single" if n == 1 else "ragged" if 4 % G else "split")
        PT.run_adjoint("p16", p, r, dev, G)
        PT.run_normal("p16", p, r, dev, G)
    assert seen == {"single", "split", "ragged"}
    # a group above n_img means n_img: the single-group form, bit for bit
    _, yc, _, _ = PT.inputs("p16", dev)
    assert PT.probe_groups(p, 2, hpt.ADJOINT, 9) == 1
    assert torch.equal(p.B.A_adjoint(yc, group=9), p.B.A_adjoint(yc, group=4))


@pytest.mark.parametrize("B", [1, 3])
def test_docstring_case(B, dev):
    """the reference's docstring example with its defaults (disk probe of radius 10, 25 shifts), the group size chosen by the
    library: the split form"""
    p, r = PT.physics("doc", dev)
    key = f"doc_b{B}"
    x, yc, _, _ = PT.run_operators(key, p, r, dev)
    assert tuple(p(x[:1]).shape) == (1, 25, 64, 64) and p.B.probe.dtype == torch.float32
    assert PT.probe_groups(p, B, hpt.ADJOINT) > 1 and PT.probe_groups(p, B, hpt.NORMAL) > 1
    PT.run_adjoint(key, p, r, dev, 0)
    PT.run_normal(key, p, r, dev)
    PT.run_autograd(key, p, r, dev, [])
    assert cdot(p.B, x, yc) <= 1e-5


def test_argument_errors(dev):
    img = (1, 16, 16)
    with pytest.raises(ValueError, match=r"\(1, H, W\)"):
        dinv.physics.Ptychography(img_size=(2, 16, 16), device=dev)
    with pytest.raises(ValueError, match="perfect square"):
        generate_shifts(img, n_img=8)
    with pytest.raises(TypeError, match="float32 or complex64"):
        dinv.physics.Ptychography(img_size=img, probe=torch.ones(img, dtype=torch.float64), device=dev)
    p, _ = PT.physics("p16", dev)
    x = PT.gold("p16_x", dev)
    with pytest.raises(TypeError, match=r"\.to\(torch\.cfloat\)"):
        p.B(x.real.contiguous())
    with pytest.raises(TypeError, match=r"\.to\(torch\.cfloat\)"):
        p.B(x.to(C128))
    with pytest.raises(ValueError, match="expected an input"):
        p.B(x[:, :, :8])
    with pytest.raises(ValueError, match="WEIGHT or the AMPLITUDE"):
        hpt.apply(x[:, 0], p.B.probe, hpt.NORMAL, hcd.ABS2)
    with pytest.raises(ValueError, match="group"):
        hpt.apply(x[:, 0], p.B.probe, hpt.NORMAL, hcd.WEIGHT, torch.ones(2, 4, 16, 16, device=x.device), group=-1)
    # the C entry point: x == out, a workspace that is too small, an epilogue the operation does not take
    l = hpt._l()
    xs, probe = x[:, 0].contiguous(), p.B.probe
    yc, out = torch.zeros(2, 4, 16, 16, dtype=torch.complex64, device=x.device), torch.zeros(2, 16, 16, dtype=torch.complex64, device=x.device)
    ptr, stream_ptr = hpt.ptr, hpt.stream_ptr
    pw, tw = hpt.fft_plan(16, x.device)
    call = lambda a, o, op, ep, group, ws, nbytes: l.dinv_ptycho_apply(ptr(a), ptr(o), ptr(probe), 0, None, 2, 4, 16, 16, op, ep, 0.0, group,
                                                                       ctypes.byref(pw), ptr(tw), ctypes.byref(pw), ptr(tw), ptr(ws), nbytes,
                                                                       stream_ptr(x.device))
    assert call(xs, xs, hpt.FORWARD, hcd.NONE, 0, None, 0) != 0 and b"distinct" in l.dinv_last_error()
    need = l.dinv_ptycho_workspace_bytes(2, 4, 16, 16, hpt.ADJOINT, 1)
    assert need == 2 * 4 * 16 * 16 * 8 and l.dinv_ptycho_workspace_bytes(2, 4, 16, 16, hpt.ADJOINT, 4) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=x.device)
    assert call(yc, out, hpt.ADJOINT, hcd.NONE, 1, ws, need - 8) != 0 and b"workspace" in l.dinv_last_error()
    assert call(yc, out, hpt.ADJOINT, hcd.NONE, 1, None, 0) != 0 and b"workspace" in l.dinv_last_error()
    assert call(yc, out, hpt.ADJOINT, hcd.ABS2, 1, ws, need) != 0 and b"no epilogue" in l.dinv_last_error()
    assert call(xs, out, hpt.NORMAL, hcd.NONE, 1, ws, need) != 0 and b"WEIGHT" in l.dinv_last_error()
    assert call(yc, out, hpt.ADJOINT, hcd.NONE, -1, ws, need) != 0 and b"group" in l.dinv_last_error()
    assert call(yc, out, 3, hcd.NONE, 0, ws, need) != 0 and b"unknown operation" in l.dinv_last_error()
    assert call(yc, out, hpt.ADJOINT, hcd.NONE, 1, ws, need) == 0


def test_lds_boundary(dev):
    """the largest plane of the fused kernels (99 x 99) and the next size up, which takes the composed path"""
    PT.run_boundary(dev)
