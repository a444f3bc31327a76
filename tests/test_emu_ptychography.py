"""Ptychography on the host emulation of the kernels: the ptychography kernels of deepinv_amd/csrc/cstructured.hip built for the
host by tests/emu/Makefile, and the product's Python layer pointed at them (tests/emu_backend.py).  The cases and their bounds are
those of tests/ptychography_cases.py.  The emulation reports 16 compute units, so the group size the library chooses for the
docstring case differs from the GPU's; both are the split form."""
import ctypes

import pytest
import torch

from emu_backend import emu_backend
import phase_retrieval_cases as PC
import ptychography_cases as PT
from ptychography_cases import C128, GOLD, cdot, crel, up

import deepinv_amd as dinv
from deepinv_amd.hip import cdense as hcd
from deepinv_amd.hip import ptycho as hpt
from deepinv_amd.physics.phase_retrieval import generate_shifts

DEV = torch.device("cpu")


@pytest.fixture(autouse=True, scope="module")
def _emu():
    with emu_backend() as emu:
        yield emu


@pytest.mark.parametrize("tag", PT.TAGS)
def test_golden_operators(tag):
    p, r = PT.physics(tag, DEV)
    x, yc, _, _ = PT.run_operators(tag, p, r, DEV)
    assert cdot(p.B, x, yc) <= 1e-5                                 # with the conjugate: also for the complex probe of c16
    assert torch.equal(p.B(x), p.B(x))


@pytest.mark.parametrize("tag", PT.TAGS)
def test_autograd(tag):
    p, r = PT.physics(tag, DEV)
    PT.run_autograd(tag, p, r, DEV, GOLD[f"{tag}_zero_planes"])


@pytest.mark.parametrize("tag", PT.TAGS)
def test_epilogues_and_normal(tag):
    p, r = PT.physics(tag, DEV)
    x = PT.gold(f"{tag}_x", DEV)
    PC.run_epilogues(p, r, x, float(GOLD[f"{tag}_B__err"]), DEV)
    PT.run_normal(tag, p, r, DEV)


@pytest.mark.parametrize("tag", ["p12x20", "c16"])
def test_zero_probe_planes(tag):
    p, _ = PT.physics(tag, DEV)
    PT.run_zero_planes(tag, p, DEV)


def test_complex_probe_adjoint_and_spectral():
    """the adjoint conjugates the probe: the stored B_adjoint is the reference's A_adjoint on the conjugated buffer, and the
    reference's own (unconjugated) product is not the adjoint of B"""
    p, r = PT.physics("c16", DEV)
    assert p.B.probe.dtype == torch.complex64
    _, yc, _, _ = PT.inputs("c16", DEV)
    plain = (up(p.B.probe) * torch.fft.ifft2(up(yc), norm="ortho")).sum(dim=1, keepdim=True)
    assert crel(p.B_adjoint(yc), plain) > 0.1
    PT.run_spectral("c16", p, r, DEV)


def test_group_forms():
    """forced groups of 1, 2, 3 (ragged: 3 + 1) and 4 positions on p16: within the bounds, bit-identical from call to call, and
    the single-group, the split and the ragged form all occur"""
    p, r = PT.physics("p16", DEV)
    seen = set()
    for G in (1, 2, 3, 4):
        n = PT.probe_groups(p, 2, hpt.ADJOINT, G)
        assert n == PT.probe_groups(p, 2, hpt.NORMAL, G) == -(-4 // G)
        seen.add("single" if n == 1 else "ragged" if 4 % G else "split")
        PT.run_adjoint("p16", p, r, DEV, G)
        PT.run_normal("p16", p, r, DEV, G)
    assert seen == {"single", "split", "ragged"}
    # a group above n_img means n_img: the single-group form, bit for bit
    _, yc, _, _ = PT.inputs("p16", DEV)
    assert PT.probe_groups(p, 2, hpt.ADJOINT, 9) == 1
    assert torch.equal(p.B.A_adjoint(yc, group=9), p.B.A_adjoint(yc, group=4))


@pytest.mark.parametrize("B", [1])
def test_docstring_case(B):
    """the reference's docstring example with its defaults (disk probe of radius 10, 25 shifts), the group size chosen by the
    library: the split form.  The batch of 3 takes the fibers seven seconds and runs on the GPU only."""
    p, r = PT.physics("doc", DEV)
    key = f"doc_b{B}"
    x, yc, _, _ = PT.run_operators(key, p, r, DEV)
    assert tuple(p(x[:1]).shape) == (1, 25, 64, 64) and p.B.probe.dtype == torch.float32
    assert PT.probe_groups(p, B, hpt.ADJOINT) > 1 and PT.probe_groups(p, B, hpt.NORMAL) > 1
    PT.run_adjoint(key, p, r, DEV, 0)
    PT.run_normal(key, p, r, DEV)
    PT.run_autograd(key, p, r, DEV, [])
    assert cdot(p.B, x, yc) <= 1e-5


def test_argument_errors():
    img = (1, 16, 16)
    with pytest.raises(ValueError, match=r"\(1, H, W\)"):
        dinv.physics.Ptychography(img_size=(2, 16, 16), device=DEV)
    with pytest.raises(ValueError, match="perfect square"):
        generate_shifts(img, n_img=8)
    with pytest.raises(TypeError, match="float32 or complex64"):
        dinv.physics.Ptychography(img_size=img, probe=torch.ones(img, dtype=torch.float64), device=DEV)
    p, _ = PT.physics("p16", DEV)
    x = PT.gold("p16_x", DEV)
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

