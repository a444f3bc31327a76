"""The spatial convolutions of csrc/blur.hip (tiled, strided and generic 2-D kernels, their transposes, the filter gradient and the
3-D kernels) on the host emulation of the kernel sources (tests/emu), against fp64: the part of the case table of
tests/conv_cases.py that the fiber emulation finishes quickly.  Every call also asserts, through the emulation's launch log, that it
reached exactly the kernel conv_cases.expected_kernel predicts: a change to a launcher threshold fails here instead of silently
moving a case to another path.  tests/test_conv_gpu.py runs the whole table on the device."""
import ctypes

import pytest
import torch

import conv_cases as K
import emu_lib as E


@pytest.fixture(scope="module")
def runner():
    l = E.lib()

    def launches():
        return [l.dinv_emu_launch_log_name(i).decode() for i in range(l.dinv_emu_launch_log_count())]

    return K.Runner(l, "cpu", lambda: ctypes.c_void_p(0), reset=l.dinv_emu_launch_log_reset, launches=launches)


@pytest.mark.parametrize("case", [c for c in K.CASES if c.emu], ids=lambda c: c.id)
def test_conv_path_emulated(runner, case):
    errs = K.run_case(runner, case)
    print(f"{case.id}: " + ", ".join(f"{op} {e:.3g}" for op, e in errs.items()))


def test_case_table_reaches_every_path():
    """the table itself: every kernel instantiation on the emulation, the branches of the tiled kernel, the strides of the strided
    kernels, plane chunking on the device"""
    two = [c for c in K.CASES if isinstance(c.conv, K.Conv2) and not c.rejected]
    emu = [c for c in two if c.emu]
    reached = {k for c in emu for op in ("fwd", "adj") for k in c.kernels[op]}
    assert reached == set(K.SHORT), set(K.SHORT) - reached
    tiled = [c.conv for c in emu if c.kernels["fwd"] == ["conv2d_tiled_kernel"]]
    assert {d.fw % 4 for d in tiled} == {0, 1, 2, 3} and any(d.fw == 1 for d in tiled)
    assert {1, 2, 3} <= {d.fh for d in tiled} and any(d.fh >= 4 for d in tiled)
    assert {K.out_size(d.W, d.fw, d.mode) % 4 for d in tiled} == {0, 1, 2, 3}
    assert {d.mode for d in tiled} == set(K.MODES)
    assert any(d.fh > 64 + 1 or d.fw > 64 + 1 or (d.H > 64 and d.W > 64) for d in tiled)
    assert max(d.fh * d.fw for d in tiled if d.fh == d.fw) == 52 * 52
    assert K.tiled_lds(52, 52) <= K.LDS_MAX < K.tiled_lds(53, 53)
    sf = {c.conv.stride for c in emu if c.kernels["fwd"] == ["conv2d_strided_kernel<false>"]}
    assert {2, 3, 5, 8} <= sf
    assert K.strided_lds(4, 4, 8, False) <= K.LDS_MAX < K.strided_lds(5, 5, 8, False)
    st = {c.conv.stride for c in emu if c.kernels["adj"] == ["conv2d_strided_transpose_kernel<false>"]}
    assert set(range(2, 17)) <= st
    assert {12, 16, 17} <= {c.conv.stride for c in emu if c.kernels["fwd"] == ["conv2d_pad_kernel"]}
    three = [c for c in K.CASES if isinstance(c.conv, K.Conv3) and not c.rejected]
    assert all(len(c.kernels[op]) == 2 for c in three if not c.emu for op in ("fwd", "adj"))
    assert any(len(c.kernels["fgrad"]) == 2 for c in three)


def test_launch_log_records_one_entry_per_launch(runner):
    """the emulation's launch log itself: a conv3d cut into no chunks is one launch, and reset empties the log"""
    d = K.Conv3(1, 2, 3, 4, 5, 1, 1, 1, 1, 1, "constant")
    x, k = torch.randn(2 * 3 * 4 * 5), torch.randn(1)
    y = torch.empty_like(x)
    runner.run("dinv_conv3d", d, x, k, y, ["conv3d_pad_kernel"])
    assert torch.equal(y, x * k)
    runner.reset()
    assert runner.launches() == []
