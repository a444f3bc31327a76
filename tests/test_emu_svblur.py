"""SpaceVaryingBlur on the host emulation (tests/emu): the product-convolution kernels of csrc/blur.hip (dinv_pconv2d /
dinv_pconv2d_transpose) over the part of the case table of tests/svblur_cases.py the fiber emulation finishes quickly - exact on
integers, per element against fp64 within the counted bounds, the dot test, guarded buffers - with the launch log asserting that
every accepted call is ONE launch of the kernel the restated rules predict; then the class, autograd and golden checks with the
product's Python layer pointed at the emulation.  tests/test_svblur_gpu.py runs the same on the device."""
import ctypes

import pytest
import torch

import emu_lib as E
import svblur_cases as S
from emu_backend import emu_backend


@pytest.fixture(scope="module")
def runner():
    l = E.lib()

    def launches():
        return [l.dinv_emu_launch_log_name(i).decode() for i in range(l.dinv_emu_launch_log_count())]

    return S.Runner(l, "cpu", lambda: ctypes.c_void_p(0), reset=l.dinv_emu_launch_log_reset, launches=launches)


@pytest.mark.parametrize("item", [i for i in S.CASES if i[0].emu], ids=S.item_id)
def test_product_convolution_path_emulated(runner, item):
    S.run_case(runner, *item)


@pytest.mark.parametrize("item", S.refusals(), ids=lambda i: i[0])
def test_bad_arguments_are_refused_emulated(runner, item):
    S.run_refusal(runner, item)


def test_empty_batch_launches_nothing_emulated(runner):
    S.run_empty_batch(runner)


def test_case_table_reaches_every_path():
    """the table itself: the four kernels on the emulation, both sides of the tiled LDS limit, every mode, the scalar store"""
    emu = [i for i in S.CASES if i[0].emu and not S.rejection(*i)]
    reached = {S.expected_kernel(c, m, t) for c, m in emu for t in (False, True)}
    assert reached == {"pconv2d_tiled_kernel", "pconv2d_tiled_transpose_kernel", "pconv2d_pad_kernel", "pconv2d_pad_transpose_kernel"}
    assert {m for _, m in emu} == set(S.ALL)
    sizes = {(c.fh, S.expected_kernel(c, m, False)) for c, m in S.CASES}
    assert {(51, "pconv2d_tiled_kernel"), (52, "pconv2d_tiled_kernel"), (53, "pconv2d_pad_kernel")} <= sizes
    assert any(S.expected_kernel(c, m, True) == "pconv2d_pad_transpose_kernel" and m == "valid" for c, m in emu)
    assert any(c.W % 4 and c.W > 64 for c, _ in emu) and any(c.K == 10 for c, _ in emu)
    assert any(S.rejection(c, m) for c, m in S.CASES)


def test_class_emulated():
    with emu_backend():
        S.check_class("cpu")


def test_autograd_emulated():
    with emu_backend():
        S.check_autograd("cpu")


def test_golden_definition_matches_the_reference():
    S.check_golden_definition(S.golden())


def test_golden_product_emulated():
    with emu_backend():
        S.check_golden_product(S.golden(), "cpu")
