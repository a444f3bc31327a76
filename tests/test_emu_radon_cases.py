"""The Radon kernels of csrc/radon.hip and csrc/radon_tiled.hip on the host emulation of the kernel sources (tests/emu), against
fp64: the part of the case table of tests/radon_cases.py that the fiber emulation finishes quickly.  Every call asserts, through
the emulation's launch log, the instantiations (NB, SWAP, MAXPF) and block sizes radon_cases.expected_launches predicts, and after
every tiled call that no tap fell outside the planned window and no contributing detector outside the staged segment.
tests/test_radon_gpu.py runs the whole table on the device."""
import ctypes

import numpy as np
import pytest
import torch

import emu_lib as E
import radon_cases as K


@pytest.fixture(scope="module")
def runner():
    l = E.lib()

    def launches():
        return [l.dinv_emu_launch_log_instance(i).decode() for i in range(l.dinv_emu_launch_log_count())]

    def reset():
        l.dinv_emu_launch_log_reset()
        for name in ("dinv_emu_window_misses", "dinv_emu_segment_misses"):
            ctypes.c_int.in_dll(l, name).value = 0

    def fft_plan(n):
        plan, table = E.fft_plan(n)
        return plan, torch.from_numpy(table)

    return K.Runner(l, "cpu", lambda: ctypes.c_void_p(0), fft_plan=fft_plan, reset=reset, launches=launches)


@pytest.mark.parametrize("case", [c for c in K.CASES if c.emu], ids=lambda c: c.id)
def test_radon_path_emulated(runner, case):
    errs = K.run_case(runner, case)
    print(f"{case.id}: " + ", ".join(f"{op} {e:.3g}" for op, e in errs.items()))


def test_empty_batch_launches_nothing(runner):
    K.run_empty(runner)


def test_case_table_reaches_every_path():
    """the table itself: NB 1 / 2 / 4 / 8 on both pairs, every plan width, both MAXPF values, the ramp's CT values and the
    direct kernel, the G edges of the tiled kernels, every rejection"""
    par = [c for c in K.CASES if c.kind == "par"]
    for gather in (False, True):
        assert {K.nb_of(c.n_img) for c in par if c.emu and c.gather == gather} == {1, 2, 4, 8}
        assert any(c.n_img % K.nb_of(c.n_img) for c in par if c.emu and c.gather == gather and c.n_img > 1)
    assert {c.kw_expect for c in par if c.emu} >= {1, 2, 4, 8}
    assert {c.geo.G for c in par if not c.emu} >= {4096, 4097}
    assert any(c.geo.A == 1 for c in par if c.emu) and any(c.geo.A % 16 and c.geo.A % 4 for c in par if c.emu)
    cts = {K.ramp_ct(K.ramp_padded(c.N)) for c in K.CASES if c.kind == "ramp" and K.ramp_padded(c.N) <= K.RAMP_FFT_MAX_P and
           not c.direct}
    assert cts == {8, 2, 1}
    assert any(K.ramp_padded(c.N) > K.RAMP_FFT_MAX_P for c in K.CASES if c.kind == "ramp" and c.emu)
    assert K.ramp_ct(2048) == 8 and K.ramp_ct(4096) == 2 and K.ramp_ct(8192) == 1


@pytest.mark.parametrize("W,angles,circle", [(20, K.BORDERS, False), (17, K.WILD, True), (12, K.uniform(7), False)])
def test_references_are_a_transpose_pair(W, angles, circle):
    """the fp64 forward (sample enumeration) and adjoint (lattice points around each pixel) are exact transposes of each other;
    the 4 x 4-neighbourhood measures T likewise"""
    geo = K.RadonGeom(angles, W, circle)
    g = torch.Generator().manual_seed(W)
    x = torch.randn(2, W, W, generator=g, dtype=torch.float64)
    v = torch.randn(2, geo.G, geo.A, generator=g, dtype=torch.float64)
    y, M, T = K.ref_forward(geo, x)
    xa, m, Ta = K.ref_adjoint(geo, v)
    disc = geo.disc().double().reshape(-1)
    lhs, rhs = float((y * v).sum()), float((x.reshape(2, -1) * disc * xa).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(y.norm() * v.norm())
    _, _, T1 = K.ref_forward(geo, x.abs())
    assert abs(float((T1 * v.abs()).sum()) - float((x.abs().reshape(2, -1) * disc * Ta).sum())) <= 1e-9 * float(T1.sum())
