"""The FFT engine's dispatch paths (csrc/fft_launch.hpp: wave, static v4, static scalar and generic rows kernels, static and
generic column kernels, the fused BlurFFT column pass) on the host emulation of the kernel sources (tests/emu), against
complex128 torch.fft: the part of the case table of tests/fft_cases.py that the fiber emulation finishes quickly (line counts up
to a few hundred, no grid-crossing cases).  Each case checks the worst per-transform error, guard bands around every output,
in-place against out-of-place and call-to-call reproducibility; tests/test_fft_gpu.py runs the whole table on the device."""
import ctypes

import pytest
import torch

import emu_lib as E
import fft_cases as F

_plans = {}


def _plan(n):
    if n not in _plans:
        plan, table = E.fft_plan(n)
        _plans[n] = (plan, torch.from_numpy(table))
    return _plans[n]


@pytest.fixture(scope="module")
def runner():
    return F.Runner(E.lib(), "cpu", _plan, lambda: ctypes.c_void_p(0))


@pytest.mark.parametrize("case", [c for c in F.CASES if c.emu], ids=lambda c: c.id)
def test_fft_path_emulated(runner, case):
    err = F.run_case(runner, case)
    print(f"{case.id}: worst per-transform error {err:.3g} (bound {F.BOUNDS[case.family]:.3g})")


def test_case_table_reaches_every_path():
    """the table itself: every static length on each axis, the wave kernel's persistent round, the grid-stride tails"""
    c2c = [c for c in F.CASES if c.kind == "c2c"]
    assert {c.n for c in c2c if c.inner == 1 and c.family == "rows-wave"} == set(F.WAVE_ROWS)
    assert {c.n for c in c2c if c.inner == 1 and c.family == "rows-v4"} == {64, 128}
    assert {c.n for c in c2c if c.inner > 1 and c.family == "cols-static"} == set(F.STATIC_COLS)
    assert any(c.family == "rows-wave" and c.outer > 2 * 8192 for c in c2c)
    assert any(c.family == "rows-v4" and c.outer > F.KMAX_GRID * F.rows_tile(c.n) for c in c2c)
    assert any(c.family == "cols-static" and c.outer * -(-c.inner // F.cols_tile(c.n)) > F.KMAX_GRID for c in c2c)
    r2 = [c for c in F.CASES if c.kind == "rfft2"]
    assert set(F.STATIC_ROWS) <= {c.W for c in r2} and set(F.STATIC_COLS) <= {c.H for c in r2}
    assert any(c.outer * c.H > F.KMAX_GRID * F.rows_tile(c.W) for c in r2)
    bl = [c for c in F.CASES if c.kind == "blurfft"]
    assert set(F.FUSED_BLUR_H) | {16, 17, 100} <= {c.H for c in bl} and {64, 255, 256, 320} <= {c.W for c in bl}
    assert any(c.Ps == c.outer for c in bl) and any(c.Ps < c.outer for c in bl)
    assert any(c.outer * -(-(c.W // 2 + 1) // 16) > 4 * F.KMAX_GRID for c in bl if c.H == 64)


def test_lds_limit_lengths_match_the_plans():
    """the lengths the LDS-limit cases use: the `generic` flag the restated size formula assumes is the plan's own"""
    smooth, prime, rejected = F.lds_limit_lengths()
    for n, generic in ((smooth, 0), (prime, 1), (rejected, 0)):
        assert _plan(n)[0].generic == generic, n
    assert F.generic_rows_lds(smooth)[0] <= F.KMAX_LDS < F.generic_rows_lds(rejected)[0]
