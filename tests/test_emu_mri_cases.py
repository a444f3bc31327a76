"""The MRI pipelines of csrc/mri.hip and csrc/mri_wave.hpp on the host emulation of the kernel sources (tests/emu), against
complex128: every case of tests/mri_cases.py that is not a grid case.  Every call asserts, through the emulation's launch log,
the instantiations mri_cases.expected_kernels restates from the dispatch rules.  tests/test_mri_gpu.py runs the whole table on
the device."""
import ctypes

import pytest
import torch

import emu_lib as E
import mri_cases as K


@pytest.fixture(scope="module")
def runner():
    l = E.lib()

    def launches():
        return [l.dinv_emu_launch_log_instance(i).decode() for i in range(l.dinv_emu_launch_log_count())]

    def fft_plan(n):
        plan, table = E.fft_plan(n)
        return plan, torch.from_numpy(table)

    return K.Runner(l, "cpu", lambda: ctypes.c_void_p(0), fft_plan, reset=l.dinv_emu_launch_log_reset, launches=launches)


@pytest.mark.parametrize("case", [c for c in K.CASES if c.emu], ids=lambda c: c.id)
def test_mri_path_emulated(runner, case):
    errs = K.run_case(runner, case)
    print(f"{case.id}: " + ", ".join(f"{op} {K.family(case, i)} {errs[op]:.3g}" for i, op in enumerate(("A", "AT", "ATA"))
                                      if op in errs) + (f", A^T A vs A^T(A x) {errs['chain']:.3g}" if "chain" in errs else ""))


def test_rejections_write_nothing(runner):
    K.run_rejections(runner)


def test_empty_batch_launches_nothing(runner):
    K.run_empty(runner)


def test_case_table_reaches_every_path():
    """the table itself: every wave R and width, per-sample maps on the wave pipelines, the natural B = 15 / 16 threshold, every
    expand first axis, every rows_normal / rows_combine_static width, the coil counts and batches of both combine passes, the
    width limits, a grid case for every capped launcher"""
    emu = [c for c in K.CASES if c.emu]
    assert {c.vol for c in emu if K.wave2d_ok(c, 0)} == {(h, w) for h in K.WAVE_SIZES for w in K.WAVE_SIZES}
    wave_adj = [c for c in emu if K.wave2d_ok(c, 1)]
    assert {c.maps for c in wave_adj} == {"none", "shared", "per"}
    assert any(c.hook == 0 and c.B == 16 for c in wave_adj)
    assert any(c.B == 15 and c.vol == (256, 256) and not K.wave2d_ok(c, 1) for c in emu)
    stat = [c for c in emu if K.all_static(c)]
    assert {c.vol[0] for c in stat if K.expand_ok(c) and len(c.vol) == 2} == {32, 64, 128, 256, 320, 512}
    assert any(K.expand_ok(c) and len(c.vol) == 3 for c in stat)
    for first in (True, False):
        assert {c.vol[-1] for c in stat if K.normal_ok(c) and K.expand_ok(c) == first} == set(K.STATIC_ROWS)
    comb8 = [c for c in stat if K.expand_ok(c)]
    assert {c.N for c in comb8} >= {1, 7, 8, 9, 16, 17} and {c.B for c in comb8} >= {1, 4, 5, 9}
    assert {c.maps for c in comb8} == {"none", "shared", "per"} and {K.combine_cached(c) for c in comb8} == {True, False}
    inv16 = [c for c in stat if not K.expand_ok(c)]
    assert {c.N for c in inv16} >= {1, 2, 3, 4, 5} and {c.maps for c in inv16} == {"none", "shared", "per"}
    gen = [c for c in emu if not K.all_static(c)]
    assert {c.vol[-1] for c in gen} >= set(K.STATIC_ROWS) | {16, 32}
    assert any(c.vol[-1] % 2 and c.vol[-1] not in K.STATIC for c in gen) and any(len(c.vol) == 3 and c.vol[1] not in K.STATIC
                                                                                  for c in gen)
    fams = {K.family(c, op) for c in emu if c.kind == "op" for op in (0, 1, 2) if op < 2 or K.normal_ok(c) or K.wave2d_ok(c, 2)}
    assert fams == set(K.BOUNDS)
    lim = K.width_limits()
    widths = {c.vol[-1]: c.kind for c in emu if len(c.vol) == 2 and c.vol[0] == 2}
    for g in (True, False):
        assert widths[lim[("combine", g)][0]] == widths[lim[("combine", g)][1]] == widths[lim[("rows", g)][0]] == "op"
        assert widths[lim[("rows", g)][1]] == "reject"
    # device-only grid cases: past each launcher's cap
    caps = {"expand blocks": 4 * K.KMAX_GRID, "combine_inv tiles": 4 * K.KMAX_GRID, "rows_normal tiles": 4 * K.KMAX_GRID,
            "rows tiles": K.KMAX_GRID, "cols tiles": K.KMAX_GRID, "combine_static tiles": K.KMAX_GRID,
            "rows_dif waves": K.RESIDENT_WAVES, "cols64 waves": K.RESIDENT_WAVES, "cols64_combine waves": K.RESIDENT_WAVES,
            "rows_combine waves": K.RESIDENT_WAVES}
    for key, cap in caps.items():
        assert any(K.grid_facts(c).get(key, 0) > cap for c in K.CASES if not c.emu), key
