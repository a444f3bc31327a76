"""The Gaussian-mixture kernels of csrc/patch_gmm.hpp on the host emulation of the kernel sources (tests/emu): the cases of
tests/gmm_cases.py that the fiber emulation finishes quickly, through the C entry points on guarded buffers, exactly and against
fp64.  Every call also asserts, through the emulation's launch log, what the restated dispatch rules predict: the instantiation
gmm_score_kernel<IMAGE, NP>, and for a step the estimate and aggregate kernels after it - three launches.
tests/test_gmm_kernels_gpu.py runs the whole table on the device."""
import ctypes

import pytest

import emu_lib as E
import gmm_cases as GC


@pytest.fixture(scope="module")
def runner():
    l = E.lib()
    log = lambda: [l.dinv_emu_launch_log_name(i).decode() for i in range(l.dinv_emu_launch_log_count())]
    return GC.Runner(l, "cpu", lambda: ctypes.c_void_p(0), reset=l.dinv_emu_launch_log_reset, launches=log)


@pytest.mark.parametrize("case", [c for c in GC.CASES if c.emu], ids=lambda c: c.id)
def test_gmm_path_emulated(runner, case):
    GC.run_case(runner, case)


def test_ties_go_to_the_lowest_index(runner):
    GC.run_ties(runner)


def test_refusals_and_empty_batch(runner):
    GC.run_refusals(runner)


def test_case_table_reaches_every_path():
    """the table itself: both operand sources, every NP of each, the three epilogues and the step (run_case runs all of them for
    every case that has an r), d on both sides of the MFMA k step and of the row tile, K d on both sides of a multiple of 32,
    patches per row and rows of patches on both sides of the LDS tile, one patch, one row, several images with several r, colour,
    non-square images, the unregularised model and every rows-mode N edge"""
    T = GC.CASES
    img, rows = [c for c in T if c.image], [c for c in T if not c.image]
    for group in (img, rows):
        assert {GC.patch_tiles(c) for c in group} == {1, 2, 4}
    assert {GC.score_kernel(c) for c in T} == {f"(gmm_score_kernel<{m}, {n}>)" for m in ("true", "false") for n in (1, 2, 4)}
    assert any(c.r is not None for c in img), "no case runs the step"
    assert {9, 16, 27, 36, 108} <= {c.d for c in T} and {9, 16, 27, 36, 108} <= {c.d for c in img}
    assert any(c.d % 2 for c in T) and any(c.d % 2 == 0 for c in T) and any(c.d % 32 for c in T)
    assert {1, 3, 8, 200} <= {c.K for c in T}
    assert any((c.K * c.d) % 32 == 0 for c in T) and any((c.K * c.d) % 32 for c in T) and any(c.K * c.d < 32 for c in T)
    assert {1, 31, 32, 33} <= {c.PW for c in img}
    np1 = [c for c in img if GC.patch_tiles(c) == 1]
    assert {3, 4, 5} <= {c.PH for c in np1}, "rows of patches one short of, at and one past the NP = 1 tile"
    assert any(c.PH == 1 and c.PW > 1 for c in img) and any(c.PH == 1 and c.PW == 1 for c in img)
    assert {1, 3} <= {c.B for c in img} and any(c.r and len(set(c.r)) == 3 and c.B == 3 for c in img)
    assert {1, 3} <= {c.C for c in img} and any(c.H != c.W for c in img)
    assert any(c.r is None for c in img) and any(c.r is None for c in rows) and any(c.r for c in rows)
    assert {1, 31, 33, 129} <= {c.N for c in rows}
    for c in T:
        assert GC.lds_bytes(c) <= GC.MAX_LDS
    # dynamic LDS on both sides of the default limit of a launch (the opt-in branch of the launcher), the larger side also above
    # the 64 KB at which the emulation enforces the opt-in; the largest d the limits name
    assert any(GC.lds_bytes(c) <= GC.DEFAULT_LDS for c in T) and any(GC.lds_bytes(c) > 64 * 1024 and c.emu for c in T)
    assert 192 in {c.d for c in img}
    # the emulation runs every path but the large-grid ones
    assert {GC.patch_tiles(c) for c in T if c.emu} == {1}
