"""The EM kernels of the Gaussian mixture (csrc/patch_gmm.hpp POSTERIOR epilogue, csrc/gmm_moments.hpp) on the host emulation of
the kernel sources (tests/emu): the cases of tests/gmm_fit_cases.py that the fiber emulation finishes quickly, through the C entry
points on guarded buffers, exactly and against fp64.  Every call also asserts, through the emulation's launch log, what the
restated dispatch rules predict: one score-kernel launch for the posterior, gmm_moments_kernel<NJ> and the reduce for the moments -
three launches per batch.  tests/test_gmm_fit_kernels_gpu.py runs the whole table on the device."""
import ctypes

import pytest

import emu_lib as E
import gmm_cases as GC
import gmm_fit_cases as FC


@pytest.fixture(scope="module")
def runner():
    l = E.lib()
    log = lambda: [l.dinv_emu_launch_log_name(i).decode() for i in range(l.dinv_emu_launch_log_count())]
    return GC.Runner(l, "cpu", lambda: ctypes.c_void_p(0), reset=l.dinv_emu_launch_log_reset, launches=log)


@pytest.mark.parametrize("case", [c for c in FC.CASES if c.emu], ids=lambda c: c.id)
def test_gmm_fit_path_emulated(runner, case):
    FC.run_case(runner, case)


def test_far_component_gets_exactly_zero(runner):
    FC.run_underflow(runner)


def test_refusals_and_empty_batch(runner):
    FC.run_refusals(runner)


def test_case_table_reaches_every_path():
    """the table itself: d on both sides of the MFMA k step, of the dp padding and of d + 1 against the output tile of 32, every
    accumulator count and every split of a tile row over waves, the K and N edges, forced chunks one row short of, at and one row
    past a chunk and three chunks with a ragged last one, automatic chunking with one and with several chunks"""
    T = FC.CASES
    assert {1, 9, 16, 36, 37, 108, 192} <= {c.d for c in T}
    assert any(c.d % 2 for c in T) and any(c.d % 4 for c in T) and any(c.d % 4 == 0 for c in T)
    assert {31, 32} <= {c.d for c in T}, "d + 1 exactly one tile and one past it"
    assert {1, 3, 8, 200} <= {c.K for c in T}
    assert {1, 31, 32, 33, 129} <= {c.N for c in T}
    forced = [c for c in T if c.chunk_rows]
    assert {c.N - c.chunk_rows for c in forced if FC.chunks(c) <= 2} >= {-1, 0, 1}
    assert any(FC.chunks(c) == 3 and c.N % c.chunk_rows for c in forced), "three chunks, the last ragged"
    auto = [c for c in T if not c.chunk_rows]
    assert any(FC.chunks(c) == 1 for c in auto) and any(FC.chunks(c) > 1 for c in auto)
    # every output-block split: one, two and four accumulators; a tile row that fits one wave and one split over two
    assert {FC.accumulators(c) for c in T} == {1, 2, 4} == {FC.accumulators(c) for c in T if c.emu}
    assert {FC.tiles(c) for c in T} >= {1, 2, 4, 7}
    assert any(FC.tiles(c) > FC.accumulators(c) and c.emu for c in T), "a tile row split over waves"
    assert [FC.waves_per_chunk(FC.Case(1, d, 1)) for d in (9, 36, 108, 192)] == [1, 2, 4, 10]
    assert [FC.blocks(FC.Case(1, d, 1)) for d in (9, 36, 108, 192)] == [1, 3, 10, 28]
    for c in T:
        assert c.N <= 400 and (c.chunk_rows % FC.ROWS == 0)
        assert GC.patch_tiles(c.score_case) == 1
    # the largest shapes are GPU only
    assert max(c.K * c.d for c in T if c.emu) < max(c.K * c.d for c in T)
