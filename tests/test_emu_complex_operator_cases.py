"""The complex measurement-operator kernels - csrc/cdense.hip (RandomPhaseRetrieval) and csrc/cstructured.hip
(StructuredRandomPhaseRetrieval, Ptychography) - on the host emulation of the kernel sources (tests/emu), per element against
fp64: the cases of tests/cdense_cases.py and tests/cplane_cases.py that the fiber emulation finishes quickly, through the C entry
points on guarded buffers.  Every call also asserts, through the emulation's launch log, what the restated dispatch rules predict:
cdense_partial_kernel<NI> and whether cdense_reduce_kernel follows it, one cstructured_plane_kernel launch, and the instance
ptycho_kernel<OP, ACC> with ptycho_reduce_kernel if and only if a call has several groups.  The tables' self-tests and the
host-only scans of the restated rules live here too.  tests/test_complex_operator_kernels_gpu.py runs the whole tables on the
device."""
import ctypes

import pytest
import torch

import cdense_cases as CD
import cplane_cases as CP
import emu_lib as E


def _log(l, instances):
    name = l.dinv_emu_launch_log_instance if instances else l.dinv_emu_launch_log_name
    return lambda: [name(i).decode() for i in range(l.dinv_emu_launch_log_count())]


def _stream():
    return ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def cdense():
    l = E.lib()
    return CD.Runner(l, "cpu", _stream, reset=l.dinv_emu_launch_log_reset, launches=_log(l, False))


@pytest.fixture(scope="module")
def plane():
    l = E.lib()

    def fft_plan(n):
        plan, table = E.fft_plan(n)
        return plan, torch.from_numpy(table)

    plans = {}
    return CP.Runner(l, "cpu", _stream, lambda n: plans.setdefault(n, fft_plan(n)), CP.EMU_CUS, reset=l.dinv_emu_launch_log_reset,
                     launches=_log(l, True))


# ------------------------------------------------------------------ cdense.hip
@pytest.mark.parametrize("case", [c for c in CD.CASES if c.emu], ids=lambda c: c.id)
def test_cdense_path_emulated(cdense, case):
    CD.run_case(cdense, case)


def test_cdense_rejections_write_nothing(cdense):
    CD.run_rejections(cdense)


def test_cdense_table_reaches_every_path():
    """the table itself: every NI with one to three row chunks, one slice and several for each NI, a short and a full last slice,
    both load paths of both operands, all four forms and every edge of the 16-k block"""
    C = CD.CASES
    assert {(CD.accumulators(c.I), CD.row_chunks(c.I)) for c in C} == {(1, 1), (2, 1), (4, 1), (4, 2), (4, 3)}
    for ni in (1, 2, 4):
        mine = [c for c in C if CD.accumulators(c.I) == ni]
        assert {(c.transposed, c.conj) for c in mine} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert {CD.split_k(c.I, c.K, c.R)[0] > 1 for c in mine} == {False, True}
        assert {CD.vector_loads(c)[0] for c in mine} == {False, True}
        assert {CD.vector_loads(c)[1] for c in mine if not c.transposed} == {False, True}
        assert any(c.off for c in mine) and {c.pad for c in mine} >= {0, 1, 3, 4}
        assert any(c.R % 32 for c in mine) and any(c.I % 32 for c in mine)
        # ldm = K + 1 with K odd: the 16-byte loads of M stay on and the last 8 of a row is short
        assert any(c.pad == 1 and c.K % 2 and not c.transposed and CD.vector_loads(c)[1] and c.K % 8 == 7 for c in mine)
    assert {c.K for c in C} >= {1, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 97, 1000, 1024}
    # 16-byte loads of `in` with a short last 8: K even and no multiple of 8
    assert {CD.accumulators(c.I) for c in C if CD.vector_loads(c)[0] and c.K % 8} == {1, 2, 4}
    assert {c.I for c in C} == {1, 4, 5, 8, 9, 31, 32, 33, 64, 65, 128, 129, 257} and {c.R for c in C} == {1, 31, 32, 33, 70}
    # a short last slice and a full one
    several = [c for c in C if CD.split_k(c.I, c.K, c.R)[0] > 1]
    assert any(c.K % CD.split_k(c.I, c.K, c.R)[1] for c in several)
    assert any(c.K % CD.split_k(c.I, c.K, c.R)[1] == 0 for c in several)
    # the min_k = 2 I rule, which dense.hip does not have: K = 17 is two slices of 16 at I = 8 and one of 32 at I = 9
    assert CD.split_k(8, 17, 70) == (2, 16) and CD.split_k(9, 17, 31) == (1, 32) and CD.split_k(9, 33, 32) == (2, 32)
    assert any((c.I, c.K) == (8, 17) for c in C) and any((c.I, c.K) == (9, 17) for c in C)
    assert CD.split_k(32, 64, 70) == (1, 64) and CD.split_k(32, 97, 70) == (2, 64)


def test_cdense_exclusion_cap_holds_for_every_seed():
    """the elements the AMPLITUDE bound does not cover (|Z| < 8 d) are at most 1 % of every case: a condition on the fp64 data"""
    worst = max((CD.excluded_fraction(c), c.id) for c in CD.CASES)
    print(f"largest excluded fraction {worst[0]:.3%} ({worst[1]})")
    assert worst[0] <= 0.01, worst


def test_cdense_workspace_restated(cdense):
    for I in (1, 4, 5, 8, 9, 31, 32, 33, 64, 65, 128, 129, 257, 1000):
        for K in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 128, 129, 1000, 1024, 4096, 100000):
            for R in (1, 31, 32, 33, 70, 1024, 40000):
                assert cdense.workspace_bytes(I, K, R) == CD.workspace_bytes(I, K, R), (I, K, R)
    assert cdense.workspace_bytes(0, 8, 8) == 0


# ------------------------------------------------------------------ cstructured.hip: the structured operator
@pytest.mark.parametrize("adjoint", [False, True], ids=["B", "Bh"])
@pytest.mark.parametrize("case", [c for c in CP.STRUCTURED if c.emu], ids=lambda c: c.id)
def test_cstructured_path_emulated(plane, case, adjoint):
    CP.run_structured(plane, case, adjoint)


@pytest.mark.parametrize("adjoint", [False, True], ids=["B", "Bh"])
@pytest.mark.parametrize("case", CP.EXACT, ids=lambda c: c.id)
def test_cstructured_exact_emulated(plane, case, adjoint):
    CP.run_exact(plane, case, adjoint)


def test_cstructured_rejections_write_nothing(plane):
    CP.run_structured_rejections(plane)


def test_cstructured_fits_scan(plane):
    """host only: the restated `fits` is dinv_cstructured_fits on every plane of up to 11000 elements, a plane that fits has at
    most 512 x 20 elements (what dinv_ptycho_apply requires and the Python layer does not check before it takes the fused path),
    and the largest fused square is the 99 of the existing boundary tests"""
    CP.run_fits_scan(plane)


def test_cstructured_table_reaches_every_path():
    CP.check_structured_table()


# ------------------------------------------------------------------ cstructured.hip: ptychography
@pytest.mark.parametrize("case", [c for c in CP.PTYCHO if c.emu], ids=lambda c: c.id)
def test_ptycho_path_emulated(plane, case):
    CP.run_ptycho(plane, case)


def test_ptycho_rejections_write_nothing(plane):
    CP.run_ptycho_rejections(plane)


def test_ptycho_workspace_restated(plane):
    """host only: dinv_ptycho_workspace_bytes against the restated group rule at the emulation's 16 compute units, automatic and
    forced, over batches that take the per_cu rule to both of its values and G above 1"""
    CP.run_workspace_scan(plane)


def test_ptycho_table_reaches_every_path():
    CP.check_ptycho_table()


def test_ptycho_groups_at_256_compute_units():
    """the restated group rule at the compute-unit count of an MI355X, for the cases only the device runs"""
    CP.check_groups_at_256()
