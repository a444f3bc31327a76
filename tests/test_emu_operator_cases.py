"""The three real-valued measurement-operator kernels - csrc/dense.hip (CompressedSensing), csrc/dst.hip (dst1, StructuredRandom)
and csrc/hadamard.hip (SinglePixelCamera) - on the host emulation of the kernel sources (tests/emu), against fp64: the cases of
tests/dense_cases.py, tests/dst_cases.py and tests/hadamard_cases.py that the fiber emulation finishes quickly, through the C entry
points on guarded buffers.  Every call also asserts, through the emulation's launch log, what the restated dispatch rules predict:
dense_partial_kernel<NI> and whether dense_reduce_kernel follows it, one dst_tile_kernel launch, and the one, two or three
hadamard_tile_kernel launches with their block sizes.  tests/test_operator_kernels_gpu.py runs the whole tables on the device."""
import ctypes

import pytest
import torch

import dense_cases as DN
import dst_cases as DS
import emu_lib as E
import hadamard_cases as HD


def _log(l, instances):
    name = l.dinv_emu_launch_log_instance if instances else l.dinv_emu_launch_log_name
    return lambda: [name(i).decode() for i in range(l.dinv_emu_launch_log_count())]


def _stream():
    return ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def dense():
    l = E.lib()
    return DN.Runner(l, "cpu", _stream, reset=l.dinv_emu_launch_log_reset, launches=_log(l, False))


@pytest.fixture(scope="module")
def dst():
    l = E.lib()

    def fft_plan(n):
        plan, table = E.fft_plan(n)
        return plan, torch.from_numpy(table)

    plans = {}
    return DS.Runner(l, "cpu", _stream, lambda n: plans.setdefault(n, fft_plan(n)), reset=l.dinv_emu_launch_log_reset,
                     launches=_log(l, True))


@pytest.fixture(scope="module")
def hadamard():
    l = E.lib()
    return HD.Runner(l, "cpu", _stream, HD.EMU_CUS, reset=l.dinv_emu_launch_log_reset, launches=_log(l, True))


# ------------------------------------------------------------------ dense.hip
@pytest.mark.parametrize("case", [c for c in DN.CASES if c.emu], ids=lambda c: c.id)
def test_dense_path_emulated(dense, case):
    DN.run_case(dense, case)


def test_dense_table_reaches_every_path():
    """the table itself: every NI, one to three row chunks with a ragged last one, both load paths of both operands in both
    layouts, one slice and several, and every K edge of the 32-k block"""
    C = DN.CASES
    assert {(DN.accumulators(c.I), DN.row_chunks(c.I)) for c in C} == {(1, 1), (2, 1), (4, 1), (4, 2), (4, 3)}
    for ni in (1, 2, 4):
        mine = [c for c in C if DN.accumulators(c.I) == ni]
        assert {c.transposed for c in mine} == {0, 1}
        assert {DN.split_k(c.I, c.K, c.R)[0] > 1 for c in mine} == {False, True}
        assert {DN.vector_loads(c)[0] for c in mine} == {False, True}
        assert {DN.vector_loads(c)[1] for c in mine if not c.transposed} == {False, True}
        assert any(c.off for c in mine) and {c.pad for c in mine} >= {0, 3, 4}
        assert any(c.R % 32 for c in mine) and any(c.I % 32 for c in mine)
    assert {c.K for c in C} == {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 1000, 1024}
    assert {c.I for c in C} == {1, 4, 5, 31, 32, 33, 64, 65, 128, 129, 257} and {c.R for c in C} == {1, 31, 32, 33, 70}
    # a short last slice and a full one
    assert any(c.K % DN.split_k(c.I, c.K, c.R)[1] for c in C if DN.split_k(c.I, c.K, c.R)[0] > 1)
    assert any(c.K % DN.split_k(c.I, c.K, c.R)[1] == 0 for c in C if DN.split_k(c.I, c.K, c.R)[0] > 1)


# ------------------------------------------------------------------ dst.hip
@pytest.mark.parametrize("case", [c for c in DS.BARE if c.emu], ids=lambda c: c.id)
def test_dst1_path_emulated(dst, case):
    DS.run_bare(dst, case)


@pytest.mark.parametrize("adjoint", [False, True], ids=["A", "At"])
@pytest.mark.parametrize("case", [c for c in DS.STRUCTURED if c.emu], ids=lambda c: c.id)
def test_structured_path_emulated(dst, case, adjoint):
    DS.run_structured(dst, case, adjoint)


def test_dst_rejections_write_nothing(dst):
    DS.run_rejections(dst)


def test_dst_table_reaches_every_path():
    """the table itself: the lengths around the 256-thread line group, every `lines` the issue names, and the zero fill that
    strides its grid"""
    assert {c.n for c in DS.BARE} == {1, 2, 3, 12, 31, 100, 255, 256, 257, 1024}
    assert {c.rows for c in DS.BARE} >= {1, 2, 3, 5, 513, 1025, 16385}
    assert {c.lines for c in DS.BARE} == {1, 2, 3, 32}
    assert any(c.n == 255 and c.rows > 2 * 256 * 3 and c.lines == 3 for c in DS.BARE)
    assert any(c.rows % (2 * c.lines) not in (0, 2 * c.lines - 1) and c.lines == 32 for c in DS.BARE)
    assert any(c.inplace and c.lines > 1 for c in DS.BARE)
    assert {c.layers for c in DS.STRUCTURED} >= {0.5, 1, 1.5, 2, 3}
    big = next(c for c in DS.STRUCTURED if "zero-fill-strides" in c.what)
    zeros = big.planes * (big.hout - big.hin) * big.wout
    assert zeros > DS.workgroups(big.planes * big.hin, big.wout) * DS.THREADS and big.lines == 2


# ------------------------------------------------------------------ hadamard.hip
@pytest.mark.parametrize("case", [c for c in HD.TABLE if c.emu], ids=lambda c: c.id)
def test_hadamard_path_emulated(hadamard, case):
    print(HD.report(case, HD.run_case(hadamard, case)))


def test_hadamard_misaligned_operands_are_refused(hadamard):
    HD.run_misaligned(hadamard)


def test_hadamard_form_at_256_compute_units():
    """the restated choice of form for the cases only the device runs, at the compute-unit count of an MI355X: what each is named for"""
    for c in HD.TABLE:
        want = c.expect.get(256)
        if want:
            planes, l = (c.P, HD.bits(c.H, c.W)) if c.plain or c.masks else (c.P * c.H, c.W.bit_length() - 1)
            f = HD.form(planes, l, l, c.c, 256)
            assert {k: f[k] for k in want} == want, c.id
    # the forced forms stay two-pass whatever the count; a resident plane is one launch, an operator with two transforms three
    assert HD.form(1, 16, 16, 0, 256, True)["tiles"] == [4, 4, 4] and HD.form(3, 20, 20, 0, 256)["tiles"] == [192, 192]
