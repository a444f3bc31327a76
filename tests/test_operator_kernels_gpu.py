"""Every dispatch path of csrc/dense.hip, csrc/dst.hip and csrc/hadamard.hip on the MI355X against fp64 on the CPU: the whole case
tables of tests/dense_cases.py, tests/dst_cases.py and tests/hadamard_cases.py through the C entry points on guarded buffers -
including what the host emulation cannot tell or cannot run: the accumulator-to-row map of v_mfma_f32_32x32x2_f32 (the emulation
holds the kernel's own formula), the grouped Hadamard tiles with a partial last group at 256 compute units and the planes of
2^16 to 2^20 floats that are two-pass on any device.  The last test of each table prints the worst ratio of error to bound."""
import pytest
import torch

import dense_cases as DN
import dst_cases as DS
import hadamard_cases as HD

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
WORST = {"dense": {}, "dst": {}, "hadamard": {}}


@pytest.fixture(scope="module")
def dense():
    from deepinv_amd import hip
    from deepinv_amd.hip import dense as hdense

    return DN.Runner(hdense._l(), DEV, lambda: hip.stream_ptr(DEV))


@pytest.fixture(scope="module")
def dst():
    from deepinv_amd import hip
    from deepinv_amd.hip import dst as hdst

    return DS.Runner(hdst._l(), DEV, lambda: hip.stream_ptr(DEV), lambda n: hip.fft_plan(n, DEV))


@pytest.fixture(scope="module")
def hadamard():
    from deepinv_amd import hip
    from deepinv_amd.hip import hadamard as hhad

    return HD.Runner(hhad._l(), DEV, lambda: hip.stream_ptr(DEV), torch.cuda.get_device_properties(DEV).multi_processor_count)


def _summary(table):
    if not WORST[table]:          # the cases were deselected: nothing to report
        return
    cid, ratio = max(WORST[table].items(), key=lambda kv: kv[1])
    print(f"{table}: {len(WORST[table])} cases, worst error / bound {ratio:.3g} ({cid})")
    assert ratio <= 1.0


# ------------------------------------------------------------------ dense.hip
@pytest.mark.parametrize("case", DN.CASES, ids=lambda c: c.id)
def test_dense_path(dense, case):
    WORST["dense"][case.id] = DN.run_case(dense, case)


def test_dense_worst_ratio():
    _summary("dense")


# ------------------------------------------------------------------ dst.hip
@pytest.mark.parametrize("case", DS.BARE, ids=lambda c: c.id)
def test_dst1_path(dst, case):
    WORST["dst"][case.id] = DS.run_bare(dst, case)


@pytest.mark.parametrize("adjoint", [False, True], ids=["A", "At"])
@pytest.mark.parametrize("case", DS.STRUCTURED, ids=lambda c: c.id)
def test_structured_path(dst, case, adjoint):
    WORST["dst"][f"{case.id}-{'At' if adjoint else 'A'}"] = DS.run_structured(dst, case, adjoint)


def test_dst_rejections_write_nothing(dst):
    DS.run_rejections(dst)


def test_dst_worst_ratio():
    _summary("dst")


# ------------------------------------------------------------------ hadamard.hip
@pytest.mark.parametrize("case", HD.TABLE, ids=lambda c: c.id)
def test_hadamard_path(hadamard, case):
    worst = HD.run_case(hadamard, case)
    print(HD.report(case, worst))
    WORST["hadamard"][case.id] = max(ratio for ratio, _ in worst.values())


def test_hadamard_misaligned_operands_are_refused(hadamard):
    HD.run_misaligned(hadamard)


def test_hadamard_worst_ratio():
    _summary("hadamard")
