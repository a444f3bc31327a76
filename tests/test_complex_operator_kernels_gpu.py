"""Every dispatch path of csrc/cdense.hip and csrc/cstructured.hip (the structured operator and ptychography) on the MI355X, per
element against fp64 on the CPU: the whole case tables of tests/cdense_cases.py and tests/cplane_cases.py through the C entry
points on guarded buffers - including what the host emulation cannot tell or cannot run: the accumulator-to-row map and the
signs of the four v_mfma_f32_32x32x2_f32 of a complex multiply-accumulate (the emulation holds the kernel's own formula), the
dynamic-LDS opt-in of the planes above 48 KiB, the group rule at the device's compute-unit count and the cases the fiber
emulation takes too long for.  The last test of each table prints the case count and the worst ratio of error to bound."""
import pytest
import torch

import cdense_cases as CD
import cplane_cases as CP

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
WORST = {"cdense": {}, "cstructured": {}, "ptycho": {}}


@pytest.fixture(scope="module")
def cdense():
    from deepinv_amd import hip
    from deepinv_amd.hip import cdense as hcd

    return CD.Runner(hcd._l(), DEV, lambda: hip.stream_ptr(DEV))


@pytest.fixture(scope="module")
def plane():
    from deepinv_amd import hip
    from deepinv_amd.hip import cstructured as hcs
    from deepinv_amd.hip import ptycho as hpt

    hcs._l()
    return CP.Runner(hpt._l(), DEV, lambda: hip.stream_ptr(DEV), lambda n: hip.fft_plan(n, DEV),
                     torch.cuda.get_device_properties(DEV).multi_processor_count)


def _summary(table):
    if not WORST[table]:          # the cases were deselected: nothing to report
        return
    kinds = sorted({k for w in WORST[table].values() for k in w})
    for kind in kinds:
        cid, w = max(WORST[table].items(), key=lambda kv: kv[1].get(kind, 0.0))
        print(f"{table} {kind}: worst error / bound {w[kind]:.3g} ({cid})")
    cid, w = max(WORST[table].items(), key=lambda kv: max(kv[1].values()))
    ratio = max(w.values())
    print(f"{table}: {len(WORST[table])} cases, worst error / bound {ratio:.3g} ({cid})")
    assert ratio <= 1.0


# ------------------------------------------------------------------ cdense.hip
@pytest.mark.parametrize("case", CD.CASES, ids=lambda c: c.id)
def test_cdense_path(cdense, case):
    WORST["cdense"][case.id] = CD.run_case(cdense, case)


def test_cdense_rejections_write_nothing(cdense):
    CD.run_rejections(cdense)


def test_cdense_worst_ratio():
    _summary("cdense")


# ------------------------------------------------------------------ cstructured.hip: the structured operator
@pytest.mark.parametrize("adjoint", [False, True], ids=["B", "Bh"])
@pytest.mark.parametrize("case", CP.STRUCTURED, ids=lambda c: c.id)
def test_cstructured_path(plane, case, adjoint):
    WORST["cstructured"][f"{case.id}-{'Bh' if adjoint else 'B'}"] = CP.run_structured(plane, case, adjoint)


@pytest.mark.parametrize("adjoint", [False, True], ids=["B", "Bh"])
@pytest.mark.parametrize("case", CP.EXACT, ids=lambda c: c.id)
def test_cstructured_exact(plane, case, adjoint):
    CP.run_exact(plane, case, adjoint)


def test_cstructured_rejections_write_nothing(plane):
    CP.run_structured_rejections(plane)


def test_cstructured_bound_is_the_derived_one(plane):
    """`per` of the runner is that of phase_retrieval_cases.derived_fft_bound"""
    import phase_retrieval_cases as PC

    for H, W in ((12, 15), (7, 49), (99, 99), (1, 64), (3, 2500)):
        assert plane.per(H, W) * CP.U == PC.derived_fft_bound(H, W, 1, 0, DEV)


def test_cstructured_worst_ratio():
    _summary("cstructured")


# ------------------------------------------------------------------ cstructured.hip: ptychography
@pytest.mark.parametrize("case", CP.PTYCHO, ids=lambda c: c.id)
def test_ptycho_path(plane, case):
    WORST["ptycho"][case.id] = CP.run_ptycho(plane, case)


def test_ptycho_rejections_write_nothing(plane):
    CP.run_ptycho_rejections(plane)


def test_ptycho_workspace_restated(plane):
    """dinv_ptycho_workspace_bytes against the restated group rule at the device's compute-unit count"""
    CP.run_workspace_scan(plane)


def test_ptycho_worst_ratio():
    _summary("ptycho")
