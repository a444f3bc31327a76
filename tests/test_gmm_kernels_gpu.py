"""Every path of the Gaussian-mixture kernels of csrc/patch_gmm.hpp on the MI355X, exactly and against fp64 on the CPU: the whole
case table of tests/gmm_cases.py through the C entry points on guarded buffers - including what the host emulation cannot tell or
does not run: the accumulator-to-row map of v_mfma_f32_32x32x2_f32 (the emulation holds the kernel's own formula), the device's
logf / expf against the ulp counts the bounds allow, and the instantiations with two and four patch tiles per wave, which need
256 workgroups.  The last test prints the worst ratio of error to bound."""
import pytest
import torch

import gmm_cases as GC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
WORST = {}


@pytest.fixture(scope="module")
def runner():
    from deepinv_amd import hip
    from deepinv_amd.hip import gmm as hgmm

    return GC.Runner(hgmm._l(), DEV, lambda: hip.stream_ptr(DEV))


@pytest.mark.parametrize("case", GC.CASES, ids=lambda c: c.id)
def test_gmm_path(runner, case):
    WORST[case.id] = GC.run_case(runner, case)


def test_ties_go_to_the_lowest_index(runner):
    GC.run_ties(runner)


def test_refusals_and_empty_batch(runner):
    GC.run_refusals(runner)


def test_gmm_worst_ratio():
    if not WORST:          # the cases were deselected: nothing to report
        return
    flat = {(cid, name): v for cid, w in WORST.items() for name, v in w.items()}
    (cid, name), ratio = max(flat.items(), key=lambda kv: kv[1])
    print(f"gmm: {len(WORST)} cases, worst error / bound {ratio:.3g} ({name} of {cid})")
    assert ratio <= 1.0
