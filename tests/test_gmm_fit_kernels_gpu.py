"""Every path of the EM kernels of the Gaussian mixture (csrc/patch_gmm.hpp POSTERIOR epilogue, csrc/gmm_moments.hpp) on the
MI355X, exactly and against fp64 on the CPU: the whole case table of tests/gmm_fit_cases.py through the C entry points on guarded
buffers - including what the host emulation cannot tell or does not run: the accumulator-to-row map of v_mfma_f32_32x32x2_f32, the
device's logf / expf against the ulp counts the bounds allow, the largest shapes and the POSTERIOR epilogue with two and four patch
tiles per wave.  The last test prints the worst ratio of error to bound."""
import pytest
import torch

import gmm_cases as GC
import gmm_fit_cases as FC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
WORST = {}


@pytest.fixture(scope="module")
def runner():
    from deepinv_amd import hip
    from deepinv_amd.hip import gmm as hgmm

    return GC.Runner(hgmm._l(), DEV, lambda: hip.stream_ptr(DEV))


@pytest.mark.parametrize("case", FC.CASES, ids=lambda c: c.id)
def test_gmm_fit_path(runner, case):
    WORST[case.id] = FC.run_case(runner, case)


def test_far_component_gets_exactly_zero(runner):
    FC.run_underflow(runner)


def test_posterior_with_two_and_four_patch_tiles(runner):
    FC.run_patch_tiles(runner)


def test_refusals_and_empty_batch(runner):
    FC.run_refusals(runner)


def test_gmm_fit_worst_ratio():
    if not WORST:          # the cases were deselected: nothing to report
        return
    flat = {(cid, name): v for cid, w in WORST.items() for name, v in w.items()}
    (cid, name), ratio = max(flat.items(), key=lambda kv: kv[1])
    print(f"gmm fit: {len(WORST)} cases, worst error / bound {ratio:.3g} ({name} of {cid})")
    assert ratio <= 1.0
