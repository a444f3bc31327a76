"""Every path of csrc/tv.hip, csrc/tgv.hip and csrc/elementwise.hip on the MI355X, per element against fp64 on the CPU: the whole
case tables of tests/variational_cases.py and tests/loop_algebra_cases.py through the C entry points of the product library on
guarded buffers - including what the host emulation does not run: the second pass of every grid-stride loop with a ragged end
(above 2048 x 256 pixels, above 256 x 1024 pixels per sample of dinv_tv_fn, above the workgroup caps of the loop algebra), and
the device's own division, square root and expf.  The last test of each table prints the worst ratio of error to bound."""
import pytest
import torch

import loop_algebra_cases as LA
import variational_cases as VC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
WORST = {"variational": {}, "loop-algebra": {}}


@pytest.fixture(scope="module")
def variational():
    from deepinv_amd import hip
    from deepinv_amd.hip import tgv as htgv
    from deepinv_amd.hip import tv as htv

    assert htv._l() is htgv._l()
    return VC.Runner(htv._l(), DEV, lambda: hip.stream_ptr(DEV))


@pytest.fixture(scope="module")
def loop_algebra():
    from deepinv_amd import hip
    from deepinv_amd.hip import elementwise as hew

    return LA.Runner(hew._l(), DEV, lambda: hip.stream_ptr(DEV))


def _summary(table):
    if not WORST[table]:          # the cases were deselected: nothing to report
        return
    cid, ratio = max(WORST[table].items(), key=lambda kv: kv[1])
    print(f"{table}: {len(WORST[table])} cases, worst error / bound {ratio:.3g} ({cid})")
    assert ratio <= 1.0


# ------------------------------------------------------------------ tv.hip, tgv.hip
@pytest.mark.parametrize("case", VC.TABLE, ids=lambda c: c.id)
def test_variational_path(variational, case):
    WORST["variational"][case.id] = VC.run_case(variational, case)


def test_variational_rejections_write_nothing(variational):
    VC.run_rejections(variational)


def test_variational_worst_ratio():
    _summary("variational")


# ------------------------------------------------------------------ elementwise.hip
@pytest.mark.parametrize("case", LA.TABLE, ids=lambda c: c.id)
def test_loop_algebra_path(loop_algebra, case):
    WORST["loop-algebra"][case.id] = LA.run_case(loop_algebra, case)


def test_loop_algebra_rejections_write_nothing(loop_algebra):
    LA.run_rejections(loop_algebra)


def test_loop_algebra_worst_ratio():
    _summary("loop-algebra")
