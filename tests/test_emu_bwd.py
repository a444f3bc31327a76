"""The training kernels (the weight gradients, the bias gradient and the ReLU backward of csrc/drunet_bwd.hip; the data
gradients = the forward kernels on flipped / transposed packs with their gate and residual epilogues, called as
models/drunet_train.py and models/drunet3d.py call them) on the host emulation of the kernel sources (tests/emu): the part of the
case table of tests/bwd_cases.py that the fiber emulation finishes in seconds.  Every `int` and `wide` run must equal the fp64
reference bit for bit, every `randn` run stays inside its derived ceiling.  tests/test_bwd_gpu.py runs the whole table on the device.
`python -m pytest tests/test_emu_bwd.py -s` prints every randn run's worst fraction of its ceiling."""
import pytest

import bwd_cases as C
from emu_backend import emu_backend


@pytest.fixture(scope="module")
def be():
    with emu_backend():
        yield C.Backend("cpu")


@pytest.mark.parametrize("case,cls", C.items(emu=True), ids=C.item_id)
def test_bwd_case_emulated(be, case, cls):
    C.run_case(be, case, cls)


def test_case_table_reaches_every_regime():
    """the table itself, through the restated launcher arithmetic: one, several and more than 16 slices (the second round of the
    reduction) with an empty last slice, both tile widths of both weight-gradient kernels, more than one bias slice and reduce
    block, the grid-stride pass of the ReLU kernel on the device, every data-gradient branch - and the emulation keeps all of it
    except what is marked gpu_only"""
    def nparts(c):
        return C.part_count(C.padded(c.B * (c.D + 2 if c.D else 1), c.H, c.W)[3], c.M, c.N)

    for kind in ("wgrad3", "wgrad2"):
        for emu in (True, False):
            cs = [c for c in C.CASES if c.kind == kind and not (emu and c.gpu_only)]
            thin = {c.M <= 16 and c.N <= 16 for c in cs}
            assert thin == {True, False}, kind
            n = sorted({nparts(c) for c in cs})
            assert n[0] == 1 and any(1 < v <= 16 for v in n) and n[-1] > 16, (kind, n)
    w3 = [c for c in C.CASES if c.kind == "wgrad3"]
    assert any(nparts(c) == 128 and c.gpu_only for c in w3)                        # the slice count saturated at np / 512
    assert any(nparts(c) > 1 for c in C.CASES if c.kind == "wgrad3x3x3") and any(nparts(c) > 1 for c in C.CASES if c.kind == "wgrad2x2x2")
    assert {c.D for c in C.CASES if c.kind == "wgrad2x2x2"} >= {1, 3, 4} and any(c.D == 1 for c in C.CASES if c.kind == "wgrad3x3x3")
    bias = [c for c in C.CASES if c.kind == "bias"]
    assert {C.bias_slices(C.padded(c.B, c.H, c.W)[3]) for c in bias} >= {1, 2, 4} and any(c.M > 256 and c.M % 256 for c in bias)
    assert any(c.M // 4 > 8192 * 256 for c in C.CASES if c.kind == "relu")
    assert {c.branch for c in C.CASES if c.kind == "dgrad3"} == {"split", "direct"}
    assert {(c.branch, c.up) for c in C.CASES if c.kind == "dgrad2"} == {(b, u) for b in ("bf16s", "fp32") for u in (False, True)}
    assert {c.branch for c in C.CASES if c.kind == "dgrad3d"} == {"split", "thin", "fp32"}
    assert {(c.D, c.up) for c in C.CASES if c.kind == "dstride3d"} == {(d, u) for d in (1, 2) for u in (False, True)}
    assert {c.mode for c in C.CASES if c.kind in ("dgrad3", "dgrad3d")} == {"plain", "res", "gate"}
    # every wide class that is left out is left out for the stated arithmetic reason
    for c in C.CASES:
        if c.kind.startswith("wgrad") or c.kind == "bias":
            assert c.wide == (c.B * max(c.D, 1) * c.H * c.W * 8190 + 3 * 1024 < 2 ** 24), c.id
