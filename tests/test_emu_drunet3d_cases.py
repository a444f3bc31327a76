"""The 3-D forms of the DRUNet kernels (dinv_conv3x3x3 in its wide and thin kernels, dinv_conv3x3x3_split,
dinv_conv_down2x2_bf16s_3d, dinv_conv_up2x2_bf16s_3d) on the host emulation of the kernel sources (tests/emu): the case table of
tests/drunet3d_cases.py, every call through the C entry points on guarded buffers with NaN in every slack and guard plane.  Every `int`
and `wide` run must equal the fp64 reference bit for bit, every `randn` run stays inside its derived per-element ceiling; guards,
untouched words, zero frames and padding slices, unchanged operands and the launched kernel instance (the emulation's launch log) are
checked on every run.  Then every layer shape of the 16 / 32 / 64 / 128 network through Ops3d.conv3 / down / up in three settings:
which kernel runs, and the bits of the table's call.  tests/test_drunet3d_kernels_gpu.py runs the same table on the device.
`python -m pytest tests/test_emu_drunet3d_cases.py -s` prints every run's worst fraction of its ceiling."""
import pytest

import drunet3d_cases as C
from emu_backend import emu_backend


@pytest.fixture(scope="module")
def be():
    with emu_backend():
        yield C.Backend("cpu")


@pytest.mark.parametrize("case,cls", C.items(emu=True), ids=C.item_id)
def test_drunet3d_case_emulated(be, case, cls):
    C.run_case(be, case, cls)


@pytest.mark.parametrize("layer,setting", C.production_items(emu=True), ids=lambda v: v if isinstance(v, str) else v[0])
def test_ops3d_launches_what_the_table_tests_emulated(be, layer, setting):
    C.run_production(be, *layer, setting)


def test_case_table_reaches_every_regime():
    """the table itself, through the restated launcher arithmetic (drunet3d_cases.reached): every regime the issue of the 3-D kernels
    names is reached by a case that runs on the emulation (the automatic 256-pixel workgroup of the 2-D tiles: device only)"""
    for emu in (True, False):
        R = {k: [(c, C.reached(c)) for c in C.CASES if c.kind == k and not (emu and c.gpu_only)] for k in {c.kind for c in C.CASES}}

        def some(kind, *names, mode=None, **attr):
            return any(all(n in r for n in names) and (mode is None or c.mode == mode) and all(getattr(c, k) == v for k, v in attr.items())
                       for c, r in R[kind])

        # 1. dinv_conv3x3x3
        for n in ("np<256", "D1", "volumes-in-tile", "straddles", "plane>256", "ragged", "tpx1-idle", "9tiles"):
            for k in ("mrep2", "thin"):
                assert some("direct", n, k), (n, k)
        for m in ("plain", "relu", "res", "relu+res"):
            assert some("direct", "mrep2", mode=m, cin=16, cout=64) or some("direct", "mrep2", mode=m, cin=8, cout=128), m
        assert {c.mode for c, r in R["direct"] if "mrep2" in r and (c.cin, c.cout) == (8, 128)} >= {"plain", "res", "relu+res"}
        assert some("direct", "mrep1", cout=32) and some("direct", "mrep1", "ytiles3", cout=96) and some("direct", "mrep2", "cbv5of8", cout=40)
        assert {c.mode for c, r in R["direct"] if "mrep1" in r} >= {"plain", "relu", "res", "relu+res"}
        for cin, cout, m in ((16, 16, "relu"), (16, 16, "relu+res"), (3, 16, "relu"), (16, 2, "plain"), (16, 2, "res"), (8, 8, "plain")):
            assert some("direct", "thin", mode=m, cin=cin, cout=cout), (cin, cout, m)
        assert some("direct", "thin", "plane>256", mode="gate", cin=16, cout=16)
        assert any(c.special and "thin" in r for c, r in R["direct"]) and any(c.special and "mrep2" in r and c.D > 1 for c, r in R["direct"])
        # 2. dinv_conv3x3x3_split
        for n in ("tc8", "tc16", "tc32", "partial-col", "ragged-row", "pad-slice-in-tile", "nk3", "nk6", "nk24", "ytiles2"):
            assert some("split", n), n
        assert some("split", "tc8", "partial-col", W=12) and some("split", "D1", V=1)
        s2 = [c for c, _ in R["split"]]
        assert {c.mode for c in s2} == {"plain", "relu", "res", "gate"} and {c.tile for c in s2} >= {0, 1, 2}
        assert {c.cin for c in s2} >= {16, 32, 128} and {c.cout for c in s2} == {64, 128}
        assert {(c.mode, c.fmt) for c in s2} >= {("relu", "out_split"), ("res", "in_split")} and R["pair"]
        assert all(c.fmt == "presplit" and C.pair_halves(c)[0].fmt == "out_split" and C.pair_halves(c)[1].fmt == "in_split" for c, _ in R["pair"])
        assert some("split", "auto1")
        if not emu:
            assert some("split", "auto1", "n256=382") and some("split", "auto2", "n256=384")
        # 3. the stride-2 pair
        for k, geos in (("down", {(2, 1, 2, 4), (1, 3, 5, 6), (2, 2, 7, 9)}), ("up", {(2, 1, 2, 4), (1, 3, 5, 6), (2, 2, 7, 5)})):
            cs = [c for c, _ in R[k]]
            assert {(c.V, c.D, c.H, c.W) for c in cs} >= geos and {c.cin for c in cs} == {16, 64} and {c.cout for c in cs} == {64, 128}
            assert some(k, "straddles") and some(k, "D1")
        assert {c.mode for c, _ in R["up"]} == {"plain", "x2"}
    # every case that leaves the wide classes out says why
    for c in C.CASES:
        assert c.wide or c.note, c.id
    # what production launches: every layer of the network, and the dispatch restated for each setting
    names = [l[0] for l in C.production_layers()]
    assert len(names) == len(set(names)) == 12
    for setting, (train, prec) in C.SETTINGS.items():
        got = {l[0]: C.production_case(*l, train, prec) for l in C.production_layers()}
        assert all(got[n].kind == "direct" and C.direct_pack(got[n].cout)[1] == 16 for n in ("head", "tail"))
        assert got["block0"].fmt == "direct" and C.direct_pack(got["block0"].cout)[1] == 16        # thin in every setting
        for i in (1, 2, 3):
            assert got[f"block{i}"].fmt == ("presplit" if setting == "infer-bf16split" else "direct"), (setting, i)
        assert (got["down2"].D, got["down2"].H, got["down2"].W) == (2, 2, 2) == (got["up2"].D, got["up2"].H, got["up2"].W)
