"""The DRUNet / DnCNN inference kernels (pack / unpack, the direct fp32 convolution and its thin form, Winograd F(4x4)
in its fp32 and bf16x3 forms, the bf16-split 2-D-tile and Winograd F(2,3) convolutions, the stride-2 layers, the tail) on the host
emulation of the kernel sources (tests/emu): the part of the case table of tests/drunet_fwd_cases.py that the fiber emulation
finishes in seconds, every call through the C entry points on guarded buffers with NaN in every slack.  Every `int` and `wide` run
must equal the fp64 reference bit for bit (F(4x4): inside the ceiling computed from its pack's rounding), every `randn` run stays inside its derived
per-element ceiling; guards, untouched words, frame and NaN-free interior are checked on every run, the launched kernel instance
through the emulation's launch log.  tests/test_drunet_kernels_gpu.py runs the whole table on the device (F(2x2) only there: its
LDS barrier is inline assembly).  `python -m pytest tests/test_emu_drunet_cases.py -s` prints every run's worst fraction of its ceiling."""
import pytest

import drunet_fwd_cases as C
from emu_backend import emu_backend


@pytest.fixture(scope="module")
def be():
    with emu_backend():
        yield C.Backend("cpu")


@pytest.mark.parametrize("case,cls", C.items(emu=True), ids=C.item_id)
def test_drunet_fwd_case_emulated(be, case, cls):
    C.run_case(be, case, cls)


def _cases(kind, backend):
    return [c for c in C.CASES if c.kind == kind and not (backend == "emu" and c.gpu_only)]


def test_case_table_reaches_every_regime():
    """the table itself, through the restated launcher arithmetic (drunet_fwd_cases.reached), for the emulated device (2 compute units
    per XCD) and for the MI355X (32): every regime the kernels' launchers distinguish is reached by a case that runs on that backend
    (F(2x2), the n256 = 384 pair of the 2-D tiles, the flat tail kernel and the device's full + tail round of F(4x4): device only)"""
    for backend in ("emu", "gpu"):
        R = {k: [(c, C.reached(c, backend)) for c in _cases(k, backend)] for k in {c.kind for c in C.CASES}}

        def some(kind, *names, mode=None):
            return any(all(n in r for n in names) and (mode is None or c.has(mode) or (mode == "plain" and c.mode == "plain"))
                       for c, r in R[kind])

        # 1. pack / unpack: widths around the 64-column block, every channel count and sigma form
        assert {c.W for c in _cases("pack", backend)} >= {1, 63, 64, 65, 130} and {c.cin for c in _cases("pack", backend)} >= {1, 3, 7}
        assert {c.fmt for c in _cases("pack", backend)} == {"py", "dev", "batch", "map"}
        assert {c.W for c in _cases("unpack", backend)} >= {1, 63, 64, 65, 130} and {c.cout for c in _cases("unpack", backend)} >= {1, 3, 8}
        # 2. the direct kernel
        for n in ("np<256", "np=256", "ragged", "9tiles", "head", "tail-layer", "pick32"):
            assert some("direct", n), (backend, n)
        d = _cases("direct", backend)
        assert any(c.B == 3 and c.H == 1 and c.W == 1 for c in d)
        assert any((c.cin, c.cout, c.B, c.H, c.W) == (o.cin, o.cout, o.B, o.H, o.W) and {c.tile, o.tile} == {32, 64} and c.cout % 64 == 0
                   for c in d for o in d)                                   # MREP 2 and MREP 1 on the same layer
        assert any(c.cout == 96 and c.tile == 32 for c in d) and any(c.cout == 128 and c.tile == 64 for c in d)
        plain = [c for c in d if not c.has("bias")]
        assert {c.mode for c in plain if c.tile != 16} >= {"plain", "relu", "res", "relu+res", "res+res2", "x2"}
        assert {c.cout for c in plain if c.tile == 16} >= {2, 16} and {c.mode for c in plain if c.tile == 16} >= {"plain", "relu", "res"}
        assert {(c.tile, c.mode) for c in d if c.has("bias")} == {(t, m) for t in (16, 32, 64) for m in ("bias", "bias+relu", "bias+res")}
        # 3. F(2x2) (device only)
        if backend == "gpu":
            for rect in ((4, 16), (8, 8), (4, 4)):
                assert some("wino2", rect, True) and some("wino2", rect, False), rect
            w2 = _cases("wino2", backend)
            assert any(c.H % 2 and c.W % 2 for c in w2) and any((c.H, c.W) == (1, 1) for c in w2) and any((c.H, c.W) == (37, 51) for c in w2)
            assert any((c.H, c.W) == (2, 330) for c in w2) and {c.cin for c in w2} >= {32, 48, 64} and any(c.cout == 128 for c in w2)
            assert some("wino2", "straddles") and some("wino2", "walks") and {c.mode for c in w2} == {"plain", "relu", "res"}
        else:
            assert not R["wino2"]
        # 4. F(4x4), both forms
        for k in ("wino4", "wino4x3"):
            for rect in ((4, 8), (4, 4), (2, 2)):
                assert some(k, rect, True) and some(k, rect, False), (k, rect)
            w4 = _cases(k, backend)
            assert some(k, "ct-major") and any(not c.ws for c in w4)
            assert some(k, "ntail0-" + backend)                            # with a workspace and nothing to split
            got = {r_ for c, r in R[k] if c.ws for r_ in r if isinstance(r_, tuple) and r_[0] == "split"}
            assert {f for _, f, _ in got} >= ({1, 2} if backend == "emu" else {1, 2, 4, 8}), (k, backend, got)
            assert some(k, "unsplit-48") and some(k, "all-tail") and some(k, "full+tail-" + backend)
            for m in ("relu", "res"):                                      # in tail tiles, in a full + tail launch and in full tiles
                assert some(k, "all-tail", mode=m) and some(k, "full+tail-" + backend, mode=m), (k, m)
                assert any(c.has(m) and ("split", 1, 0) in r for c, r in R[k]), (k, m)
            assert any(c.mode == "plain" and ("split", 1, 0) not in r for c, r in R[k])
        assert {c.mode for c in _cases("wino4", backend) if c.has("bias")} == {"bias", "bias+relu"}
        # 5. the 2-D tiles
        for n in ("tc32", "tc16", "tc8", "partial-col", "auto1"):
            assert some("split", n), n
        s2 = _cases("split", backend)
        assert {c.tile for c in s2} >= {0, 1, 2} and {c.fmt for c in s2} == {"f32", "in_split", "out_split"}
        assert {c.mode for c in s2} == {"plain", "relu", "res"}
        if backend == "gpu":
            assert some("split", "auto1", "n256=376") and some("split", "auto2", "n256=384")
        # 6. F(2,3) on the bf16 cores
        for n in ("tc32", "tc16", "tc8", "partial-col", "ragged-row", "ends-inside"):
            assert some("wsplit", n), n
        ws = _cases("wsplit", backend)
        assert {c.W for c in ws} >= {2, 34} and {c.cin for c in ws} == {16, 32} and {c.cout for c in ws} == {64, 128}
        assert {c.mode for c in ws} == {"plain", "relu", "res"}
        # 7. stride 2
        for k, cins in (("down", {8, 24}), ("down_bf16s", {16, 32}), ("down_bf16x3", {16, 32})):
            cs = _cases(k, backend)
            assert {c.cin for c in cs} == cins and {c.cout for c in cs} == {64, 128} and some(k, "9tiles")
            assert {(c.H, c.W) for c in cs} >= {(1, 1), (5, 6)}
        for k, cins in (("up", {24, 64}), ("up_bf16s", {64})):
            cs = _cases(k, backend)
            assert {c.cin for c in cs} == cins and {c.cout for c in cs} == {64, 128} and {c.mode for c in cs} == {"plain", "x2"}
            for n in ("np<128", "np=128", "np>128"):
                assert some(k, n), (k, n)
        # 8. the tail
        t = _cases("tail", backend)
        assert {c.cout for c in t} == {1, 2, 3, 4} and {c.W for c in t} >= {62, 63, 124, 125}
        # (rb = 4 and 8 need 2048 waves in the launch - 15 s of fibers each - and the flat kernel 65536 images: the device only)
        rbs = ("rb2", "rb4", "rb8") if backend == "gpu" else ("rb2",)
        for n in ("strips1", "strips2", "strips3") + rbs:
            assert some("tail", n), n
        assert all(any(n in r and "ragged" in r for c, r in R["tail"]) for n in rbs)
        assert {m for c in t for m in c.mode.split("+")} >= {"x2", "bias", "res"}
        if backend == "gpu":
            assert some("tail", "flat")
    # every case that leaves the wide classes out says why: F(4x4) always, F(2x2) at cin = 64
    for c in C.CASES:
        assert c.wide or (c.note and (c.kind in ("wino4", "wino4x3") or (c.kind == "wino2" and c.cin == 64))), c.id
