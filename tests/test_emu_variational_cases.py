"""The total-variation, total-generalized-variation and loop-algebra kernels - csrc/tv.hip, csrc/tgv.hip, csrc/elementwise.hip -
on the host emulation of the kernel sources (tests/emu), per element against fp64: the cases of tests/variational_cases.py and
tests/loop_algebra_cases.py that the fiber emulation finishes quickly, through the C entry points on guarded buffers, and the
checks of the tables on themselves: the share of records on each side of every projection, the margins of the stop, the fp32
evaluation of the restatement within every bound, and that each grid-stride case exceeds the cap it is named for.
tests/test_variational_kernels_gpu.py runs the whole tables on the device."""
import ctypes

import pytest

import emu_lib as E
import loop_algebra_cases as LA
import variational_cases as VC

WORST = {"variational": {}, "loop-algebra": {}}


def _stream():
    return ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def variational():
    return VC.Runner(E.lib(), "cpu", _stream)


@pytest.fixture(scope="module")
def loop_algebra():
    return LA.Runner(E.lib(), "cpu", _stream)


def _summary(table):
    if not WORST[table]:
        return
    cid, ratio = max(WORST[table].items(), key=lambda kv: kv[1])
    print(f"{table} (emulated): {len(WORST[table])} cases, worst error / bound {ratio:.3g} ({cid})")
    assert ratio <= 1.0


# ------------------------------------------------------------------ tv.hip, tgv.hip
@pytest.mark.parametrize("case", [c for c in VC.TABLE if c.emu], ids=lambda c: c.id)
def test_variational_path_emulated(variational, case):
    WORST["variational"][case.id] = VC.run_case(variational, case)


def test_variational_rejections_write_nothing(variational):
    VC.run_rejections(variational)


def test_variational_worst_ratio_emulated():
    _summary("variational")


STEPS = [c for c in VC.TABLE if c.kind in ("tv-step", "tgv-step")]


@pytest.mark.parametrize("case", STEPS, ids=lambda c: c.id)
def test_fp32_restatement_is_within_the_bound(case):
    """the bound is one a correct fp32 implementation can meet: the fp32 evaluation of the fp64 restatement meets it"""
    ratio = VC.fp32_step_ratio(case)
    print(f"{case.id}: fp32 restatement at {ratio:.3g} of the bound")
    assert ratio <= 1.0


def test_both_sides_of_every_projection_are_taken():
    """in every case of 64 records or more, each side of the TV ball or clamp, of the TGV shrink of r and projection of u, and of
    the |Dx| == 0 branch of tv_grad takes between 10 % and 90 % of the records"""
    seen = 0
    for c in VC.TABLE:
        shares = VC.branch_shares(c)
        assert (shares is None) == (c.kind not in ("tv-step", "tgv-step", "tv-grad") or c.n < VC.MIN_RECORDS), c.id
        for name, share in (shares or {}).items():
            seen += 1
            assert 0.1 <= share <= 0.9, f"{c.id}: {name} at {share:.3f} of the records"
    assert seen >= 4 * 8          # the four named shapes and the workgroup and grid-stride shapes, each with 4 kinds


def test_stop_margins():
    """the fp64 sequence of every stop case has a k in 4..12 that fp32 cannot move: rel_k < 0.99 crit, every earlier tested
    ratio > 1.01 crit; and crit = 1 stops at the first tested iteration"""
    stops = [c for c in VC.TABLE if c.kind.endswith("-stop")]
    assert {c.shape for c in stops} == set(VC.STOP) and {c.kind for c in stops} == {"tv-stop", "tgv-stop"}
    for c in stops:
        _, _, k, crit, rels = VC.stop_plan(c)
        assert 4 <= k <= 12, f"{c.id}: no usable k in {rels}"
        assert rels[k] < 0.99 * crit and rels[k - 1] > 1.01 * crit and min(rels[2:k]) > 1.01 * crit, (c.id, k, crit, rels)
        assert rels[2] < 0.99


def test_table_holds_every_listed_shape():
    shapes = VC.EDGE + VC.ORDINARY + VC.STRIDED
    assert len(shapes) == 17 and len(set(shapes)) == 17
    for kind, aniso in (("tv-step", 0), ("tv-step", 1), ("tgv-step", 0), ("tv-ops", 0), ("tgv-ops", 0), ("tv-grad", 0)):
        assert {c.shape for c in VC.TABLE if c.kind == kind and c.aniso == aniso} == set(shapes)
    assert {c.shape for c in VC.TABLE if c.kind == "tv-fn"} == set(VC.EDGE + VC.ORDINARY) | {VC.FN_STRIDED}
    assert all(c.emu for c in VC.TABLE if c.n < 10 ** 5 or c.kind in ("tv-ops", "tgv-ops", "tv-grad"))
    assert max(max(v.values()) for v in VC.BOUNDS.values()) <= 64
    assert all(VC.tv_fn_bound(c.nd, m, c.n // c.shape[0]) <= 64 for c in VC.TABLE if c.kind == "tv-fn" for m in (0, 1))


def test_grid_stride_cases_exceed_their_caps():
    """csrc/tv_common.hpp grid_for, csrc/tv.hip dinv_tv_fn_blocks and csrc/elementwise.hip stream_blocks, dinv_batched_dot_blocks
    and the 2048-workgroup cap of the pointwise kernels, restated: each case named for a second pass has more work than its
    capped grid holds, a count that is no multiple of the 256 lanes, and the library returns the restated counts"""
    l = E.lib()
    for shape in VC.STRIDED:
        n = VC.Case("tv-step", shape).n
        assert VC.grid_for(n) == VC.MAX_BLOCKS == l.dinv_tv_cp_partials(n) == l.dinv_tgv_cp_partials(n)
        assert n > VC.MAX_BLOCKS * VC.THREADS and n % VC.THREADS and n < 2 * VC.MAX_BLOCKS * VC.THREADS
    per = VC.Case("tv-fn", VC.FN_STRIDED).n // VC.FN_STRIDED[0]
    assert VC.tv_fn_blocks(per) == 256 == l.dinv_tv_fn_blocks(per) and per > 256 * 1024 and per % VC.THREADS and VC.FN_STRIDED[0] == 2
    for n in (1, 255, 256, 257, 4096, 4097, 524288, 524289):
        assert VC.grid_for(n) == l.dinv_tv_cp_partials(n) and VC.tv_fn_blocks(n) == l.dinv_tv_fn_blocks(n)
        assert LA.dot_blocks(n) == l.dinv_batched_dot_blocks(n)
    named = {"lincomb": 1, "cg-update": 1, "dot": 1, "cdiv": 2, "mask-solve": 2, "fidelity": 1}
    for kind, count in named.items():
        over = [c for c in LA.TABLE if c.kind == kind and LA.strided(c)[0] > LA.strided(c)[1]]
        assert len(over) == count, (kind, [c.id for c in over])
        for c in over:
            items, lanes = LA.strided(c)
            assert items % 256 and items < 2 * lanes, c.id
    assert LA.stream_blocks(LA.STREAM_SIZES[-1]) == 2048 == LA.stream_blocks(LA.CG_BIG) and LA.dot_blocks(LA.DOT_SIZES[-1]) == 256
    assert LA.pointwise_blocks(LA.POINTWISE_BIG) == 2048 and LA.STREAM_SIZES[-1] % 4 == 3 and LA.CG_BIG % 4 == 0
    assert all(LA.dot_bound(n) <= 64 for n in LA.DOT_SIZES)


# ------------------------------------------------------------------ elementwise.hip
@pytest.mark.parametrize("case", [c for c in LA.TABLE if c.emu], ids=lambda c: c.id)
def test_loop_algebra_path_emulated(loop_algebra, case):
    WORST["loop-algebra"][case.id] = LA.run_case(loop_algebra, case)


def test_loop_algebra_rejections_write_nothing(loop_algebra):
    LA.run_rejections(loop_algebra)


def test_loop_algebra_worst_ratio_emulated():
    _summary("loop-algebra")
