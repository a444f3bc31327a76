"""The noise and mask-generator kernels - csrc/random.hip - on the host emulation of the kernel sources (tests/emu), per element
against the replay of the Philox stream in tests/random_cases.py: the cases that the fiber emulation finishes quickly, through
the C entry points on guarded buffers, and the checks of the replay and of the tables on themselves: the Random123 known-answer
vectors, the uniforms, and that each grid case exceeds the cap it is named for.  tests/test_random_kernels_gpu.py runs the whole
table on the device."""
import ctypes

import numpy as np
import pytest

import emu_lib as E
import random_cases as RC

WORST = {}


def _stream():
    return ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def runner():
    return RC.Runner(E.lib(), "cpu", _stream)


# ------------------------------------------------------------------ the replay on itself
def test_philox_known_answers():
    """the three vectors of Random123's kat_vectors for philox4x32-10"""
    for counter, key, want in (
            ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = tuple(int(v[0]) for v in RC.philox_block(counter, key))
        assert got == want, [hex(v) for v in got]
    # the kernels' layout of the same function: the counter's and the seed's high words are words 1 of counter and key
    a = RC.philox(0x299f31d0a4093822, 0x85a308d3243f6a88, 0x13198a2e, 0x03707344)
    assert tuple(int(v[0]) for v in a) == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    assert int(RC.counters(2 ** 64 - 1, np.arange(3, dtype=np.uint64))[2]) == 1              # offset + index modulo 2^64


def test_uniforms_are_in_the_half_open_interval():
    r = np.asarray([0, 255, 256, 0xFFFFFFFF, 0xFFFFFF00, 0x40000000, 0x80000000], dtype=np.uint64)
    u = RC.u01(r)
    assert u.dtype == np.float32 and float(u[0]) == float(u[1]) == 2.0 ** -25 and float(u[2]) == 2.0 ** -24 + 2.0 ** -25
    # the sum rounds once, ties to even: the largest to 1, 1/2 + 2^-25 to 1/2
    assert float(u[3]) == float(u[4]) == 1.0 and float(u[5]) == 0.25 + 2.0 ** -25 and float(u[6]) == 0.5


def test_grid_cases_exceed_their_caps():
    """csrc/random.hip's launch rules, restated: each case named for a cap has more work than the capped grid holds and a ragged end"""
    big = [c for c in RC.GAUSS_TABLE if not c.emu]
    assert len(big) == 1 and RC.gaussian_blocks(big[0].n) == RC.GAUSS_CAP
    nq = RC.cdiv(big[0].n, 4)
    assert RC.GAUSS_CAP * 256 < nq < 2 * RC.GAUSS_CAP * 256 and nq % 256 and big[0].n % 4 == 3
    assert RC.gaussian_blocks(RC.GAUSS_CAP * 256 * 4) == RC.GAUSS_CAP and RC.gaussian_blocks(1027) == 2
    grid = {c.name: (RC.poisson_grid(c.batch, c.per), c) for c in RC.POIS_TABLE if c.name.startswith("grid-")}
    (bx, by), c = grid["grid-flat"]
    assert (bx, by) == (RC.POISSON_CAP, 1) and bx * 256 < c.per < 2 * bx * 256 and c.per % 256
    (bx, by), c = grid["grid-b64"]
    assert (bx, by) == (RC.POISSON_CAP // 64, 64) and bx * 256 < c.per < 2 * bx * 256 and c.per % 256
    (bx, by), c = grid["grid-b16385"]
    assert (bx, by) == (1, 16385) and RC.POISSON_CAP // by == 0 and 256 < c.per < 512
    (bx, by), c = grid["grid-b65538"]
    assert (bx, by) == (1, RC.POISSON_Y_CAP) and c.batch == RC.POISSON_Y_CAP + 3 and c.emu
    assert sorted(RC.POIS_BIG) == sorted(c.id for _, c in grid.values() if not c.emu) and len(RC.POIS_BIG) == 3
    assert all(c.emu for c in RC.MASK_TABLE) and {c.W for c in RC.MASK_TABLE} >= set(RC.MASK_WIDTHS)
    assert any(c.B * c.C * c.T * c.H * c.W < 256 for c in RC.MASK_TABLE) and any(c.H * c.W % 256 for c in RC.MASK_TABLE)


def test_advances_are_the_documented_ones():
    assert [RC.gaussian_advance(n) for n in (1, 4, 5, 16, 17, 1027)] == [4, 4, 4, 4, 8, 260]
    assert [RC.poisson_advance(n) for n in (1, 4, 5)] == [4, 4, 8]
    assert RC.mask_advance(3, 2) == 4 * ((6 * 1024 + 3 + 3) // 4)


def test_tight_elements_guard_the_log_pmf():
    """the fixture of nearly tied acceptance tests is what tests/random_cases.py says it is, from the replay alone"""
    k, m = RC.tight_margins()
    assert not np.isnan(k).any() and len(set(RC.TIGHT)) == len(RC.TIGHT)
    for kk in range(2, 10):                          # the table of log k!
        sel = m[k == kk]
        assert (sel > 0).sum() >= 2 and (sel < 0).sum() >= 2 and np.abs(sel).max() < 2e-5, (kk, sel)
    for kk in range(10, 16):                         # the Stirling series
        sel = m[k == kk]
        assert (kk == 15 or (sel > 0).sum() >= 2) and (sel < 0).sum() >= 2, (kk, sel)
        assert 1e-9 < np.abs(sel).min() and np.abs(sel).max() < 0.4 * RC.stirling_term(kk), (kk, sel)
    assert set(k.tolist()) == set(range(2, 16))


# ------------------------------------------------------------------ random.hip
@pytest.mark.parametrize("case", [c for c in RC.TABLE if c.emu], ids=lambda c: c.id)
def test_random_path_emulated(runner, case):
    WORST[case.id] = RC.run_case(runner, case)


def test_random_rejections_write_nothing(runner):
    RC.run_rejections(runner)


def test_random_worst_ratio_emulated():
    if not WORST:
        return
    cid, ratio = max(WORST.items(), key=lambda kv: kv[1])
    print(f"random (emulated): {len(WORST)} cases, worst error / bound {ratio:.3g} ({cid})")
    assert ratio <= 1.0
