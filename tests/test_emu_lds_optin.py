"""The dynamic-LDS opt-in of every launcher whose tile can exceed the default limit of 48 KB (csrc/common.hpp: raise_lds_cap), on
the host emulation, which counts the attribute calls and refuses a launch above the runtime's own limit of 64 KB unless
hipFuncSetAttribute recorded a cap for the kernel (tests/emu/include/hip/hip_runtime.h).

Each family runs the smallest shape whose request crosses the limit, twice: the first call makes exactly one attribute call (one
kernel instantiation is reached), the second none, both give the same bits, and the result is within the bound the family's own
emulated tests use.  The library is a copy of its own (emu_lib.private_copy: a TARGET of tests/emu/Makefile no other test loads),
so no other test has raised a cap before.  The sizes are those of the launchers, restated: fft_lds_bytes of fft_cases.py, 28 P
bytes a line for the DST, the tables of both axes and two planes for the structured operator, a 2^14-float tile for Hadamard,
(P + 8 (P + 1)) complex values for the ramp filter."""
import ctypes
import math

import numpy as np
import pytest
import torch

import emu_lib as E
import fft_cases as F
import radon_cases as K

LIMIT = 48 * 1024                 # kDefaultLdsBytes: the launchers opt in above this
EMU_LIMIT = 64 * 1024             # what the runtime, and so the emulation, lets through without a cap
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    return E.private_copy()


def fft_plan(lib, n):
    plan = E.FftPlan()
    table = np.zeros(lib.dinv_fft_table_bytes(n), np.uint8)
    assert lib.dinv_fft_plan_init(n, ctypes.byref(plan), E.p(table)) == 0
    return plan, table


def stage_cost(plan):
    """tests/test_emu_dst.py: a radix-r stage adds at most (r + 3) u to the relative l2 error, radix 4 and 8 count as two and
    three radix-2 levels"""
    return sum({4: 10, 8: 15}.get(r, r + 3) for r in plan.radix[:plan.nstages])


def rel(a, b):
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


# ---------------------------------------------------------------- one runner per family: () -> (result, error, bound)
N_FFT = 1792                      # 2^8 7: outside the static set, a generic stage; one line with its tables is 50 192 bytes


def fft_axis(lib, inner, inverse):
    plan, table = fft_plan(lib, N_FFT)
    assert plan.generic == 1
    lines = F.rows_lines_per_block(N_FFT, True) if inner == 1 else 1      # cols_tile_width: one column is all that fits 48 KB
    assert lines == 1 and F.fft_lds_bytes(N_FFT, True, lines) > LIMIT
    x = torch.randn(2, N_FFT, inner, dtype=torch.complex64, generator=torch.Generator().manual_seed(inner))
    scale = 1.0 / math.sqrt(N_FFT)

    def run():
        out = torch.full_like(x, float("nan"))
        rc = lib.dinv_fft_c2c_axis(E.p(torch.view_as_real(x)), E.p(torch.view_as_real(out)), 2, inner, ctypes.byref(plan), E.p(table),
                                   inverse, 0, scale, None)
        assert rc == 0, lib.dinv_last_error()
        ref = F.c2c_ref(x.to(torch.complex128), 1, inverse, 0, scale)
        return out, F.worst_line_error(out.transpose(1, 2), ref.transpose(1, 2)), F.BOUNDS["rows-generic" if inner == 1 else "cols-generic"]
    return run


def dst1(lib):
    n, P = 1024, 2050
    assert F.fft_lds_bytes(P, True, 1) > LIMIT                           # one pair of rows: 2 rows make one workgroup
    plan, table = fft_plan(lib, P)
    x = torch.randn(2, n, generator=torch.Generator().manual_seed(n))
    j = torch.arange(1, n + 1, dtype=torch.float64)
    want = x.double() @ (-math.sqrt(2.0 / (n + 1)) * torch.sin(math.pi * j[:, None] * j[None, :] / (n + 1)))

    def run():
        out = torch.full_like(x, float("nan"))
        assert lib.dinv_dst1(E.p(x), E.p(out), 2, n, ctypes.byref(plan), E.p(table), None) == 0, lib.dinv_last_error()
        return out, rel(out.double(), want), (stage_cost(plan) + 2) * U
    return run


def cstructured(lib):
    n = 64
    tables = 2 * (n * 8 + n * 4)
    assert tables + 2 * n * (n + 1) * 8 == 68096
    plan, table = fft_plan(lib, n)
    x = torch.randn(1, n, n, dtype=torch.complex64, generator=torch.Generator().manual_seed(n))
    want = torch.fft.fft2(x.to(torch.complex128), norm="ortho")

    def run():
        out = torch.full_like(x, float("nan"))
        rc = lib.dinv_cstructured_apply(E.p(torch.view_as_real(x)), E.p(torch.view_as_real(out)), None, None, 1, n, n, n, n, n, n, 0, 0, 1,
                                        0, 1, 0, 0, 0.0, ctypes.byref(plan), E.p(table), ctypes.byref(plan), E.p(table), None)
        assert rc == 0, lib.dinv_last_error()
        return out, rel(out.to(torch.complex128), want), (2 * stage_cost(plan) + 1) * U      # phase_retrieval_cases.derived_fft_bound
    return run


def hadamard(lib):
    side = 128                    # one plane of 2^14 floats: a tile of 69 648 bytes with its padding
    x = torch.randn(1, 1, side, side, generator=torch.Generator().manual_seed(side))
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < side:
        h = torch.cat((torch.cat((h, h), 1), torch.cat((h, -h), 1)), 0)
    want = h @ x.double() @ h / side

    def run():
        out = torch.full_like(x, float("nan"))
        assert lib.dinv_hadamard(E.p(x), E.p(out), 1, side, side, 0, 1.0, None, 0, None) == 0, lib.dinv_last_error()
        return out, rel(out.double(), want), (14 + 4) * U                                    # tests/test_emu_hadamard.py
    return run


def ramp(lib):
    N, A = 257, 2                 # P = 1024: the twiddles and 8 columns of P + 1 are 73 792 bytes
    P = lib.dinv_radon_ramp_padded_size(N)
    assert P == 1024 and K.ramp_ct(P) == 8 and (P + 8 * (P + 1)) * 8 > LIMIT
    plan, table = fft_plan(lib, P)
    filt = np.zeros(P, np.float32)
    assert lib.dinv_radon_ramp_filter_init(P, E.p(table), E.p(filt)) == 0
    y = torch.randn(1, N, A, generator=torch.Generator().manual_seed(N))

    def run():
        out = torch.full_like(y, float("nan"))
        assert lib.dinv_radon_ramp_fft(1, N, A, P, ctypes.byref(plan), E.p(table), E.p(filt), E.p(y), E.p(out), None) == 0, lib.dinv_last_error()
        return out, K.ramp_fft_ratio(out, y, P), K.BOUNDS["ramp_fft"]
    return run


FAMILIES = {
    "fft-rows-fwd": lambda l: fft_axis(l, 1, 0), "fft-rows-inv": lambda l: fft_axis(l, 1, 1),      # two instantiations of one template:
    "fft-cols-fwd": lambda l: fft_axis(l, 2, 0), "fft-cols-inv": lambda l: fft_axis(l, 2, 1),      # each raises its own cap
    "dst1": dst1, "cstructured": cstructured, "hadamard": hadamard, "radon-ramp": ramp,
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_first_call_raises_the_cap_once(lib, family):
    run = FAMILIES[family](lib)
    calls = lib.dinv_emu_func_attribute_calls
    before = calls()
    first, err, bound = run()
    assert calls() == before + 1, "the first launch above 48 KB makes one attribute call for the one kernel it reaches"
    print(f"{family}: error {err:.3g} bound {bound:.3g}")
    assert not torch.isnan(torch.view_as_real(first) if first.is_complex() else first).any()
    assert err <= bound
    second, _, _ = run()
    assert calls() == before + 1, "a later launch of the same kernel makes no runtime call"
    assert torch.equal(torch.view_as_real(first) if first.is_complex() else first, torch.view_as_real(second) if second.is_complex() else second)


def test_emulation_refuses_a_launch_without_its_cap(lib):
    """the emulation itself, on a kernel of the test's own (tests/emu/lds_probe.cpp): at the limit any launch runs, above it only
    one whose kernel has a recorded cap that covers it, and a refused launch is an error of the call and runs nothing"""
    out = torch.zeros(1, dtype=torch.int32)
    calls = lib.dinv_emu_func_attribute_calls
    before = calls()
    assert lib.dinv_emu_lds_probe(E.p(out), EMU_LIMIT, 0) == 0 and int(out) == 7
    out.zero_()
    assert lib.dinv_emu_lds_probe(E.p(out), EMU_LIMIT + 16, 0) != 0
    assert b"kernel launch failed" in lib.dinv_last_error() and b"dynamic LDS" in lib.dinv_last_error()
    assert int(out) == 0 and calls() == before
    assert lib.dinv_emu_lds_probe(E.p(out), EMU_LIMIT + 16, 1) == 0 and int(out) == 7 and calls() == before + 1
    assert lib.dinv_emu_lds_probe(E.p(out), 160 * 1024, 1) == 0 and calls() == before + 1
    out.zero_()
    assert lib.dinv_emu_lds_probe(E.p(out), 160 * 1024 + 16, 1) != 0 and int(out) == 0       # above the recorded cap
    assert lib.dinv_emu_lds_probe(E.p(out), EMU_LIMIT, 0) == 0 and int(out) == 7                   # the error did not stick
