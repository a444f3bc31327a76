"""Walsh-Hadamard kernels (deepinv_amd/csrc/hadamard.hip) on the host emulation: both kernel forms (the resident one and the
two-pass one, forced on small planes through DINV_HAD_RESIDENT_LOG2) against the float64 restatement of tests/hadamard_cases.py
(an fp64 butterfly, H_H x H_W / sqrt(H W)), which also holds the case table, for every operator of SinglePixelCamera
(deepinv/physics/singlepixel.py:408-439 with deepinv/physics/forward.py:1080-1117, 1212-1252).

The bound against fp64 is the worst-case rounding of the arithmetic, not a measured figure: a transform over L index bits is L
rounded additions per output, each relative 2^-24, and the scale, the symbol's products and its division add at most four
more, so the relative l2 error of one transform is at most (L + 4) 2^-24 and of an operator with two transforms twice that."""
import pytest
import torch

import emu_lib as E
from emu_backend import emu_backend
from emu_lib import check, lib
from hadamard_cases import (CASES, IDS, LAST_AXIS, NO_NORMALIZE, NO_TRANSFORM, PRE, RESIDENT_LOG2, SECOND, SYM, U, bits, make,
                            r_h2, r_inv, r_last, rel)

from deepinv_amd.hip import hadamard as hhad


def hadamard(x, flags=0, scale=1.0):
    P, H, W = x.shape[0] * x.shape[1], x.shape[2], x.shape[3]
    out = torch.full_like(x, float("nan"))
    check(lib().dinv_hadamard(E.p(x), E.p(out), P, H, W, flags, scale, None, 0, None))
    return out


def apply(x, mask, flags, y=None, add=0.0, scale=1.0):
    P, H, W = x.shape[0] * x.shape[1], x.shape[2], x.shape[3]
    out = torch.full_like(x, float("nan"))
    check(lib().dinv_hadamard_apply(E.p(x), E.p(y), E.p(mask), E.p(out), P, H, W, mask.shape[0] * mask.shape[1], flags, add,
                                    scale, None, 0, None))
    return out


@pytest.mark.parametrize("shape,c", CASES, ids=IDS)
def test_plain_transform(shape, c):
    x, _, _ = make(shape, 1)
    f = RESIDENT_LOG2(c)
    L = bits(*shape[2:])
    got = hadamard(x, f)
    assert rel(got, r_h2(x)) <= (L + 4) * U
    if not c:                                                    # the product's wrapper makes the same call (it forces no kernel form)
        with emu_backend():
            assert torch.equal(hhad.fwht(x), got)
    # un-normalised, and the caller's scale
    got = hadamard(x, f | NO_NORMALIZE, 0.5)
    assert rel(got, 0.5 * r_h2(x) * (shape[2] * shape[3]) ** 0.5) <= (L + 4) * U
    # involution and Parseval
    back = hadamard(hadamard(x, f), f)
    assert rel(back, x.double()) <= 2 * (L + 4) * U
    assert abs(float(hadamard(x, f).double().norm() / x.double().norm()) - 1) <= (L + 4) * U
    # in place
    z = x.clone()
    P = shape[0] * shape[1]
    check(lib().dinv_hadamard(E.p(z), E.p(z), P, shape[2], shape[3], f, 1.0, None, 0, None))
    assert torch.equal(z, hadamard(x, f))


@pytest.mark.parametrize("shape,c", CASES, ids=IDS)
def test_last_axis(shape, c):
    """hadamard_1d: the last axis only, both normalize values; an odd number of rows of 2 floats ends inside a 16-byte access"""
    x, _, _ = make(shape, 2)
    W = shape[3]
    f = RESIDENT_LOG2(min(c, 14)) if c else 0
    L = W.bit_length() - 1
    want = r_last(x)
    assert rel(hadamard(x, f | LAST_AXIS), want / W ** 0.5) <= (L + 4) * U
    assert rel(hadamard(x, f | LAST_AXIS | NO_NORMALIZE), want) <= (L + 4) * U


@pytest.mark.parametrize("mask_batch", [False, True], ids=["shared", "per-batch"])
@pytest.mark.parametrize("binary", [True, False], ids=["binary", "real"])
@pytest.mark.parametrize("shape,c", CASES, ids=IDS)
def test_operator_table(shape, c, binary, mask_batch):
    x, y, mask = make(shape, 3, mask_batch, binary)
    f = RESIDENT_LOG2(c)
    L = bits(*shape[2:])
    m = mask.double()
    one, two = (L + 4) * U, 2 * (L + 4) * U
    zero = (mask == 0).expand(shape)

    def exactly_zero(t):
        """zero where the mask is: the sign bit aside (0 * negative = -0), every bit"""
        return bool(((t[zero].view(torch.int32) & 0x7FFFFFFF) == 0).all())

    Ax = apply(x, mask, f | SYM(1))
    assert rel(Ax, m * r_h2(x)) <= one and exactly_zero(Ax)
    assert rel(apply(y, mask, f | PRE(1)), r_h2(m * y.double())) <= one
    assert rel(apply(x, mask, f | SYM(2) | SECOND), r_h2(m * m * r_h2(x))) <= two
    AAt = apply(y, mask, f | SYM(2) | NO_TRANSFORM)
    assert exactly_zero(AAt)
    if binary:
        assert torch.equal(AAt, mask * mask * y)         # an exact product
    else:
        assert rel(AAt, m * m * y.double()) <= 2 * U
    for gamma in (0.7, 1e-3):
        want = r_h2((m * y.double() + r_h2(x) / gamma) / (m * m + 1 / gamma))
        assert rel(apply(x, mask, f | SYM(3) | SECOND, y=y, add=1 / gamma), want) <= two + 4 * U, gamma
    assert rel(apply(y, mask, f | PRE(2)), r_h2(y.double() * r_inv(m))) <= one + U
    # the transposes the backward passes use
    assert rel(apply(x, mask, f | SYM(4), add=1 / 0.7), m * r_h2(x) / (m * m + 1 / 0.7)) <= one + 2 * U
    Dx = apply(x, mask, f | SYM(5))
    assert rel(Dx, r_h2(x) * r_inv(m)) <= one + U and exactly_zero(Dx)
    assert rel(apply(x, mask, f | SYM(3) | SECOND, add=1 / 0.7), r_h2(r_h2(x) / 0.7 / (m * m + 1 / 0.7))) <= two + 4 * U
    # the caller's scale
    assert rel(apply(x, mask, f | SYM(1), scale=-2.0), -2 * m * r_h2(x)) <= one


@pytest.mark.parametrize("shape,c", [((5, 7, 32, 32), 0), ((1, 3, 8, 8), 4), ((2, 1, 64, 64), 11)])
def test_two_forms_agree_and_repeat(shape, c):
    """the run-to-run result is bit-identical, and the fused two-transform call equals the composed single calls"""
    x, y, mask = make(shape, 4)
    f = RESIDENT_LOG2(c)
    a = apply(x, mask, f | SYM(2) | SECOND)
    assert torch.equal(a, apply(x, mask, f | SYM(2) | SECOND))
    composed = apply(apply(x, mask, f | SYM(1)), mask, f | PRE(1))
    assert rel(a, composed.double()) <= 2 * (bits(*shape[2:]) + 4) * U


def test_full_mask_round_trip():
    """m = H W: A_dagger(A(x)) = x"""
    x, _, _ = make((2, 2, 16, 32), 5)
    mask = torch.ones(1, 2, 16, 32)
    back = apply(apply(x, mask, SYM(1)), mask, PRE(2))
    assert rel(back, x.double()) <= 2 * (9 + 4) * U


def test_argument_checks():
    l = lib()
    x = torch.zeros(1, 1, 8, 8)
    out = torch.empty_like(x)
    assert l.dinv_hadamard_workspace_bytes(4, 128, 128) == 0
    assert l.dinv_hadamard(E.p(x), E.p(out), 1, 6, 8, 0, 1.0, None, 0, None) != 0
    assert b"powers of two" in l.dinv_last_error()
    assert l.dinv_hadamard(E.p(x), E.p(out), 1, 2048, 8, 0, 1.0, None, 0, None) != 0
    assert b"side above 1024" in l.dinv_last_error()
    assert l.dinv_hadamard(E.p(x), None, 1, 8, 8, 0, 1.0, None, 0, None) != 0
    buf = torch.zeros(65)
    assert l.dinv_hadamard(E.p(buf[1:]), E.p(out), 1, 8, 8, 0, 1.0, None, 0, None) != 0
    assert b"aligned" in l.dinv_last_error()
    assert l.dinv_hadamard(E.p(x), E.p(out), 1, 8, 8, RESIDENT_LOG2(1), 1.0, None, 0, None) != 0
    m = torch.ones(1, 1, 8, 8)
    assert l.dinv_hadamard_apply(E.p(x), None, E.p(m), E.p(out), 3, 8, 8, 2, SYM(1), 0.0, 1.0, None, 0, None) != 0
    assert b"divides P" in l.dinv_last_error()
    assert l.dinv_hadamard_apply(E.p(x), None, None, E.p(out), 1, 8, 8, 1, SYM(1), 0.0, 1.0, None, 0, None) != 0
    assert l.dinv_hadamard_apply(E.p(x), None, E.p(m), E.p(out), 1, 8, 8, 1, SYM(7), 0.0, 1.0, None, 0, None) != 0
    assert b"symbol mode" in l.dinv_last_error()
    assert l.dinv_hadamard_apply(E.p(x), None, E.p(m), E.p(out), 1, 8, 8, 1, SYM(2) | SECOND | NO_TRANSFORM, 0.0, 1.0, None, 0,
                                 None) != 0
    assert l.dinv_hadamard_apply(E.p(x), E.p(out), E.p(m), E.p(out), 1, 8, 8, 1, SYM(3) | SECOND, 1.0, 1.0, None, 0, None) != 0
    assert b"alias" in l.dinv_last_error()
