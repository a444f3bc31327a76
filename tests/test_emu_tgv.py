"""Total-generalized-variation kernels (deepinv_amd/csrc/tgv.hip) on the host emulation, on small odd shapes, against a float64
PyTorch restatement of the reference (deepinv/models/tgv.py:93-310): the Chambolle-Pock iteration with its device stopping
rule and ping-pong buffers, and the epsilon / epsilon^T pair."""
import pytest
import torch

import emu_lib as E
from emu_backend import emu_backend
from emu_lib import check, lib
from variational_cases import r_epsilon, r_epsilon_adjoint, r_tgv_prox      # the float64 restatement of the reference

from deepinv_amd.hip import tgv as htgv


def geo(shape):
    return (2, shape[0], shape[1], 1, shape[2], shape[3]) if len(shape) == 4 else (3, *shape)


def run_cp(y, lam, x2, r2, u2, n_launch, crit):
    """n_launch iterations enqueued on the emulation (no host polling: launches after convergence must be no-ops)"""
    l = lib()
    nd, B, C, D, H, W = geo(y.shape)
    xs, rs, us = (x2.clone(), torch.empty_like(x2)), (r2.clone(), torch.empty_like(r2)), (u2.clone(), torch.empty_like(u2))
    z, w = torch.empty_like(y), torch.empty_like(r2)
    part = torch.empty(2 * l.dinv_tgv_cp_partials(y.numel()))
    st = torch.zeros(2, dtype=torch.int32)
    sigma = 1 / 0.01 / (72 * (3 if nd == 3 else 1))
    l1, l2 = lam * 0.1, lam * 0.15
    for _ in range(n_launch):
        check(l.dinv_tgv_cp_iter(nd, B, C, D, H, W, E.p(xs[0]), E.p(xs[1]), E.p(rs[0]), E.p(rs[1]), E.p(us[0]), E.p(us[1]),
                                 E.p(y), E.p(l1), E.p(l2), 0.01, sigma, 1.99, crit, E.p(z), E.p(w), E.p(part), E.p(st), None))
    it = int(st[1])
    return xs[it & 1], rs[it & 1], us[it & 1], it, int(st[0])


def zeros_state(shape, dtype=torch.float32):
    nd = len(shape) - 2
    return torch.zeros(*shape, nd, dtype=dtype), torch.zeros(*shape, nd * nd, dtype=dtype)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# about 4x the worst (x2, r2, u2) errors measured on the emulation over the cases below: against the fp64 restatement
# (fp32 rounding: the fp32 restatement is as far from it) and against the same restatement run in fp32
BOUND64 = (6.5e-6, 1.2e-5, 1.6e-4)
BOUND32 = (3.5e-7, 9e-7, 5e-6)


def assert_matches(got, y, lam, x0, r0, u0, n_it, crit=0.0):
    """got = (x2, r2, u2) of the kernels against the restatement in fp64 and in fp32 from the same start"""
    ref64 = r_tgv_prox(y.double(), lam.double(), x0.double(), r0.double(), u0.double(), n_it, crit)
    ref32 = r_tgv_prox(y, lam, x0, r0, u0, n_it, crit)
    for a, b64, b32, t64, t32 in zip(got, ref64[:3], ref32[:3], BOUND64, BOUND32):
        assert rel(a, b64) < t64 and rel(a, b32) < t32, (rel(a, b64), rel(a, b32))
    return ref64[3]


# H and W odd and not multiples of a workgroup's 256 pixels (several workgroups, planes crossing workgroup edges), axes of
# length 1 and 2, C > 1 with distinct per-sample ths
SHAPES = [(3, 2, 17, 19), (2, 3, 1, 23), (1, 2, 2, 9), (2, 2, 5, 9, 7), (1, 1, 2, 1, 6), (1, 1, 3, 4, 2)]


def warm_state(shape, seed):
    """a warm start with nonzero r2 / u2, so every term of the update is exercised from the first iteration"""
    g = torch.Generator().manual_seed(seed)
    nd = len(shape) - 2
    y = torch.rand(shape, generator=g)
    x0 = y + 0.05 * torch.randn(shape, generator=g)
    r0 = 0.002 * torch.randn(*shape, nd, generator=g)
    u0 = 0.01 * torch.randn(*shape, nd * nd, generator=g)
    return y, x0, r0, u0


@pytest.mark.parametrize("shape", SHAPES)
def test_cp_fixed_iterations(shape):
    """crit = 0: every enqueued iteration runs; x2 / r2 / u2 against the fp64 restatement, per-sample thresholds"""
    y, x0, r0, u0 = warm_state(shape, len(shape) + shape[-1])
    B = shape[0]
    lam = torch.linspace(0.05, 0.3, B)
    x, r, u, it, done = run_cp(y, lam, x0, r0, u0, 30, 0.0)
    assert (it, done) == (30, 0)
    assert assert_matches((x, r, u), y, lam, x0, r0, u0, 30) == 30


@pytest.mark.parametrize("shape", [(3, 2, 17, 19), (2, 2, 5, 9, 7)])
def test_cp_cold_start(shape):
    """the reference's first call: x2 = y, r2 = u2 = 0"""
    g = torch.Generator().manual_seed(5)
    y = torch.rand(shape, generator=g)
    lam = torch.linspace(0.1, 0.4, shape[0])
    r0, u0 = zeros_state(shape)
    x, r, u, it, _ = run_cp(y, lam, y, r0, u0, 20, 0.0)
    assert it == 20
    assert_matches((x, r, u), y, lam, y, r0, u0, 20)


@pytest.mark.parametrize("shape", [(2, 2, 17, 19), (1, 2, 5, 9, 7)])
def test_cp_early_stop_and_noop_after_done(shape):
    """the stopping rule of tgv.py:162-171 over the whole batch; launches after the flag leave the result (and the iteration
    count) exactly where the reference breaks"""
    y, x0, r0, u0 = warm_state(shape, 7)
    lam = torch.full((shape[0],), 0.2)
    crit = 2e-3
    rit = r_tgv_prox(y.double(), lam.double(), x0.double(), r0.double(), u0.double(), 400, crit)[3]
    assert 3 < rit < 400
    x, r, u, it, done = run_cp(y, lam, x0, r0, u0, rit + 9, crit)
    assert done == 1 and it == rit
    assert assert_matches((x, r, u), y, lam, x0, r0, u0, 400, crit) == rit


def test_cp_no_stop_before_index_2():
    """the test only applies from iteration index 2 on: with crit = inf the third iteration stops the loop"""
    y, x0, r0, u0 = warm_state((1, 1, 6, 7), 9)
    lam = torch.tensor([0.1])
    x, r, u, it, done = run_cp(y, lam, x0, r0, u0, 10, float("inf"))
    assert (it, done) == (3, 1)
    assert assert_matches((x, r, u), y, lam, x0, r0, u0, 10, float("inf")) == 3


@pytest.mark.parametrize("shape", SHAPES)
def test_epsilon_and_adjoint(shape):
    l = lib()
    g = torch.Generator().manual_seed(11)
    nd, B, C, D, H, W = geo(shape)
    v = torch.randn(*shape, nd, generator=g)
    u = torch.randn(*shape, nd * nd, generator=g)
    ev = torch.empty(*shape, nd * nd)
    check(l.dinv_tgv_epsilon(nd, B * C, D, H, W, E.p(v), E.p(ev), None))
    assert torch.allclose(ev.double(), r_epsilon(v.double()), atol=1e-6)
    au = torch.empty(*shape, nd)
    check(l.dinv_tgv_epsilon_adjoint(nd, B * C, D, H, W, E.p(u), E.p(au), None))
    assert torch.allclose(au.double(), r_epsilon_adjoint(u.double()), atol=1e-6)
    lhs, rhs = float((ev.double() * u.double()).sum()), float((v.double() * au.double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * ev.double().norm() * u.double().norm()
    with emu_backend():                                          # the product's wrappers make the same calls
        assert torch.equal(htgv.epsilon(v), ev) and torch.equal(htgv.epsilon_adjoint(u), au)


def test_argument_checks():
    l = lib()
    v = torch.zeros(1, 1, 4, 4, 2)
    out = torch.empty(1, 1, 4, 4, 4)
    assert l.dinv_tgv_epsilon(4, 1, 1, 4, 4, E.p(v), E.p(out), None) != 0
    assert b"nd must be 2 or 3" in l.dinv_last_error()
    assert l.dinv_tgv_epsilon(2, 1, 2, 4, 4, E.p(v), E.p(out), None) != 0          # 2-D with D != 1
    assert l.dinv_tgv_epsilon_adjoint(3, 1, 1 << 10, 1 << 10, 256, E.p(out), E.p(v), None) != 0
    assert b"too large" in l.dinv_last_error()
    y = torch.zeros(1, 1, 4, 4)
    x = torch.zeros(1, 1, 4, 4)
    part = torch.empty(64)
    st = torch.zeros(2, dtype=torch.int32)
    lam = torch.ones(1)
    r = torch.zeros(1, 1, 4, 4, 2)
    r2 = torch.zeros(1, 1, 4, 4, 2)
    u = torch.zeros(1, 1, 4, 4, 4)
    u2 = torch.zeros(1, 1, 4, 4, 4)
    z = torch.zeros(1, 1, 4, 4)
    w = torch.zeros(1, 1, 4, 4, 2)
    assert l.dinv_tgv_cp_iter(2, 1, 1, 1, 4, 4, E.p(x), E.p(x), E.p(r), E.p(r2), E.p(u), E.p(u2), E.p(y), E.p(lam), E.p(lam),
                              0.01, 1.0, 1.99, 0.0, E.p(z), E.p(w), E.p(part), E.p(st), None) != 0
    assert b"distinct" in l.dinv_last_error()
    ub = torch.zeros(1 + 16 * 4)
    assert l.dinv_tgv_cp_iter(2, 1, 1, 1, 4, 4, E.p(x), E.p(z), E.p(r), E.p(r2), E.p(u), E.p(ub[1:]), E.p(y), E.p(lam),
                              E.p(lam), 0.01, 1.0, 1.99, 0.0, E.p(torch.zeros(16)), E.p(w), E.p(part), E.p(st), None) != 0
    assert b"aligned" in l.dinv_last_error()
