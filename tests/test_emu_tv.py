"""Total-variation kernels (deepinv_amd/csrc/tv.hip) on the host emulation, on small odd shapes, against a float64 PyTorch
restatement of the reference (deepinv/models/tv.py:86-218, deepinv/optim/prior.py:485-612): the Chambolle-Pock iteration
with its device stopping rule and ping-pong buffers, the finite differences, their adjoint, TVPrior.fn and grad."""
import pytest
import torch

import emu_lib as E
from emu_backend import emu_backend
from emu_lib import check, lib
from variational_cases import r_nabla, r_nabla_adjoint, r_tv_prox      # the float64 restatement of the reference

from deepinv_amd.hip import tv as htv


def geo(shape):
    return (2, shape[0], shape[1], 1, shape[2], shape[3]) if len(shape) == 4 else (3, *shape)


def run_cp(y, lam, x2, u2, n_launch, crit, aniso):
    """n_launch iterations enqueued on the emulation (no host polling: launches after convergence must be no-ops)"""
    l = lib()
    nd, B, C, D, H, W = geo(y.shape)
    xa, xb = x2.clone(), torch.empty_like(x2)
    ua, ub = u2.clone(), torch.empty_like(u2)
    part = torch.empty(2 * l.dinv_tv_cp_partials(y.numel()))
    st = torch.zeros(2, dtype=torch.int32)
    sigma = 1 / 0.01 / 2 ** (y.ndim - 1)
    for _ in range(n_launch):
        check(l.dinv_tv_cp_iter(nd, B, C, D, H, W, E.p(xa), E.p(xb), E.p(ua), E.p(ub), E.p(y), E.p(lam), int(aniso), 0.01, sigma,
                                1.99, crit, E.p(part), E.p(st), None))
    it = int(st[1])
    return (xa, xb)[it & 1], (ua, ub)[it & 1], it, int(st[0])


SHAPES = [(3, 2, 17, 19), (1, 1, 5, 9, 7)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("aniso", [0, 1])
def test_cp_fixed_iterations(shape, aniso):
    """crit = 0: every enqueued iteration runs; x2 / u2 against the restatement, per-sample thresholds"""
    g = torch.Generator().manual_seed(len(shape) + aniso)
    y = torch.rand(shape, generator=g)
    B, nd = shape[0], len(shape) - 2
    lam = torch.linspace(0.05, 0.2, B)
    x, u, it, done = run_cp(y, lam, y, torch.zeros(*shape, nd), 25, 0.0, aniso)
    rx, ru, rit = r_tv_prox(y.double(), lam.double(), y.double(), torch.zeros(*shape, nd, dtype=torch.float64), 25, 0.0, aniso)
    assert (it, done, rit) == (25, 0, 25)
    assert float((x.double() - rx).norm() / rx.norm()) < 1e-5
    assert float((u.double() - ru).norm() / ru.norm()) < 1e-4          # the dual sees x's rounding times 2 sigma = 25
    fx, fu, _ = r_tv_prox(y, lam, y, torch.zeros(*shape, nd), 25, 0.0, aniso)      # the same restatement in fp32
    assert float((x - fx).norm() / fx.norm()) < 1e-6 and float((u - fu).norm() / fu.norm()) < 1e-5


@pytest.mark.parametrize("shape", SHAPES)
def test_cp_early_stop_and_noop_after_done(shape):
    """the stopping rule of tv.py:141-148 over the whole batch, from a warm start; launches after the flag leave the result
    (and the iteration count) exactly where the reference breaks"""
    g = torch.Generator().manual_seed(7)
    y = torch.rand(shape, generator=g)
    B, nd = shape[0], len(shape) - 2
    lam = torch.full((B,), 0.1)
    u0 = 0.05 * torch.randn(*shape, nd, generator=g)
    x0 = y + 0.01 * torch.randn(shape, generator=g)
    rx, _, rit = r_tv_prox(y.double(), lam.double(), x0.double(), u0.double(), 400, 1e-3, 0)
    assert 3 < rit < 400
    x, _, it, done = run_cp(y, lam, x0, u0, rit + 9, 1e-3, 0)
    assert done == 1 and it == rit
    assert float((x.double() - rx).norm() / rx.norm()) < 1e-5


def test_cp_one_sample_keeps_the_batch_iterating():
    """rel_err is a batch norm (tv.py:141-143): a second sample changes when the first one stops"""
    g = torch.Generator().manual_seed(3)
    y1 = torch.rand(1, 1, 17, 19, generator=g)
    _, _, it1, _ = run_cp(y1, torch.tensor([0.1]), y1, torch.zeros(1, 1, 17, 19, 2), 1000, 1e-4, 0)
    y2 = torch.cat([y1, torch.rand(1, 1, 17, 19, generator=g)])
    lam = torch.tensor([0.1, 1.0])
    x2, _, it2, _ = run_cp(y2, lam, y2, torch.zeros(2, 1, 17, 19, 2), 1000, 1e-4, 0)
    rx, _, rit2 = r_tv_prox(y2.double(), lam.double(), y2.double(), torch.zeros(2, 1, 17, 19, 2, dtype=torch.float64), 1000,
                            1e-4, 0)
    assert it2 == rit2 and it2 != it1
    assert float((x2.double() - rx).norm() / rx.norm()) < 1e-5


@pytest.mark.parametrize("shape", SHAPES)
def test_nabla_adjoint_grad_fn(shape):
    l = lib()
    g = torch.Generator().manual_seed(11)
    nd, B, C, D, H, W = geo(shape)
    x = torch.randn(shape, generator=g)
    x.view(-1)[::5] = 0.0                                        # flat patches: |Dx| = 0 somewhere
    x[..., 2, :] = x[..., 1, :]
    v = torch.randn(*shape, nd, generator=g)
    gx = torch.empty(*shape, nd)
    check(l.dinv_tv_nabla(nd, B * C, D, H, W, E.p(x), E.p(gx), None))
    assert torch.allclose(gx.double(), r_nabla(x.double()), atol=1e-6)
    av = torch.empty(shape)
    check(l.dinv_tv_nabla_adjoint(nd, B * C, D, H, W, E.p(v), E.p(av), None))
    assert torch.allclose(av.double(), r_nabla_adjoint(v.double()), atol=1e-6)
    lhs, rhs = float((gx.double() * v.double()).sum()), float((x.double() * av.double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * gx.double().norm() * v.double().norm()
    gr = torch.empty(shape)
    check(l.dinv_tv_grad(nd, B * C, D, H, W, E.p(x), E.p(gr), None))
    dx = r_nabla(x.double())
    n = dx.norm(dim=-1, keepdim=True)
    ref = r_nabla_adjoint(torch.where(n > 0, dx / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(dx)))
    assert torch.allclose(gr.double(), ref, atol=1e-5)
    with emu_backend():                                          # the product's wrappers make the same calls
        assert torch.equal(htv.nabla(x), gx) and torch.equal(htv.nabla_adjoint(v), av) and torch.equal(htv.grad(x), gr)
    for mode in (0, 1):
        out = torch.empty(B)
        part = torch.empty(B * l.dinv_tv_fn_blocks(x.numel() // B))
        check(l.dinv_tv_fn(nd, mode, B, C, D, H, W, E.p(x), E.p(out), E.p(part), None))
        r = (dx.abs().sum(-1) if mode else dx.norm(dim=-1)).reshape(B, -1).sum(-1)
        assert torch.allclose(out.double(), r, rtol=1e-5)
        with emu_backend():
            assert torch.equal(htv.fn(x, l1=bool(mode)), out)


def test_argument_checks():
    l = lib()
    x = torch.zeros(1, 1, 4, 4)
    out = torch.empty(1, 1, 4, 4, 2)
    assert l.dinv_tv_nabla(4, 1, 1, 4, 4, E.p(x), E.p(out), None) != 0
    assert b"nd must be 2 or 3" in l.dinv_last_error()
    assert l.dinv_tv_nabla(2, 1, 2, 4, 4, E.p(x), E.p(out), None) != 0          # 2-D with D != 1
    y = torch.zeros(1, 1, 4, 4)
    part = torch.empty(64)
    st = torch.zeros(2, dtype=torch.int32)
    lam = torch.ones(1)
    assert l.dinv_tv_cp_iter(2, 1, 1, 1, 4, 4, E.p(x), E.p(x), E.p(out), E.p(out), E.p(y), E.p(lam), 0, 0.01, 12.5, 1.99, 0.0,
                             E.p(part), E.p(st), None) != 0
    assert b"distinct" in l.dinv_last_error()
