"""SpaceVaryingBlur on the device: the whole case table of tests/svblur_cases.py through the gfx950 library on guarded device
buffers (the cases the emulation skips included), the class, autograd and golden checks on cuda:0, and one PGD + TVPrior loop
against the golden reconstruction of the reference."""
import pytest
import torch

import svblur_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def runner(dev):
    import deepinv_amd.hip as H
    from deepinv_amd.hip import conv as hc

    return S.Runner(hc._l(), dev, lambda: H.stream_ptr(dev))


@pytest.mark.parametrize("item", S.CASES, ids=S.item_id)
def test_product_convolution_path(runner, item):
    S.run_case(runner, *item)


@pytest.mark.parametrize("item", S.refusals(), ids=lambda i: i[0])
def test_bad_arguments_are_refused(runner, item):
    S.run_refusal(runner, item)


def test_empty_batch_launches_nothing(runner):
    S.run_empty_batch(runner)


def test_class(dev):
    S.check_class(dev)


def test_autograd(dev):
    S.check_autograd(dev)


def test_golden_product(dev):
    S.check_golden_product(S.golden(), dev)


def test_pgd_tv_golden(dev):
    """PGD + TVPrior, 10 iterations on a 1 x 1 x 48 x 40 image with a generated reflect-padded operator (K = 5, 9 x 9 filters)
    against the reference's fp32 reconstruction, in the l2 norm.  Allowed: the fp32-against-fp64 spread of the REFERENCE's own
    loop, stored by the golden script (3.3e-5 of |rec| = 22.1), plus the counted bound of the operator per iteration.  The
    gradient step I - A^T A (stepsize 1, |A| <= 1) and the proximal step do not expand l2 distances, so what an iteration adds
    is at most the operator's own error, | gamma_(n_A) |A||x| | + | gamma_(n_AT) |A|^T |r| | with n_A = K fh fw + 1 and
    n_AT = 9 fh fw + K (tests/svblur_cases.py), evaluated on the final iterate and summed over the 10 iterations."""
    import deepinv_amd as dinv

    gold = S.golden()
    h, w, y = (torch.from_numpy(gold[f"pgd_{n}"]) for n in ("filters", "multipliers", "y"))
    K, fh, fw = h.shape[2:]
    assert (K, fh, fw) == (5, 9, 9) and tuple(y.shape) == (1, 1, 48, 40)
    p = dinv.physics.SpaceVaryingBlur(filters=h, multipliers=w, padding="reflect", device=dev)
    m = dinv.optim.PGD(prior=dinv.optim.TVPrior(n_it_max=20), data_fidelity=dinv.optim.L2(), stepsize=1.0, lambda_reg=0.02, max_iter=10,
                       early_stop=False)
    with torch.no_grad():
        rec = m(y.to(dev), p).cpu().double()
    ref = torch.from_numpy(gold["pgd_rec"]).double()
    hd, wd = h.double(), w.double()
    ax = S.ref_A(ref.abs(), wd.abs(), hd.abs(), "reflect")
    r = (S.ref_A(ref, wd, hd, "reflect") - y.double()).abs()
    per_iter = float((S.gamma(K * fh * fw + 1) * S.ref_AT(ax, wd.abs(), hd.abs(), "reflect", (48, 40))).norm()) + \
        float((S.gamma(9 * fh * fw + K) * S.ref_AT(r, wd.abs(), hd.abs(), "reflect", (48, 40))).norm())
    tol = float(gold["pgd_spread_l2"]) + 10 * per_iter
    err = float((rec - ref).norm())
    print(f"PGD: |rec - golden|_2 = {err:.3g}, allowed {tol:.3g} (spread {float(gold['pgd_spread_l2']):.3g}, counted {10 * per_iter:.3g})")
    assert err <= tol
    assert float((rec - y.double()).norm()) > 10 * tol          # the loop moved
