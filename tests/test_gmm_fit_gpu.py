"""GaussianMixtureModel.fit on the MI355X against the real reference's float64 fit (tests/golden/gmm_fit.npz, written by
tests/golden/make_golden_gmm_fit.py): every iteration's weights, means, covariances and objective within FOUR times the reference's
own fp32-against-fp64 spread of that quantity, stored beside the golden.  Why four: two fp32 computations with different summation
orders each sit about one spread from fp64, the spread is a maximum over a single draw, and on the overlapping records EM
amplifies both alike.  Each comparison prints its distance over the spread before it asserts (DESIGN 3.17 records them).
Then the stopping criterion, the state dict, EPLLDenoiser on a fitted model, data_init from a short first batch, CPU against
device batches and tuple batches."""
import os

import numpy as np
import pytest
import torch

import deepinv_amd as dinv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmm_fit.npz"))
NAMES = ("weights", "mu", "cov", "objective")


def t(key):
    return torch.from_numpy(GOLD[key])


def batches(tag, device="cpu"):
    return [b.to(device) for b in t(f"{tag}_x").split(int(GOLD[f"{tag}_batch"]))]


def traced_fit(tag, **kw):
    """fit on the golden's rows: (the model, one (weights, mu, cov, objective) per iteration, fp64 on the host)"""
    x = t(f"{tag}_x")
    m = dinv.optim.GaussianMixtureModel(int(GOLD[f"{tag}_K"]), x.shape[1], device=DEV)
    if f"{tag}_init_mu" in GOLD:
        m.set_weights(t(f"{tag}_init_weights"))
        m.mu.data = t(f"{tag}_init_mu").to(DEV)
        m.set_cov(t(f"{tag}_init_cov"))
    log, step = [], m._EM_step

    def traced(*a, **k):
        res = step(*a, **k)
        log.append(tuple(torch.as_tensor(v, dtype=torch.float64).clone() for v in res))
        return res

    m._EM_step = traced
    m.fit(batches(tag), cov_regularization=1e-5, **kw)
    return m, log


def compare(tag, m, log):
    iters = int(GOLD[f"{tag}_iters"])
    assert len(log) == iters, f"{tag}: {len(log)} iterations, the reference ran {iters}"
    ratios = {}
    for i, name in enumerate(NAMES):
        got, want, spread = torch.stack([it[i] for it in log]), t(f"{tag}_{name}_f64"), float(GOLD[f"{tag}_{name}_spread"])
        ratios[name] = float((got - want).abs().max()) / spread
    print(f"{tag}: distance to the reference's fp64 fit over its own fp32 spread: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    # the fitted model holds the last iteration, rounded to fp32 once
    last = log[-1]
    assert torch.equal(m.mu.cpu(), last[1].float()) and torch.equal(m.get_cov().cpu(), last[2].float())
    assert torch.allclose(m.get_weights().cpu().double(), last[0] / last[0].sum(), atol=1e-7, rtol=0)
    for name, v in ratios.items():
        assert v <= 4.0, f"{tag}: {name} is {v:.3g} spreads from the reference's fp64 result (bound 4)"


@pytest.mark.parametrize("tag,kw", [("a", dict(max_iters=5)), ("b3", dict(max_iters=8)), ("b4", dict(max_iters=8)),
                                    ("c", dict(max_iters=1, data_init=False))])
def test_fit_against_the_reference(tag, kw):
    compare(tag, *traced_fit(tag, **kw))


def test_stopping_criterion_stops_where_the_reference_does():
    m, log = traced_fit("d", max_iters=40, stopping_criterion=float(GOLD["d_threshold"]))
    compare("d", m, log)


@pytest.fixture(scope="module")
def fitted():
    return traced_fit("b4", max_iters=3)[0]


def test_state_dict_loads_strict(fitted):
    fresh = dinv.optim.GaussianMixtureModel(fitted.n_components, fitted.dimension, device=DEV)
    fresh.load_state_dict(fitted.state_dict(), strict=True)
    x = t("b4_x").to(DEV)
    assert torch.equal(fresh(x), fitted(x)) and torch.equal(fresh.mu, fitted.mu) and torch.equal(fresh.get_cov(), fitted.get_cov())


def test_fitted_model_drives_the_denoiser(fitted):
    den = dinv.models.EPLLDenoiser(GMM=fitted, pretrained=None, patch_size=3, channels=1)
    y = torch.rand(1, 1, 12, 13, generator=torch.Generator().manual_seed(0)).to(DEV)
    out = den(y, 0.05)
    assert out.shape == y.shape and bool(torch.isfinite(out).all())


def test_data_init_from_a_short_first_batch():
    x = t("b4_x")
    data = [x[:2], x[2:130], x[130:]]
    runs = []
    for _ in range(2):
        torch.manual_seed(7)
        m = dinv.optim.GaussianMixtureModel(4, x.shape[1], device=DEV)
        m.fit(data, max_iters=0)
        runs.append(m.mu.cpu().clone())
    assert torch.equal(runs[0][:2], x[:2]) and bool(torch.isfinite(runs[0]).all())
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0][2], runs[0][3])


def test_cpu_and_device_batches_give_the_same_bits():
    res = []
    for device in ("cpu", DEV):
        m = dinv.optim.GaussianMixtureModel(4, 9, device=DEV)
        m.fit(batches("b4", device), max_iters=3)
        res.append([v.cpu().clone() for v in m.state_dict().values()])
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_tuple_batches():
    plain = dinv.optim.GaussianMixtureModel(4, 9, device=DEV)
    plain.fit(batches("b4"), max_iters=2)
    tup = dinv.optim.GaussianMixtureModel(4, 9, device=DEV)
    tup.fit([(b, torch.zeros(b.shape[0], dtype=torch.long)) for b in batches("b4")], max_iters=2)
    lst = dinv.optim.GaussianMixtureModel(4, 9, device=DEV)
    lst.fit([[b, None] for b in batches("b4")], max_iters=2)
    assert torch.equal(plain.mu, tup.mu) and torch.equal(plain.get_cov(), tup.get_cov()) and torch.equal(plain.mu, lst.mu)
