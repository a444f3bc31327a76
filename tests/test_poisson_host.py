"""Host logic of the Poisson-family noise models, likelihoods and the Anscombe wrapper, and their torch path on the CPU against the
reference's values in tests/golden/poisson.npz (tests/golden/make_golden_poisson.py; on the CPU these are the same formulas: 1e-6
relative)."""
import os

import numpy as np
import pytest
import torch

import deepinv_amd as dinv

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poisson.npz")
TOL = 1e-6


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def close(a, b, tol=TOL):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).norm()) <= tol * float(b.norm()), float((a - b).norm() / b.norm())


def test_exports():
    for name in ("PoissonNoise", "PoissonGaussianNoise", "LogPoissonNoise"):
        assert issubclass(getattr(dinv.physics, name), dinv.physics.NoiseModel)
    for name in ("PoissonLikelihoodDistance", "L1Distance", "LogPoissonLikelihoodDistance"):
        assert issubclass(getattr(dinv.optim, name), dinv.optim.Distance)
    for name in ("PoissonLikelihood", "L1", "LogPoissonLikelihood"):
        assert issubclass(getattr(dinv.optim, name), dinv.optim.DataFidelity)
    assert issubclass(dinv.models.AnscombeDenoiser, dinv.models.Denoiser)
    assert callable(dinv.models.generalized_anscombe_transform) and callable(dinv.models.inverse_generalized_anscombe_transform)


def test_constructor_buffers_and_update_parameters():
    n = dinv.physics.PoissonNoise(gain=0.25)
    assert set(dict(n.named_buffers())) == {"gain", "normalize"}
    assert n.gain.dtype == torch.float32 and float(n.gain) == 0.25 and n.normalize.dtype == torch.bool and bool(n.normalize)
    assert n.clip_positive is False
    n.update_parameters(gain=0.5, sigma=3.0, nothing=None)           # only what the model has
    assert float(n.gain) == 0.5 and not hasattr(n, "sigma")
    n.update_parameters(gain=torch.tensor([1.0, 2.0]))
    assert n.gain.tolist() == [1.0, 2.0] and "gain" in n.state_dict()
    pg = dinv.physics.PoissonGaussianNoise(gain=2, sigma=torch.tensor([0.1, 0.2]))
    assert set(dict(pg.named_buffers())) == {"gain", "sigma"} and float(pg.gain) == 2.0 and pg.min_gain == 1e-12
    lp = dinv.physics.LogPoissonNoise()
    assert set(dict(lp.named_buffers())) == {"N0", "mu"} and float(lp.N0) == 1024.0 and abs(float(lp.mu) - 0.02) < 1e-9
    lp.update_parameters(N0=100, mu=0.5)
    assert float(lp.N0) == 100.0 and float(lp.mu) == 0.5
    with pytest.raises(ValueError, match="Unsupported type for noise level"):
        dinv.physics.PoissonNoise(gain="1")
    base = dinv.physics.NoiseModel()
    assert float(base._float_to_tensor(3)) == 3.0 and base._float_to_tensor(None) is None
    u = dinv.physics.NoiseModel(rng=torch.Generator().manual_seed(0)).rand_like(torch.empty(1000), seed=3)
    assert 0 <= float(u.min()) and float(u.max()) < 1 and abs(float(u.mean()) - 0.5) < 0.05
    # GaussianNoise keeps its own parameter handling
    gn = dinv.physics.GaussianNoise(0.3)
    gn.update_parameters(sigma=0.7, gain=2.0)
    assert abs(float(gn.sigma) - 0.7) < 1e-7 and not hasattr(gn, "gain")


def test_error_messages():
    x = torch.rand(2, 1, 4, 4)
    with pytest.raises(ValueError, match="Input tensor for Poisson noise must be non-negative"):
        dinv.physics.PoissonNoise()(-x)
    with pytest.raises(ValueError, match="clip_positive=True"):
        dinv.physics.PoissonNoise()(-x)
    with pytest.raises(ValueError, match="Poisson noise gain must be positive."):
        dinv.physics.PoissonNoise(gain=0.0)(x)
    with pytest.raises(ValueError, match="Poisson-Gaussian noise gain must be positive."):
        dinv.physics.PoissonGaussianNoise(gain=-1.0, min_gain=-2.0)(x)
    with pytest.raises(ValueError, match="Input tensor for Poisson-Gaussian noise must be non-negative"):
        dinv.physics.PoissonGaussianNoise()(-x)
    assert torch.all(dinv.physics.PoissonNoise(clip_positive=True)(-x) == 0)
    assert torch.isfinite(dinv.physics.PoissonGaussianNoise(clip_positive=True)(-x)).all()


def test_cpu_torch_path_statistics_and_seeding():
    rng = torch.Generator().manual_seed(0)
    x = torch.full((4, 1, 100, 100), 3.0)
    n = dinv.physics.PoissonNoise(gain=0.5, rng=rng)
    y = n(x, seed=7)
    assert torch.equal(y, n(x, seed=7)) and not torch.equal(y, n(x))
    assert torch.equal(y * 2, (y * 2).round()) and abs(float(y.mean()) - 3.0) < 0.02 and abs(float(y.var()) - 1.5) < 0.05
    k = dinv.physics.PoissonNoise(gain=0.5, normalize=False, rng=rng)(x)
    assert torch.equal(k, k.round()) and abs(float(k.mean()) - 6.0) < 0.05
    # per-sample gain through forward(), Physics.forward and Physics.update
    gains = torch.tensor([0.1, 0.5, 1.0, 2.0])
    yb = n(x, gain=gains)
    for b in range(4):
        assert abs(float(yb[b].var()) - 3.0 * float(gains[b])) < 0.15 * 3.0 * float(gains[b])
    phys = dinv.physics.Denoising(dinv.physics.PoissonNoise(gain=1.0, rng=rng))
    assert abs(float(phys(x, gain=0.25).var()) - 0.75) < 0.05 and float(phys.noise_model.gain) == 0.25
    phys.update(gain=4.0)
    assert float(phys.noise_model.gain) == 4.0
    pg = dinv.physics.PoissonGaussianNoise(gain=0.5, sigma=0.2, rng=rng)
    ypg = pg(x)
    assert abs(float(ypg.mean()) - 3.0) < 0.02 and abs(float(ypg.var()) - (1.5 + 0.04)) < 0.05
    assert abs(float(pg(x, sigma=1.0).var()) - 2.5) < 0.08 and float(pg.sigma) == 1.0
    lp = dinv.physics.LogPoissonNoise(N0=1024.0, mu=0.02, rng=rng)
    yl = lp(torch.full((1, 1, 200, 200), 50.0))
    kk = 1024.0 * torch.exp(-0.02 * yl.double())
    assert float((kk - kk.round()).abs().max()) < 1e-2 and abs(float(yl.mean()) - 50.0) < 0.1
    with pytest.raises(ValueError):
        dinv.physics.PoissonNoise()(x, seed=1)            # a seed needs a generator (as for GaussianNoise)


def test_distances_and_fidelities_match_the_reference(gold):
    x, y = torch.from_numpy(gold["x"]), torch.from_numpy(gold["y"])
    gain, bkg, N0, mu = (float(gold[k]) for k in ("gain", "bkg", "N0", "mu"))
    physics = dinv.physics.Denoising(dinv.physics.ZeroNoise())
    assert dinv.optim.PoissonLikelihoodDistance().denormalize is False and dinv.optim.PoissonLikelihood().d.denormalize is True
    for denorm in (False, True):
        d = dinv.optim.PoissonLikelihoodDistance(gain=gain, bkg=bkg, denormalize=denorm)
        t = f"pl{int(denorm)}"
        close(d.fn(x, y), gold[f"{t}_fn"])
        close(d(x, y), gold[f"{t}_fn"])
        close(d.grad(x, y), gold[f"{t}_grad"])
        close(d.prox(x, y, gamma=0.7), gold[f"{t}_prox"])
    f = dinv.optim.PoissonLikelihood(gain=gain, bkg=bkg)
    assert f.normalize is True and f.gain == gain and f.bkg == bkg
    close(f.fn(x, y, physics), gold["plf_fn"])
    close(f.grad(x, y, physics), gold["plf_grad"])
    close(f.prox_d(x, y, gamma=1.3), gold["plf_prox_d"])
    d = dinv.optim.L1Distance()
    close(d.fn(x, y), gold["l1_fn"])
    assert torch.equal(d.grad(x, y), torch.from_numpy(gold["l1_grad"]))
    close(d.prox(x, y, gamma=0.4), gold["l1_prox"])
    f = dinv.optim.L1()
    close(f.fn(x, y, physics), gold["l1f_fn"])
    close(f.grad(x, y, physics), gold["l1f_grad"])
    xl, yl = x * 40, y * 40
    d = dinv.optim.LogPoissonLikelihoodDistance(N0=N0, mu=mu)
    close(d.fn(xl, yl), gold["lp_fn"])
    close(d.grad(xl.clone(), yl).detach(), gold["lp_grad"])
    f = dinv.optim.LogPoissonLikelihood(N0=N0, mu=mu)
    assert f.N0 == N0 and f.mu == mu
    close(f.fn(xl, yl, physics), gold["lpf_fn"])
    close(f.grad(xl.clone(), yl, physics).detach(), gold["lpf_grad"])
    # the shape of PoissonLikelihoodDistance.fn: the first term is summed over the whole batch (distance.py:231-233)
    d = dinv.optim.PoissonLikelihoodDistance(gain=gain, bkg=bkg)
    first = (-y * torch.log(x / gain + bkg)).sum()
    second = (x / gain + bkg - y).reshape(2, -1).sum(1)
    close(d.fn(x, y), first + second)


def test_l1_fidelity_prox_on_denoising_is_the_soft_threshold():
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(2, 1, 8, 8, generator=g), torch.randn(2, 1, 8, 8, generator=g)
    physics = dinv.physics.Denoising(dinv.physics.ZeroNoise())
    # (gamma = 1 with stepsize = 1: the reference hands the distance's prox its threshold positionally, data_fidelity.py:749, where
    # it is not read, so the inner threshold is the default 1 - reproduced as it is)
    out = dinv.optim.L1().prox(x, y, physics, gamma=1.0, stepsize=1.0, crit_conv=1e-7, max_iter=200)
    close(out, dinv.optim.L1Distance().prox(x, y, gamma=1.0), tol=1e-5)


class Shrink(dinv.models.Denoiser):
    def forward(self, u, sigma, **kwargs):
        return u / (1 + sigma * sigma)


def test_anscombe_matches_the_reference(gold):
    y = torch.from_numpy(gold["y"])
    gat, igat = dinv.models.generalized_anscombe_transform, dinv.models.inverse_generalized_anscombe_transform
    close(gat(y, 0.5, 0.1), gold["gat"])
    close(igat(torch.from_numpy(gold["gat"]), 0.5, 0.1), gold["igat"])
    den = dinv.models.AnscombeDenoiser(Shrink())
    close(den(y, 0.1, 0.5), gold["ansc"])
    close(den(y, 0.2), gold["ansc_none"])                                    # gain=None: the wrapped denoiser directly
    # per-sample sigma and gain over the whole batch equal the reference's sample-by-sample results
    sig, gain = torch.from_numpy(gold["ansc_b_sigma"]).float(), torch.from_numpy(gold["ansc_b_gain"]).float()
    close(den(y, sig, gain), gold["ansc_b"])
    close(den(y, sig.tolist(), gain.tolist()), gold["ansc_b"])
    with pytest.raises(ValueError, match="gain should be positive"):
        gat(y, -1.0, 0.1)
    with pytest.raises(ValueError, match="sigma should be positive"):
        igat(y, 1.0, torch.tensor([-0.1]))
    with pytest.raises(ValueError, match="does not match batch size"):
        den(y, torch.tensor([0.1, 0.2, 0.3]), 0.5)
    # the GAT stabilises the variance of Poisson-Gaussian data to gain^2
    rng = torch.Generator().manual_seed(1)
    noisy = dinv.physics.PoissonGaussianNoise(gain=0.2, sigma=0.05, rng=rng)(torch.full((1, 1, 200, 200), 4.0))
    assert abs(float(gat(noisy, 0.2, 0.05).std()) - 0.2) < 0.01


def test_golden_file_is_small():
    sizes = [os.path.getsize(os.path.join(os.path.dirname(GOLD), f)) for f in os.listdir(os.path.dirname(GOLD)) if f.endswith(".npz")]
    assert os.path.getsize(GOLD) <= max(s for s in sizes) and os.path.getsize(GOLD) < 1 << 20
