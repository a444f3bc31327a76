"""The Poisson-family noise models and likelihoods on the GPU (csrc/random.hip: dinv_poisson_noise; csrc/elementwise.hip:
dinv_fidelity_pointwise) through the public classes: distribution tests of the device sampler (the design of
tests/test_emu_poisson.py), two-sample tests against histograms of the reference's samplers, the fidelity classes against the
reference's values (tests/golden/poisson.npz) and one PGD + PoissonLikelihood + TVPrior loop against the reference's
(loop parity 1e-4 relative, BASELINE.json)."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_err
from test_emu_poisson import N, chi_square_vs_pmf
from test_emu_random import chi_square_vs_reference

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poisson.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("lam", [0.01, 0.5, 3.0, 9.99, 10.0, 10.01, 30.0, 1e3, 1e5])
def test_poisson_noise_distribution(dev, lam):
    import deepinv_amd as dinv

    lam32 = float(np.float32(lam))
    noise = dinv.physics.PoissonNoise(gain=1.0, normalize=False, rng=torch.Generator(dev).manual_seed(11))
    k = noise(torch.full((N,), lam32, device=dev)).cpu().numpy()
    assert np.all(k >= 0) and np.all(k == np.round(k))
    stat, df, bound = chi_square_vs_pmf(k, lam32)
    print(f"lambda = {lam32!r}: chi-square {stat:.1f}, df {df}, bound {bound:.1f}")
    assert stat < bound, (lam32, stat, df, bound)


def test_moments_at_a_very_large_rate(dev):
    import deepinv_amd as dinv

    lam = 1e6
    k = dinv.physics.PoissonNoise(normalize=False)(torch.full((N,), lam, device=dev)).double().cpu().numpy()
    assert abs(k.mean() - lam) < 5 * math.sqrt(lam / N) and abs(k.var() / lam - 1) < 0.02


def test_generators_seeds_and_per_sample_gains(dev):
    import deepinv_amd as dinv

    x = torch.rand(4, 2, 64, 64, device=dev) * 20
    rng = torch.Generator(dev)
    noise = dinv.physics.PoissonNoise(gain=0.5, rng=rng)
    y = noise(x, seed=3)
    assert torch.equal(y, noise(x, seed=3)) and not torch.equal(y, noise(x))             # seed= ; the generator advances
    assert torch.equal(y * 2, (y * 2).round()) and y.shape == x.shape and y.dtype == torch.float32
    before = rng.get_offset()
    noise(x)
    assert rng.get_offset() - before == x.numel()                                       # one counter per element
    plain = dinv.physics.PoissonNoise(gain=0.5)                                          # the default generator
    torch.manual_seed(5)
    a = plain(x)
    b = plain(x)
    torch.manual_seed(5)
    assert torch.equal(plain(x), a) and not torch.equal(a, b)
    gains = torch.tensor([0.05, 0.5, 1.0, 4.0], device=dev)
    xb = torch.full((4, 1, 200, 250), 6.0, device=dev)
    for normalize in (True, False):
        yb = dinv.physics.PoissonNoise(gain=gains, normalize=normalize, rng=rng)(xb)
        for b_ in range(4):
            g = float(gains[b_])
            k = (yb[b_] / g if normalize else yb[b_]).double().cpu().numpy().ravel()
            assert np.allclose(k, np.round(k), atol=1e-3)
            stat, df, bound = chi_square_vs_pmf(np.round(k), float(np.float32(6.0) / np.float32(g)))
            assert stat < bound, (normalize, b_, stat, df, bound)
    assert float(noise(xb, gain=gains)[3].var()) > 10 * float(noise(xb, gain=gains)[0].var())       # override in forward()
    assert torch.equal(noise.gain, gains)


def test_physics_forward_on_camera_and_tomography(dev):
    import deepinv_amd as dinv

    rng = torch.Generator(dev).manual_seed(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cam = dinv.physics.SinglePixelCamera(m=300, img_size=(1, 32, 32), device=dev,
                                             noise_model=dinv.physics.PoissonNoise(gain=0.01, clip_positive=True, rng=rng))
    x = torch.rand(2, 1, 32, 32, device=dev)
    y = cam(x)
    clean = cam.A(x)
    assert y.shape == clean.shape and torch.all(y >= 0) and float((y * 100 - (y * 100).round()).abs().max()) < 1e-2      # gain times a count
    assert 0 < float((y - clean.clamp_min(0)).abs().mean()) < 1.0
    y2 = cam(x, gain=0.001)                                            # Physics.forward(x, gain=...)
    assert abs(float(cam.noise_model.gain) - 0.001) < 1e-9
    assert float((y2 - clean.clamp_min(0)).abs().mean()) < float((y - clean.clamp_min(0)).abs().mean())
    cam.update(gain=0.5)                                                # physics.update(gain=...)
    assert float(cam.noise_model.gain) == 0.5
    N0, mu = 4096.0, 1 / 50.0
    tomo = dinv.physics.Tomography(angles=30, img_width=32, normalize=False, device=dev,
                                   noise_model=dinv.physics.LogPoissonNoise(N0=N0, mu=mu, rng=rng))
    img = torch.rand(2, 1, 32, 32, device=dev)
    s = tomo(img)
    clean = tomo.A(img)
    assert s.shape == clean.shape and torch.isfinite(s).all()
    k = N0 * torch.exp(-s.double() * mu)
    assert float((k - k.round()).abs().max()) < 0.05
    # the noise level: y = -log(k / N0) / mu with k ~ Poisson(lam), lam = N0 exp(-mu x) >= 2500 here, has standard deviation
    # 1 / (mu sqrt(lam)) up to O(1 / lam) (delta method).  The rms of 2760 residuals estimates the rms of that prediction to
    # 1 / sqrt(2 * 2760) = 1.3 % (one sigma); 10 % is seven sigma
    pred = torch.exp(clean.double() * mu / 2) / (mu * N0 ** 0.5)
    ratio = float((s.double() - clean.double()).square().mean().sqrt() / pred.square().mean().sqrt())
    print("log-Poisson sinogram: rms residual / predicted", ratio)
    assert abs(ratio - 1) < 0.1


def test_negative_input_raises_unless_clipped(dev):
    import deepinv_amd as dinv

    rng = torch.Generator(dev).manual_seed(0)
    x = torch.rand(2, 1, 16, 16, device=dev)
    x[1, 0, 3, 3] = -0.5
    noise = dinv.physics.PoissonNoise(gain=0.1, rng=rng)
    off = rng.get_offset()
    with pytest.raises(ValueError, match="Input tensor for Poisson noise must be non-negative"):
        noise(x)
    assert rng.get_offset() == off                                       # as in the reference, nothing was drawn
    with pytest.raises(ValueError, match="Poisson noise gain must be positive."):
        dinv.physics.PoissonNoise(gain=torch.tensor([1.0, 0.0]))(x.abs())
    with pytest.raises(ValueError, match="Input tensor for Poisson-Gaussian noise must be non-negative"):
        dinv.physics.PoissonGaussianNoise(gain=0.1, sigma=0.1)(x)
    y = dinv.physics.PoissonNoise(gain=0.1, clip_positive=True, rng=rng)(x)
    assert torch.isfinite(y).all() and float(y[1, 0, 3, 3]) == 0
    assert torch.isfinite(dinv.physics.PoissonGaussianNoise(gain=0.1, sigma=0.1, clip_positive=True)(x)).all()
    xn = x.abs()
    xn[0, 0, 0, 0] = float("nan")
    yn = dinv.physics.PoissonNoise(gain=0.1, rng=rng)(xn)
    assert torch.isnan(yn[0, 0, 0, 0]) and int(torch.isnan(yn).sum()) == 1


def _merge(a, b, least=25):
    """merge neighbouring cells left to right until the pooled count of each reaches `least`"""
    oa, ob, ca, cb = [], [], 0, 0
    for u, v in zip(a, b):
        ca, cb = ca + int(u), cb + int(v)
        if ca + cb >= least:
            oa.append(ca)
            ob.append(cb)
            ca = cb = 0
    if ca + cb and oa:
        oa[-1] += ca
        ob[-1] += cb
    return np.array(oa), np.array(ob)


def test_samplers_against_the_reference_histograms(gold, dev):
    """two-sample chi-square (test_emu_random.chi_square_vs_reference) of the device's log-Poisson and Poisson-Gaussian outputs
    against histograms of the reference's samplers on the same inputs"""
    import deepinv_amd as dinv

    rng = torch.Generator(dev).manual_seed(123)
    N0, mu = float(gold["N0"]), float(gold["mu"])
    y = dinv.physics.LogPoissonNoise(N0=N0, mu=mu, rng=rng)(torch.full((N,), float(gold["hist_lp_x"]), device=dev))
    k = torch.round(N0 * torch.exp(-mu * y.double())).long().cpu()
    assert int(k.max()) < 256
    a, b = _merge(torch.bincount(k, minlength=256).numpy(), gold["hist_lp_counts"])
    stat, df, bound = chi_square_vs_reference(a, N, b, int(gold["hist_lp_n"]))
    print(f"log-Poisson vs the reference's sampler: chi-square {stat:.1f}, df {df}, bound {bound:.1f}")
    assert stat < bound
    edges = gold["hist_pg_edges"]
    y = dinv.physics.PoissonGaussianNoise(gain=float(gold["hist_pg_gain"]), sigma=float(gold["hist_pg_sigma"]), rng=rng)(
        torch.full((N,), float(gold["hist_pg_x"]), device=dev)).cpu().numpy()
    a, b = _merge(np.histogram(np.clip(y, edges[0], edges[-1]), bins=edges)[0], gold["hist_pg_counts"])
    stat, df, bound = chi_square_vs_reference(a, N, b, int(gold["hist_pg_n"]))
    print(f"Poisson-Gaussian vs the reference's sampler: chi-square {stat:.1f}, df {df}, bound {bound:.1f}")
    assert stat < bound
    # moments of the Gaussian part: y - gain k for the same generator state
    rng.manual_seed(9)
    x = torch.full((N,), 10.0, device=dev)
    ypg = dinv.physics.PoissonGaussianNoise(gain=0.5, sigma=0.25, rng=rng)(x)
    rng.manual_seed(9)
    kk = dinv.physics.PoissonNoise(gain=0.5, normalize=False, rng=rng)(x)
    z = ((ypg - 0.5 * kk) / 0.25).cpu()
    assert abs(float(z.mean())) < 0.01 and abs(float(z.std()) - 1) < 0.01
    assert abs(float((z ** 3).mean())) < 0.03 and abs(float((z ** 4).mean()) - 3) < 0.06


def test_fidelities_against_the_reference(gold, dev):
    import deepinv_amd as dinv

    x, y = T(gold["x"], dev), T(gold["y"], dev)
    gain, bkg, N0, mu = (float(gold[k]) for k in ("gain", "bkg", "N0", "mu"))
    physics = dinv.physics.Denoising(dinv.physics.ZeroNoise())
    tol = 1e-5                                   # fp32 on both sides, different exp / log / division implementations
    res = {}
    for denorm in (False, True):
        d = dinv.optim.PoissonLikelihoodDistance(gain=gain, bkg=bkg, denormalize=denorm)
        t = f"pl{int(denorm)}"
        res[f"{t}_fn"], res[f"{t}_grad"], res[f"{t}_prox"] = d.fn(x, y), d.grad(x, y), d.prox(x, y, gamma=0.7)
    f = dinv.optim.PoissonLikelihood(gain=gain, bkg=bkg)
    res["plf_fn"], res["plf_grad"], res["plf_prox_d"] = f.fn(x, y, physics), f.grad(x, y, physics), f.prox_d(x, y, gamma=1.3)
    d = dinv.optim.L1Distance()
    res["l1_fn"], res["l1_grad"], res["l1_prox"] = d.fn(x, y), d.grad(x, y), d.prox(x, y, gamma=0.4)
    f = dinv.optim.L1()
    res["l1f_fn"], res["l1f_grad"] = f.fn(x, y, physics), f.grad(x, y, physics)
    xl, yl = x * 40, y * 40
    d = dinv.optim.LogPoissonLikelihoodDistance(N0=N0, mu=mu)
    res["lp_fn"], res["lp_grad"] = d.fn(xl, yl), d.grad(xl, yl)
    f = dinv.optim.LogPoissonLikelihood(N0=N0, mu=mu)
    res["lpf_fn"], res["lpf_grad"] = f.fn(xl, yl, physics), f.grad(xl, yl, physics)
    for key, val in res.items():
        e = rel_err(val, torch.from_numpy(gold[key]))
        print(f"{key}: {e:.2e}")
        assert val.shape == gold[key].shape and e <= tol, (key, e)
    assert not xl.requires_grad                                      # the kernel path leaves its input alone


def test_gradient_path_is_followed(dev):
    """an input that records a gradient (and a Tensor gamma) takes the torch expression: the same gradient as that expression"""
    import deepinv_amd as dinv

    g = torch.Generator().manual_seed(4)
    x0 = (torch.rand(2, 1, 8, 8, generator=g) * 3 + 0.5).to(dev)
    y = (torch.rand(2, 1, 8, 8, generator=g) * 3).to(dev)
    d = dinv.optim.PoissonLikelihoodDistance(gain=0.5, bkg=0.2, denormalize=True)
    x = x0.clone().requires_grad_()
    d.grad(x, y).square().sum().backward()
    xr = x0.clone().requires_grad_()
    (0.5 * (1 - (y / 0.5) / (xr / 0.5 + 0.2))).square().sum().backward()
    assert x.grad is not None and rel_err(x.grad, xr.grad) < 1e-6
    gamma = torch.tensor(0.7, device=dev, requires_grad=True)
    d.prox(x0, y, gamma=gamma).sum().backward()
    assert gamma.grad is not None and torch.isfinite(gamma.grad) and float(gamma.grad.abs()) > 0
    x = x0.clone().requires_grad_()
    dinv.optim.L1Distance().prox(x, y, gamma=0.3).sum().backward()
    assert rel_err(x.grad, ((x0 - y).abs() > 0.3).float()) < 1e-6
    lp = dinv.optim.LogPoissonLikelihoodDistance(N0=100.0, mu=0.5)
    x = x0.clone().requires_grad_()
    gl = lp.grad(x, y)                                               # autograd, as in the reference
    assert gl.requires_grad and rel_err(gl, lp.grad(x0, y)) < 1e-5   # ... equals the analytic kernel
    noisy = dinv.physics.PoissonGaussianNoise(gain=0.5, sigma=0.1, clip_positive=True)(x0.clone().requires_grad_())
    assert noisy.shape == x0.shape                                   # the torch expression serves a tensor that records a gradient


def test_pgd_poisson_likelihood_tv_on_the_camera(gold, dev):
    """the reference's PGD + PoissonLikelihood(gain, bkg > 0) + TVPrior reconstruction from the stored measurement"""
    import deepinv_amd as dinv

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p = dinv.physics.SinglePixelCamera(m=int(gold["pgd_m"]), img_size=(1, 32, 32), device=dev)
    model = dinv.optim.PGD(prior=dinv.optim.TVPrior(n_it_max=30),
                           data_fidelity=dinv.optim.PoissonLikelihood(gain=float(gold["pgd_gain"]), bkg=float(gold["pgd_bkg"])),
                           stepsize=100.0, lambda_reg=0.01, max_iter=30, early_stop=False)
    with torch.no_grad():
        rec = model(T(gold["pgd_y"], dev), p)
    e = rel_err(rec, torch.from_numpy(gold["pgd_rec"]))
    print("PGD + PoissonLikelihood + TVPrior vs reference", e)
    assert e <= 1e-4
