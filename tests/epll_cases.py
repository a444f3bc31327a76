"""Shared by tests/test_emu_epll.py (the host emulation, through emu_backend) and tests/test_epll_gpu.py (the MI355X): the checks
of GaussianMixtureModel, EPLL and EPLLDenoiser through the Python layers against tests/golden/epll.npz, which
tests/golden/make_golden_epll.py wrote from the real reference in float32 on the CPU.

Parity is the project's bound, 1e-4 relative (l2) to the reference's CPU result; the golden file carries the reference's own
fp32-against-fp64 spread (5e-5 absolute on the scores, below 1e-6 on the images) and the smallest top-two score gap of every
classification, at least 100 times the reference's fp32 score error, so no golden sits on a classification flip.

What these goldens do not show: the inputs were chosen, from the reference alone, so that this holds - mixtures at the scale of
images in [0, 1] (eigenvalues 0.1 logspace(-1, 0), not the ill-conditioned logspace(-3, 0)), the 37 of 96 rows with the largest
fp64 gaps, the first seeded image whose run is clear of a flip.  They pin the Python layers and the wiring against the reference
on well-separated, well-conditioned inputs; they are not parity in general.  The ill-conditioned regime and patches near a tie are
covered by the fp64 case table of tests/gmm_cases.py, where the reference's own fp32 arithmetic could not serve as the truth."""
import os

import numpy as np
import torch

import deepinv_amd as dinv

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epll.npz"))
TOL = 1e-4


def rel(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def state_dict(tag):
    return {str(k): torch.from_numpy(GOLD[f"{tag}_sd_{k}"]) for k in GOLD[f"{tag}_sd_keys"]}


def gmm(tag, device):
    sd = state_dict(tag)
    K, d = sd["mu"].shape
    m = dinv.optim.GaussianMixtureModel(K, d, device=device)
    m.load_state_dict(sd, strict=True)
    return m.to(device)


def t(name, device):
    return torch.from_numpy(GOLD[name]).to(device)


def check_rows(device):
    m = gmm("a", device)
    x = t("rows_x", device)
    assert rel(m.component_log_likelihoods(x), GOLD["rows_cll"]) <= TOL
    assert rel(m(x), GOLD["rows_nll"]) <= TOL
    assert m.classify(x).cpu().tolist() == GOLD["rows_cls"].tolist()
    m.set_cov_reg(float(GOLD["rows_reg"]))
    assert rel(m.component_log_likelihoods(x, cov_regularization=True), GOLD["rows_reg_cll"]) <= TOL
    assert m.classify(x, cov_regularization=True).cpu().tolist() == GOLD["rows_reg_cls"].tolist()
    assert m.classify(x).dtype == torch.int64
    nll = dinv.optim.EPLL(GMM=m, patch_size=4).negative_log_likelihood(x[:36].reshape(2, 18, 1, 4, 4))
    assert nll.shape == (2, 18) and rel(nll.reshape(-1), GOLD["rows_nll"][:36]) <= TOL


def denoiser(tag, device):
    m = gmm(tag, device)
    C = {"a": 1, "b": 3}[tag]
    p = int(round((m.dimension / C) ** 0.5))
    return dinv.models.EPLLDenoiser(GMM=m, patch_size=p, channels=C, device=device).to(device)


def check_denoiser(tag, device):
    den = denoiser(tag[-1], device)
    y, sigma = t(f"{tag}_y", device), t(f"{tag}_sigma", device)
    out = den(y, sigma)
    err = rel(out, GOLD[f"{tag}_out"])
    print(f"{tag}: relative error {err:.3g}, the reference's own fp32 - fp64 spread {float(GOLD[f'{tag}_spread']):.3g}")
    assert err <= TOL
    assert torch.equal(out, den(y, sigma)), "two identical calls differ"
    assert torch.equal(out, den(y, sigma, batch_size=7)), "batch_size changed the output"
    for b in range(y.shape[0]):
        assert torch.equal(out[b:b + 1], den(y[b:b + 1], sigma[b:b + 1])), f"image {b} alone differs from the batched call"
    assert torch.equal(out, den(y, sigma.cpu().tolist())), "sigma as a list differs from sigma as a tensor"


def check_blur(device):
    """EPLL with a BlurFFT physics: the conjugate-gradient path"""
    physics = dinv.physics.BlurFFT(img_size=(1, 19, 22), filter=t("blur_filter", device), device=device)
    model = dinv.optim.EPLL(GMM=gmm("a", device), patch_size=4, channels=1, device=device)
    y = t("blur_y", device)
    out = model(y, physics, sigma=float(GOLD["blur_sigma"]))
    err = rel(out, GOLD["blur_out"])
    print(f"blur: relative error {err:.3g}, the reference's own fp32 - fp64 spread {float(GOLD['blur_spread']):.3g}")
    assert err <= TOL
    assert torch.equal(out, model(y, physics, sigma=float(GOLD["blur_sigma"])))


def check_pnp(device):
    """five iterations of PGD with PnP(EPLLDenoiser) on a Denoising physics"""
    den = denoiser("a", device)
    physics = dinv.physics.Denoising(dinv.physics.GaussianNoise(0.1), device=device)
    y = t("den_a_y", device)
    model = dinv.optim.PGD(data_fidelity=dinv.optim.L2(), prior=dinv.optim.PnP(den), stepsize=1.0, g_param=0.05, max_iter=5)
    out = model(y, physics)
    assert out.shape == y.shape and bool(torch.isfinite(out).all())
    assert float((out - y).abs().max()) > 1e-3, "the denoiser did nothing"
