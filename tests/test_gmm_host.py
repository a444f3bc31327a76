"""Host-side checks of the Gaussian-mixture layers (no GPU, no kernel): the state dict against the reference's key list and a strict
load of the reference's own state dict (tests/golden/epll.npz), the tensors derived from the eigendecomposition, the operand pack
against fp64, the closed-form multiplicity against a brute-force count, the Python refusals, and that CPU tensors raise."""
import pytest
import torch

import deepinv_amd as dinv
import epll_cases as EC
from deepinv_amd.hip import HipExtensionError
from deepinv_amd.hip import gmm as G


def test_state_dict_keys_are_the_references():
    m = dinv.optim.GaussianMixtureModel(3, 4)
    assert list(m.state_dict().keys()) == [str(k) for k in EC.GOLD["a_sd_keys"]]
    assert list(dinv.optim.EPLL(n_components=3, patch_size=2).state_dict().keys()) == ["GMM." + str(k) for k in EC.GOLD["a_sd_keys"]]
    assert [k for k in dinv.models.EPLLDenoiser(n_components=3, patch_size=2).state_dict() if k.startswith("PatchGMM.GMM.")] == \
        ["PatchGMM.GMM." + str(k) for k in EC.GOLD["a_sd_keys"]]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_strict_load_rederives_the_maintained_tensors(tag):
    sd = EC.state_dict(tag)
    m = EC.gmm(tag, "cpu")
    cov = sd["_cov"].double()
    assert torch.equal(m._cov, sd["_cov"]) and torch.equal(m.mu, sd["mu"])
    assert torch.allclose(m._weights.double(), (sd["_weights"] / sd["_weights"].sum()).double(), atol=1e-7)
    # the reference's own fp32 inverse and log-determinant are in its state dict; ours come from the fp64 eigendecomposition
    assert EC.rel(m._cov_inv, torch.linalg.inv(cov)) < 1e-6 and EC.rel(m._cov_inv, sd["_cov_inv"]) < 1e-4
    assert EC.rel(m._logdet_cov, torch.logdet(cov)) < 1e-6 and EC.rel(m._logdet_cov, sd["_logdet_cov"]) < 1e-5
    m.set_cov_reg(0.05)
    r = float(torch.tensor(0.05, dtype=torch.float32))
    reg = cov + r * torch.eye(cov.shape[1], dtype=torch.float64)
    assert EC.rel(m._cov_reg, reg) < 1e-6 and EC.rel(m.get_cov_inv_reg(), torch.linalg.inv(reg)) < 1e-6
    assert EC.rel(m._logdet_cov_reg, torch.logdet(reg)) < 1e-6
    assert torch.equal(m.get_cov(), m._cov) and torch.equal(m.get_weights(), m._weights)


def test_operand_pack_against_fp64():
    sd = EC.state_dict("b")
    cov, mu, w = sd["_cov"].double(), sd["mu"].double(), sd["_weights"].double()
    K, d = mu.shape
    Wt, m, lam, logw = G.eigen_pack(cov, mu, w)
    Q = Wt.reshape(K, d, d).transpose(1, 2)
    eye = torch.eye(d, dtype=torch.float64)
    assert float((Q.transpose(1, 2) @ Q - eye).abs().max()) < 1e-12
    assert float((Q @ torch.diag_embed(lam.reshape(K, d)) @ Q.transpose(1, 2) - cov).abs().max()) < 1e-12
    assert float((m.reshape(K, d) - torch.einsum("kji,kj->ki", Q, mu)).abs().max()) < 1e-12
    assert torch.equal(logw, torch.log(w))
    ops = G.pack(cov, mu, w, "cpu")
    dp = G.padded_dim(d)
    assert dp == 28 and ops.Wt.shape == (K * dp, d) and ops.m.shape == ops.lam.shape == (K * dp,) and ops.Wt.dtype == torch.float32
    W3, m2, l2 = ops.Wt.reshape(K, dp, d), ops.m.reshape(K, dp), ops.lam.reshape(K, dp)
    assert torch.equal(W3[:, :d], Wt.reshape(K, d, d).float()) and torch.equal(m2[:, :d], m.reshape(K, d).float())       # rounded once
    assert torch.equal(l2[:, :d], lam.reshape(K, d).float()) and ops.lam_min == float(lam.float().min())
    assert not bool(W3[:, d:].any()) and not bool(m2[:, d:].any()) and bool((l2[:, d:] == 1).all())
    assert G.padded_dim(9) == 12 and [G.padded_dim(d) for d in (16, 36, 108, 192)] == [16, 36, 108, 192]


def test_operands_are_cached_per_parameter_version():
    m = EC.gmm("a", "cpu")
    ops = m.operands(True)
    assert m.operands(True) is ops
    m.set_cov_reg(0.1)                      # the regularisation is a runtime scalar: no rebuild
    assert m.operands(True) is ops
    m.set_cov(2 * m.get_cov())
    assert m.operands(True) is not ops
    ops = m.operands(True)
    m.set_weights(torch.arange(1.0, m.n_components + 1))
    assert m.operands(True) is not ops
    ops = m.operands(True)
    m.mu.data = m.mu.data + 1               # rebinding .data, as the reference's fit does
    assert m.operands(True) is not ops
    # the documented limit: an in-place write through .data bumps no version counter and has to be announced
    ops = m.operands(True)
    m.mu.data[0] = 5.0
    assert m.operands(True) is ops
    m.invalidate()
    fresh = m.operands(True)
    assert fresh is not ops and not torch.equal(fresh.m, ops.m)


@pytest.mark.parametrize("H,W,p", [(3, 3, 3), (3, 9, 3), (7, 5, 4), (19, 22, 4), (14, 17, 3), (6, 37, 6), (8, 8, 1)])
def test_multiplicity_against_brute_force(H, W, p):
    count = torch.zeros(H, W, dtype=torch.int64)
    for y0 in range(H - p + 1):
        for x0 in range(W - p + 1):
            count[y0:y0 + p, x0:x0 + p] += 1
    assert torch.equal(G.multiplicity(H, W, p), count)


def test_python_refusals():
    with pytest.raises(ValueError, match="negative"):
        dinv.optim.GaussianMixtureModel(2, 3).set_weights(torch.tensor([1.0, -1.0]))
    with pytest.raises(NotImplementedError, match="fit"):
        dinv.optim.GaussianMixtureModel(2, 3).fit(None)
    for name in ("download", "GMM_BSDS_gray", "GMM_lodopab_small"):
        with pytest.raises(ValueError, match="no network fetch"):
            dinv.optim.EPLL(pretrained=name, n_components=2, patch_size=2)
    with pytest.raises(ValueError, match=".pt"):
        dinv.models.EPLLDenoiser(pretrained="weights.bin", n_components=2, patch_size=2)
    # a covariance that is not positive definite: the unregularised operands are refused, the regularised ones are built
    m = dinv.optim.GaussianMixtureModel(2, 3)
    m.set_cov(torch.diag(torch.tensor([1.0, 0.5, 0.0]))[None].repeat(2, 1, 1))
    assert m.operands(True).lam_min <= 0
    with pytest.raises(ValueError, match="positive definite"):
        m.operands(False)
    with pytest.raises(ValueError, match="positive definite"):
        G.pack(m._cov, m.mu, m._weights, "cpu", regularized=False)
    with pytest.raises(ValueError, match="lam \\+ r must be positive"):
        G._reg(m.operands(True), 0.0, 1, torch.device("cpu"))
    with pytest.raises(ValueError, match="set_cov_reg"):
        m._r(True)
    with pytest.raises(ValueError, match="expected cov"):
        G.eigen_pack(torch.eye(3)[None], torch.zeros(1, 2), torch.ones(1))
    with pytest.raises(ValueError, match="dimension"):
        G.patch_grid((1, 1, 8, 8), 3, 16)
    with pytest.raises(ValueError, match="holds no"):
        G.patch_grid((1, 1, 3, 8), 4, 16)
    with pytest.raises(ValueError, match="sigma has 3 values"):
        from deepinv_amd.optim.epll import _per_image
        _per_image([0.1, 0.2, 0.3], 2, "sigma")


def test_state_dict_from_a_pt_file(tmp_path):
    sd = {"GMM." + k: v for k, v in EC.state_dict("a").items()}
    path = str(tmp_path / "gmm.pt")
    torch.save(sd, path)
    model = dinv.optim.EPLL(n_components=8, pretrained=path, patch_size=4, channels=1)
    assert torch.equal(model.GMM._cov, sd["GMM._cov"])


def test_cpu_tensors_raise():
    """no CPU fallback: a CPU tensor must raise, never silently compute"""
    m = EC.gmm("a", "cpu")
    x = EC.t("rows_x", "cpu")
    for call in (lambda: m(x), lambda: m.classify(x), lambda: m.component_log_likelihoods(x),
                 lambda: EC.denoiser("a", "cpu")(EC.t("den_a_y", "cpu"), 0.1)):
        with pytest.raises(HipExtensionError):
            call()
