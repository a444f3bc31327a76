#!/usr/bin/env python
"""Golden vectors for GaussianMixtureModel.fit from the REAL reference (deepinv v0.4.1, oracle/ref_shim.py), float32 and float64 on
the CPU (deepinv/optim/utils.py:314-412).  The data file holds only inputs, results and recorded spreads and margins.

Every data set is drawn from a random mixture built as tests/golden/make_golden_epll.py builds its models, at the scale of image
patches: QR of randn, eigenvalues 0.01 logspace(-1, 0, d) times a factor in [0.5, 1.5) per component, means 0.5 + sep randn, the
component of each row drawn at random, rows rounded to fp32.  Four kinds of record:
  a          separated (sep = 0.3): K = 3, d = 16, 600 rows in batches of 256, 5 iterations, data_init
  b3, b4     overlapping: K = 3, d = 16, 600 rows, sep = 0.01, 8 iterations; K = 4, d = 9, 333 rows in batches of 128, sep = 0.05,
             8 iterations.  The script asserts that more than half of the rows end with a responsibility strictly between 1e-3 and
             1 - 1e-3, so that the E-step counts.
  c          one step from a prescribed state (stored): data_init=False, max_iters=1, K = 5, d = 36, 1500 rows in batches of 512
  d          the data of b3 with stopping_criterion=1e-2 and max_iters=40; the number of iterations run is stored, and the script
             asserts that every objective decrement lies at least 100 times the fp32-against-fp64 objective difference away from
             the threshold, so the stop count does not sit on a rounding flip.
Per record and iteration: what _EM_step returned (weights, means, covariances plus the regularisation that fit adds, objective) in
fp32 and fp64, and per quantity the reference's own fp32-against-fp64 spread (largest absolute difference over all iterations).

    python tests/golden/make_golden_gmm_fit.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_shim import import_reference  # noqa: E402

import_reference()
from deepinv.optim.utils import GaussianMixtureModel  # noqa: E402

g = torch.Generator()
out = {}
REG = 1e-5


def random_mixture(K, d, sep):
    """(weights, means, covariances) in fp64"""
    Q = torch.linalg.qr(torch.randn(K, d, d, generator=g, dtype=torch.float64))[0]
    lam = 0.01 * torch.logspace(-1, 0, d, dtype=torch.float64)[None] * (0.5 + torch.rand(K, 1, generator=g, dtype=torch.float64))
    cov = Q @ torch.diag_embed(lam) @ Q.transpose(1, 2)
    mu = 0.5 + sep * torch.randn(K, d, generator=g, dtype=torch.float64)
    w = torch.rand(K, generator=g, dtype=torch.float64) + 0.1
    return w / w.sum(), mu, cov


def draw(mix, n, distinct_first=False):
    """n rows of the mixture; distinct_first: the first K rows, which data_init takes as means, come from K different components"""
    w, mu, cov = mix
    k = torch.randint(0, w.numel(), (n,), generator=g)
    if distinct_first:
        k[: w.numel()] = torch.randperm(w.numel(), generator=g)
    L = torch.linalg.cholesky(cov)
    return (mu[k] + torch.einsum("nij,nj->ni", L[k], torch.randn(n, mu.shape[1], generator=g, dtype=torch.float64))).float()


def run(x, batch, K, dtype, init=None, **fit):
    """the reference's fit on the rows x in batches: (the model, one (weights, mu, cov + reg, objective) per iteration)"""
    m = GaussianMixtureModel(K, x.shape[1])
    if dtype == torch.float64:
        m = m.double()
    if init is not None:
        w, mu, cov = init
        m.set_weights(w.to(dtype))
        m.mu.data = mu.to(dtype)
        m.set_cov(cov.to(dtype))
    log, step = [], m._EM_step

    def traced(dataloader, verbose=False):
        w, mu, cov, obj = step(dataloader, verbose)
        eye = (REG * torch.eye(x.shape[1])[None]).to(cov)
        log.append((w.clone(), mu.clone(), cov + eye, torch.as_tensor(obj).clone()))
        return w, mu, cov, obj

    m._EM_step = traced
    with torch.no_grad():
        m.fit([b.to(dtype) for b in x.split(batch)], cov_regularization=REG, **fit)
    return m, log


def record(tag, x, batch, K, init=None, **fit):
    out[f"{tag}_x"], out[f"{tag}_batch"], out[f"{tag}_K"] = x.numpy(), np.int64(batch), np.int64(K)
    if init is not None:
        for name, t in zip(("weights", "mu", "cov"), init):
            out[f"{tag}_init_{name}"] = t.float().numpy()
        init = tuple(t.float() for t in init)
    m32, log32 = run(x, batch, K, torch.float32, init, **fit)
    m64, log64 = run(x, batch, K, torch.float64, init, **fit)
    assert len(log32) == len(log64), (tag, len(log32), len(log64))
    out[f"{tag}_iters"] = np.int64(len(log64))
    for i, name in enumerate(("weights", "mu", "cov", "objective")):
        a32, a64 = torch.stack([it[i] for it in log32]), torch.stack([it[i] for it in log64])
        out[f"{tag}_{name}_f32"], out[f"{tag}_{name}_f64"] = a32.numpy(), a64.numpy()
        out[f"{tag}_{name}_spread"] = np.float64((a32.double() - a64).abs().max())
    assert torch.allclose(m64.get_cov(), log64[-1][2]) and torch.equal(m64.mu, log64[-1][1])
    # the share of rows that end soft under the fp64 model
    s = m64.component_log_likelihoods(x.double()) + torch.log(m64._weights[None])
    beta = torch.softmax(s, 1)
    soft = float(((beta > 1e-3) & (beta < 1 - 1e-3)).any(1).double().mean())
    out[f"{tag}_soft"] = np.float64(soft)
    print(tag, "iterations", len(log64), "spread of weights / means / covariances / objective",
          *(f"{float(out[f'{tag}_{n}_spread']):.3g}" for n in ("weights", "mu", "cov", "objective")),
          f"largest |cov| {float(log64[-1][2].abs().max()):.3g} soft rows {soft:.2f}")
    return log32, log64


g.manual_seed(2012)
record("a", draw(random_mixture(3, 16, 0.3), 600, distinct_first=True), 256, 3, max_iters=5, data_init=True)
g.manual_seed(2013)
record("b4", draw(random_mixture(4, 9, 0.05), 333), 128, 4, max_iters=8, data_init=True)
assert out["b4_soft"] > 0.5, out["b4_soft"]
g.manual_seed(2014)
record("c", draw(random_mixture(5, 36, 0.1), 1500), 512, 5, init=random_mixture(5, 36, 0.1), max_iters=1, data_init=False)

# b3 and d share their data: the first of a sequence of seeds whose stopping run is clear of the threshold and lasts at least as
# many iterations as b3 runs, so that the stopping test sees several decrements above the threshold before the one below it (a
# choice made from the reference's two runs alone).  Seeds 0 to 65 were tried and are skipped here to save the minutes they take:
# none qualifies (seed 15 is clear but stops after 3 iterations).
THRESHOLD = 1e-2
FIRST_SEED = 66
for seed in range(FIRST_SEED, 400):
    g.manual_seed(seed)
    xb3 = draw(random_mixture(3, 16, 0.01), 600)
    try:
        log32, log64 = record("d", xb3, 256, 3, max_iters=40, data_init=True, stopping_criterion=THRESHOLD)
    except AssertionError:          # the two precisions stop at different iterations: on a rounding flip
        continue
    o32, o64 = (np.array([float(it[3]) for it in log]) for log in (log32, log64))
    dec = -np.diff(o64)                                   # (the first decrement, from 1e100, is not among them)
    diff = float(np.abs(o32 - o64).max())
    margin = float(np.abs(dec - THRESHOLD).min())
    print("d: seed", seed, "decrements", dec, "fp32 - fp64 objective difference", diff, "smallest distance to the threshold", margin)
    if margin >= 100 * diff and 8 <= len(log64) < 40:
        break
else:
    raise SystemExit("d: no clear seed")
out["d_seed"], out["d_threshold"], out["d_objective_diff"], out["d_margin"] = np.int64(seed), np.float64(THRESHOLD), np.float64(diff), np.float64(margin)
assert margin >= 100 * diff, (margin, diff)
assert dec[-1] < THRESHOLD and (dec[:-1] >= THRESHOLD).all()
record("b3", xb3, 256, 3, max_iters=8, data_init=True)
assert out["b3_soft"] > 0.5, out["b3_soft"]

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gmm_fit.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
