"""The Poisson-family noise kernel (deepinv_amd/csrc/random.hip: dinv_poisson_noise) and the pointwise likelihood kernel
(deepinv_amd/csrc/elementwise.hip: dinv_fidelity_pointwise) on the host emulation.

A random kernel is tested on the DISTRIBUTION it must have: Pearson's chi-square of 200 000 draws against the Poisson pmf in fp64
(bins merged left to right until each expects at least 10 counts; bound df + 5 sqrt(2 df), the bound of the mask-generator tests,
false-alarm rate ~ 1e-6).  The same design passes for torch.poisson on the CPU at every rate used here."""
import ctypes
import math

import numpy as np
import pytest
import torch

import emu_lib as E

POISSON, POISSON_GAUSSIAN, POISSON_LOG = 0, 1, 2
NORMALIZE, CLIP_POSITIVE = 1, 2
PTRS_FROM = 10.0            # the kernel's switch-over rate (multiplication below, PTRS from there on)
N = 200_000


def poisson_noise(x, mode=POISSON, flags=0, gain=1.0, sigma=0.0, per=None, min_gain=1e-12, seed=1234, off=0, want_bad=True):
    """y, bad = dinv_poisson_noise(x); gain / sigma: float or a [B] table (then `per` = elements per sample)"""
    x = x.contiguous().float()
    n = x.numel()
    y = torch.full((n,), float("nan"))
    bad = torch.zeros(2, dtype=torch.int32)
    gt = gain if isinstance(gain, torch.Tensor) else None
    st = sigma if isinstance(sigma, torch.Tensor) else None
    E.check(E.lib().dinv_poisson_noise(ctypes.c_int64(n), ctypes.c_int64(per or max(n, 1)), E.p(x), E.p(gt),
                                       ctypes.c_float(0.0 if gt is not None else gain), E.p(st),
                                       ctypes.c_float(0.0 if st is not None else sigma), ctypes.c_int32(mode), ctypes.c_int32(flags),
                                       ctypes.c_float(min_gain), ctypes.c_uint64(seed), ctypes.c_uint64(off),
                                       E.p(bad) if want_bad else None, E.p(y), None))
    return y, bad


def log_pmf(k, lam):
    return -lam + k * math.log(lam) - math.lgamma(k + 1.0)


def chi_square_vs_pmf(samples, lam):
    """Pearson statistic of integer samples against Poisson(lam): cells k = lo..hi around the mean plus the two tails, merged left to
    right until every cell expects at least 10 counts"""
    k = np.asarray(samples, dtype=np.int64)
    n = k.size
    width = int(12 * math.sqrt(lam) + 30)
    lo, hi = max(0, int(lam) - width), int(lam) + width
    p = np.array([math.exp(log_pmf(j, lam)) for j in range(lo, hi + 1)])
    below = max(0.0, 1.0 - p.sum()) if lo > 0 else 0.0       # both tails are below 1e-30 of the mass at this width; kept for form
    counts = np.bincount(np.clip(k, lo, hi) - lo, minlength=hi - lo + 1).astype(float)
    expect = p * n
    expect[0] += below * n / 2
    expect[-1] += max(0.0, 1.0 - p.sum() - below / 2) * n
    cells_o, cells_e, o, e = [], [], 0.0, 0.0
    for c, ex in zip(counts, expect):
        o, e = o + c, e + ex
        if e >= 10:
            cells_o.append(o)
            cells_e.append(e)
            o = e = 0.0
    if e > 0 and cells_e:          # the remainder on the right joins the last cell
        cells_o[-1] += o
        cells_e[-1] += e
    cells_o, cells_e = np.array(cells_o), np.array(cells_e)
    df = len(cells_e) - 1
    stat = float(((cells_o - cells_e) ** 2 / cells_e).sum())
    return stat, df, df + 5.0 * math.sqrt(2.0 * max(df, 1))


RATES = [0.01, 0.5, 3.0, 9.99, 10.0, 10.01, 30.0, 1e3, 1e5,
         float(np.nextafter(np.float32(PTRS_FROM), np.float32(0))), float(np.nextafter(np.float32(PTRS_FROM), np.float32(20)))]


@pytest.mark.parametrize("lam", RATES)
def test_distribution_matches_the_exact_pmf(lam):
    lam32 = float(np.float32(lam))                       # the rate the kernel sees
    y, bad = poisson_noise(torch.full((N,), lam32), seed=2024 + int(lam * 7) % 1000)
    assert bad.tolist() == [0, 0]
    k = y.numpy()
    assert np.all(k >= 0) and np.all(k == np.round(k))                       # non-negative integers
    stat, df, bound = chi_square_vs_pmf(k, lam32)
    print(f"lambda = {lam32!r}: chi-square {stat:.1f}, df {df}, bound {bound:.1f}")
    assert df >= 1 and stat < bound, (lam32, stat, df, bound)


def test_moments_at_a_very_large_rate():
    lam = 1e6
    y, _ = poisson_noise(torch.full((N,), lam), seed=5)
    k = y.double().numpy()
    assert np.all(k == np.round(k))
    mean, var = k.mean(), k.var()
    print(f"lambda = 1e6: mean - lambda = {mean - lam:.2f} (bound {5 * math.sqrt(lam / N):.2f}), var / lambda = {var / lam:.4f}")
    assert abs(mean - lam) < 5 * math.sqrt(lam / N)
    assert abs(var / lam - 1) < 0.02


def test_zero_rate_reproducibility_and_geometry_independence():
    n = 50_001
    assert float(poisson_noise(torch.zeros(1000))[0].abs().max()) == 0                      # lambda = 0 -> exactly 0
    x = torch.linspace(0, 40, n)                          # both samplers in one call
    y, _ = poisson_noise(x, seed=99, off=16)
    assert torch.all(y >= 0) and torch.equal(y, y.round())
    assert torch.equal(y, poisson_noise(x, seed=99, off=16)[0])                             # same (seed, offset) -> same bits
    y_next = poisson_noise(x, seed=99, off=16 + n)[0]                                       # the next offset block is fresh
    assert float((y_next != y).float().mean()) > 0.5
    assert float((poisson_noise(x, seed=100, off=16)[0] != y).float().mean()) > 0.5
    # element i depends on (seed, offset + i) alone: a prefix (another launch grid) and a shifted window give the same numbers
    assert torch.equal(poisson_noise(x[:777], seed=99, off=16)[0], y[:777])
    assert torch.equal(poisson_noise(x[1000:3000], seed=99, off=16 + 1000)[0], y[1000:3000])
    # ... and a per-sample launch (a two-dimensional grid) with equal gains as well
    yb, _ = poisson_noise(x[:50_000], gain=torch.ones(50), per=1000, seed=99, off=16)
    assert torch.equal(yb, y[:50_000])


def test_per_sample_gain_and_normalize():
    B, per = 4, 50_000
    gain = torch.tensor([0.05, 0.5, 1.0, 4.0])
    x = torch.full((B * per,), 6.0)
    for flags in (0, NORMALIZE):
        y, bad = poisson_noise(x, flags=flags, gain=gain, per=per, seed=31)
        assert bad.tolist() == [0, 0]
        y = y.reshape(B, per).double()
        for b in range(B):
            g = float(gain[b])
            k = (y[b] / g if flags else y[b]).numpy()
            assert np.allclose(k, np.round(k), atol=1e-3)
            lam = float(np.float32(6.0) / np.float32(g))
            stat, df, bound = chi_square_vs_pmf(np.round(k), lam)
            assert stat < bound, (flags, b, stat, df, bound)


def test_poisson_gaussian_residual_is_gaussian():
    n = 200_003
    gain, sigma, lam = 0.5, 0.25, 20.0
    x = torch.full((n,), lam * gain)
    y, bad = poisson_noise(x, mode=POISSON_GAUSSIAN, gain=gain, sigma=sigma, seed=77)
    k, _ = poisson_noise(x, mode=POISSON, gain=gain, seed=77)          # the same Poisson stream: the count is the same draw
    assert bad.tolist() == [0, 0]
    z = (y - gain * k) / sigma
    assert abs(float(z.mean())) < 0.01 and abs(float(z.std()) - 1) < 0.01          # the tolerances of the Gaussian kernel's test
    assert abs(float((z ** 3).mean())) < 0.03 and abs(float((z ** 4).mean()) - 3) < 0.06
    assert abs(float((z.abs() < 1).float().mean()) - 0.6827) < 0.005
    stat, df, bound = chi_square_vs_pmf(k.numpy(), lam)
    assert stat < bound
    assert abs(float(np.corrcoef(z.numpy(), k.numpy())[0, 1])) < 0.01              # its own stream: independent of the count
    # min_gain: gain 0 is raised to min_gain, the rate x / min_gain and the output min_gain k (noise.py:631-646)
    y0, bad = poisson_noise(torch.full((1000,), 3.0), mode=POISSON_GAUSSIAN, gain=0.0, sigma=0.0, min_gain=0.25, seed=3)
    assert bad.tolist() == [0, 0] and torch.equal(y0 * 4, (y0 * 4).round()) and abs(float(y0.mean()) - 3.0) < 0.2
    # per-sample sigma
    ys, _ = poisson_noise(torch.zeros(4000), mode=POISSON_GAUSSIAN, gain=1.0, sigma=torch.tensor([0.0, 1.0, 2.0, 3.0]), per=1000)
    ys = ys.reshape(4, 1000)
    assert float(ys[0].abs().max()) == 0 and abs(float(ys[2].std()) - 2) < 0.15 and abs(float(ys[3].std()) - 3) < 0.2


def test_log_poisson_output_is_the_transform_of_an_integer_count():
    N0, mu = 1024.0, 1 / 50.0
    x = torch.linspace(0, 400, 100_000)
    y, bad = poisson_noise(x, mode=POISSON_LOG, gain=N0, sigma=mu, seed=8)
    assert bad.tolist() == [0, 0]
    finite = torch.isfinite(y)
    assert torch.all(y[~finite] == float("inf"))                       # k = 0 -> +inf, as in the reference
    k = N0 * torch.exp(-mu * y[finite].double())
    kr = k.round()
    assert float((k - kr).abs().max()) < 1e-3 * float(kr.max()) and float(kr.min()) >= 1
    back = -torch.log(kr.float() / np.float32(N0)) / np.float32(mu)
    assert float(((back - y[finite]).abs() / (1 + back.abs())).max()) < 1e-6
    # the counts have the Poisson law of N0 exp(-mu x): at one x, chi-square
    x1 = torch.full((N,), 100.0)
    y1, _ = poisson_noise(x1, mode=POISSON_LOG, gain=N0, sigma=mu, seed=9)
    lam = float(np.float32(N0) * np.exp(np.float32(-100.0) * np.float32(mu), dtype=np.float32))
    k1 = np.round(N0 * np.exp(-mu * y1.double().numpy()))
    stat, df, bound = chi_square_vs_pmf(k1, lam)
    assert stat < bound, (stat, df, bound)
    # a far-away x: rate ~ 0, every count 0, every output +inf
    assert torch.all(poisson_noise(torch.full((100,), 1e4), mode=POISSON_LOG, gain=N0, sigma=mu)[0] == float("inf"))


def test_negative_and_non_finite_inputs_are_defined_and_the_call_returns():
    x = torch.tensor([1.0, -2.0, 0.0, float("nan"), float("inf"), 5.0, 3e38, 1e-30, -0.0] * 30)
    y, bad = poisson_noise(x, seed=1)
    assert bad.tolist() == [1, 0]                                       # negative input: the flag, and NaN where it was
    assert torch.all(torch.isnan(y[x < 0])) and torch.all(torch.isnan(y[torch.isnan(x)]))
    assert torch.all(y[x == float("inf")] == float("inf"))
    assert torch.all(y[x == 0] == 0) and torch.all(y[x == 1e-30] == 0)
    ok = (x > 0) & torch.isfinite(x)
    assert torch.all(torch.isfinite(y[ok])) and torch.all(y[ok] >= 0)
    yc, bad = poisson_noise(x, flags=CLIP_POSITIVE, seed=1)
    assert bad.tolist() == [0, 0]                                       # clip_positive: no flag ...
    assert torch.all(yc[x < 0] == 0) and not torch.any(torch.isnan(yc[~torch.isnan(x)]))      # ... and no NaN from a negative input
    assert torch.all(torch.isnan(yc[torch.isnan(x)]))
    poisson_noise(x, flags=CLIP_POSITIVE, want_bad=False)               # no flag buffer is needed then
    assert poisson_noise(torch.ones(10), gain=-1.0)[1].tolist()[1] == 1          # a non-positive gain is flagged too
    assert poisson_noise(torch.ones(10), gain=torch.tensor([1.0, 0.0]), per=5)[1].tolist() == [0, 1]
    for mode in (POISSON_GAUSSIAN, POISSON_LOG):
        ym, _ = poisson_noise(x, mode=mode, gain=1.0 if mode == POISSON_GAUSSIAN else 1024.0, sigma=0.02, flags=CLIP_POSITIVE)
        assert torch.all(torch.isnan(ym[torch.isnan(x)]))


def test_bad_arguments_are_refused():
    l = E.lib()
    x = torch.ones(8)
    args = lambda n, per, mode, flags: (ctypes.c_int64(n), ctypes.c_int64(per), E.p(x), None, ctypes.c_float(1), None, ctypes.c_float(0),
                                        ctypes.c_int32(mode), ctypes.c_int32(flags), ctypes.c_float(0), ctypes.c_uint64(0),
                                        ctypes.c_uint64(0), None, E.p(x), None)
    assert l.dinv_poisson_noise(*args(8, 3, 0, 0)) != 0         # per_sample does not divide n
    assert l.dinv_poisson_noise(*args(8, 8, 3, 0)) != 0         # unknown mode
    assert l.dinv_poisson_noise(*args(8, 8, 0, 4)) != 0         # unknown flag
    assert l.dinv_poisson_noise(*args(0, 8, 0, 0)) == 0


# ---- dinv_fidelity_pointwise against an fp64 restatement of the reference's formulas (distance.py:222-263, 279-323, 392-395).
# Bound: twice the error of the reference's own fp32 tensor expression on the same inputs (the convention of the single-pixel tests).
FID = {"poisson_grad": 0, "poisson_prox": 1, "l1_grad": 2, "l1_prox": 3, "logpoisson_grad": 4}


def fidelity(op, x, y, p0=1.0, p1=0.0, gamma=1.0, denorm=False):
    out = torch.full_like(x, float("nan"))
    E.check(E.lib().dinv_fidelity_pointwise(ctypes.c_int32(FID[op]), ctypes.c_int64(x.numel()), E.p(x), E.p(y), ctypes.c_float(p0),
                                            ctypes.c_float(p1), ctypes.c_float(gamma), ctypes.c_int32(1 if denorm else 0), E.p(out),
                                            None))
    return out


def reference_expression(op, x, y, p0, p1, gamma, denorm):
    """the reference's tensor expressions, in the dtype of x"""
    if op.startswith("poisson"):
        gain, bkg = p0, p1
        if denorm:
            y = y / gain
        if op == "poisson_grad":
            return gain * (1 - y / (x / gain + bkg))
        return (x - (1 / (gain * gamma)) * ((x - (1 / (gain * gamma))).pow(2) + 4 * y / gamma).sqrt()) / 2
    if op == "l1_grad":
        return torch.sign(x - y)
    if op == "l1_prox":
        return torch.nn.functional.softshrink(x - y, lambd=gamma) + y
    N0, mu = p0, p1
    return N0 * mu * (torch.exp(-mu * y) - torch.exp(-mu * x))


@pytest.mark.parametrize("op,p0,p1,gamma,denorm", [
    ("poisson_grad", 1.0, 0.0, 1.0, False), ("poisson_grad", 0.1, 0.05, 1.0, True), ("poisson_grad", 3.0, 1.0, 1.0, False),
    ("poisson_prox", 1.0, 0.0, 1.0, False), ("poisson_prox", 0.1, 0.0, 0.7, True), ("poisson_prox", 2.0, 0.0, 3.0, False),
    ("l1_grad", 1.0, 0.0, 1.0, False), ("l1_prox", 1.0, 0.0, 0.3, False), ("l1_prox", 1.0, 0.0, 2.0, False),
    ("logpoisson_grad", 1024.0, 1 / 50.0, 1.0, False), ("logpoisson_grad", 100.0, 0.5, 1.0, False)])
def test_fidelity_pointwise_against_fp64(op, p0, p1, gamma, denorm):
    g = torch.Generator().manual_seed(11)
    n = 10_007                                     # not a multiple of the block or of four
    x = torch.rand(n, generator=g) * 5 + 0.01
    y = torch.rand(n, generator=g) * 5 + 0.01
    if op.startswith("l1"):
        y[::7] = x[::7]                            # ties: sign 0, inside the threshold
    ref64 = reference_expression(op, x.double(), y.double(), p0, p1, gamma, denorm)
    ref32 = reference_expression(op, x, y, p0, p1, gamma, denorm)
    out = fidelity(op, x, y, p0, p1, gamma, denorm)
    e_ref = float((ref32.double() - ref64).norm() / ref64.norm())
    e_out = float((out.double() - ref64).norm() / ref64.norm())
    print(f"{op}: kernel {e_out:.3e}, reference fp32 {e_ref:.3e}")
    if op == "l1_grad":
        assert torch.equal(out, ref32)             # exact values
    else:
        assert e_out <= 2 * e_ref, (op, e_out, e_ref)
    assert not torch.any(torch.isnan(out))


def test_fidelity_pointwise_in_place_and_bad_arguments():
    x, y = torch.rand(100) + 0.1, torch.rand(100)
    want = fidelity("l1_prox", x, y, gamma=0.2)
    xs = x.clone()
    E.check(E.lib().dinv_fidelity_pointwise(ctypes.c_int32(3), ctypes.c_int64(100), E.p(xs), E.p(y), ctypes.c_float(1), ctypes.c_float(0),
                                            ctypes.c_float(0.2), ctypes.c_int32(0), E.p(xs), None))
    assert torch.equal(xs, want)
    assert E.lib().dinv_fidelity_pointwise(ctypes.c_int32(5), ctypes.c_int64(100), E.p(x), E.p(y), ctypes.c_float(1), ctypes.c_float(0),
                                           ctypes.c_float(1), ctypes.c_int32(0), E.p(xs), None) != 0
    nan = torch.tensor([float("nan")])
    assert torch.isnan(fidelity("l1_prox", nan, torch.zeros(1))).all() and torch.isnan(fidelity("l1_grad", nan, torch.zeros(1))).all()
