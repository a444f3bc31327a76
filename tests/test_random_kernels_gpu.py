"""Every path of csrc/random.hip on the MI355X, per element against the replay of the Philox stream in tests/random_cases.py: the
whole case table through the C entry points of the product library on guarded buffers - including what the host emulation does not
run or cannot tell: the second pass of the Gaussian grid-stride loop with a ragged end above 8192 workgroups, the Poisson grid at
its caps (16384 workgroups flat, 16384 / batch per sample, one strided workgroup above 16384 samples, the loop over samples above
65535), and the device's own expf, logf, sinf, cosf and contracted fp64.  Then the public classes - the four noise models and the
four mask generators - with an explicit torch.Generator: the output is the replay at (initial_seed, offset before the call), the
offset advances by what hip.random.philox_state documents, two successive calls consume disjoint counter ranges, and a raised
ValueError leaves the offset where it was.  The last test of the table prints the worst ratio of error to bound."""
import numpy as np
import pytest
import torch

import random_cases as RC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
WORST = {}
SEED = 0x1234567811223344                      # the high word set
OFFSETS = [0, 2 ** 32 - 4, 2 ** 33 + 16]       # torch keeps Philox offsets in multiples of 4; the second crosses 2^32 inside a call


@pytest.fixture(scope="module")
def runner():
    from deepinv_amd import hip
    from deepinv_amd.hip import random as hrand

    return RC.Runner(hrand._l(), DEV, lambda: hip.stream_ptr(DEV))


@pytest.mark.parametrize("case", RC.TABLE, ids=lambda c: c.id)
def test_random_path(runner, case):
    WORST[case.id] = RC.run_case(runner, case)


def test_random_rejections_write_nothing(runner):
    RC.run_rejections(runner)


def test_random_worst_ratio():
    if not WORST:                 # the cases were deselected: nothing to report
        return
    for table in ("gaussian", "poisson", "mask"):
        part = {k: v for k, v in WORST.items() if k.startswith(table)}
        if part:
            cid, ratio = max(part.items(), key=lambda kv: kv[1])
            print(f"{table}: {len(part)} cases, worst error / bound {ratio:.3g} ({cid})")
    assert max(WORST.values()) <= 1.0


# ------------------------------------------------------------------ the public classes
def _rng(offset):
    g = torch.Generator(DEV).manual_seed(SEED)
    g.set_offset(offset)
    assert g.initial_seed() == SEED and g.get_offset() == offset
    return g


def _two_calls(rng, call, advance, consumed):
    """[(offset before the call, output)] of two successive calls; the generator advances as documented and past what was consumed"""
    seen = []
    for _ in range(2):
        before = rng.get_offset()
        out = call()
        assert rng.get_offset() - before == advance, f"the offset advanced by {rng.get_offset() - before}, documented: {advance}"
        seen.append((before, out.cpu().numpy()))
    assert consumed <= advance and rng.initial_seed() == SEED
    return seen


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("per_sample", [False, True], ids=["scalar", "per-sample"])
def test_gaussian_noise_is_the_replay(offset, per_sample):
    import deepinv_amd as dinv

    rng = _rng(offset)
    x = torch.randn(3, 2, 17, 19, generator=torch.Generator().manual_seed(1))
    sigma = torch.tensor([0.5, 0.0, 1.5]) if per_sample else 0.2
    nm = dinv.physics.GaussianNoise(sigma, rng=rng)
    xd = x.to(DEV)
    n = x.numel()
    sig = (np.repeat(np.asarray(sigma, dtype=np.float32), n // 3) if per_sample else np.full(n, np.float32(0.2))).astype(np.float64)
    for before, y in _two_calls(rng, lambda: nm(xd), RC.gaussian_advance(n), RC.cdiv(n, 4)):
        ref, M = RC.gaussian_reference(n, x.reshape(-1).double().numpy(), sig, SEED, before)
        RC._ratio(f"GaussianNoise at offset {before}", y.reshape(-1), ref, M, RC.BOUNDS["gaussian"])


def _rates(n, gain):
    rng = np.random.default_rng(5)
    lam = np.where(rng.random(n) < 0.5, rng.random(n) * 10.0, 10.0 ** (1.0 + 4.0 * rng.random(n))).astype(np.float32)
    lam[:6] = [0.0, 1e-30, 9.99, 10.0, 12.0, 1e5]
    return (lam * np.float32(gain)).astype(np.float32)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("model", ["PoissonNoise", "PoissonNoise-counts", "PoissonGaussianNoise", "LogPoissonNoise"])
def test_poisson_family_is_the_replay(offset, model):
    import deepinv_amd as dinv

    rng = _rng(offset)
    shape = (3, 2, 15, 21)
    n = int(np.prod(shape))
    if model == "LogPoissonNoise":
        nm, mode, flags, g, s, min_gain = dinv.physics.LogPoissonNoise(N0=1024.0, mu=0.02, rng=rng), RC.POISSON_LOG, 0, 1024.0, 0.02, 0.0
        x = np.linspace(0.0, 400.0, n).astype(np.float32)
    elif model == "PoissonGaussianNoise":
        nm = dinv.physics.PoissonGaussianNoise(gain=0.5, sigma=0.1, rng=rng)
        mode, flags, g, s, min_gain, x = RC.POISSON_GAUSSIAN, 0, 0.5, 0.1, 1e-12, _rates(n, 0.5)
    else:
        normalize = model == "PoissonNoise"
        nm = dinv.physics.PoissonNoise(gain=0.25, normalize=normalize, rng=rng)
        mode, flags, g, s, min_gain, x = RC.POISSON, RC.NORMALIZE if normalize else 0, 0.25, 0.0, 0.0, _rates(n, 0.25)
    xd = torch.from_numpy(x).reshape(shape).to(DEV)
    for before, y in _two_calls(rng, lambda: nm(xd), RC.poisson_advance(n), n):
        ref = RC.poisson_reference(x, np.full(n, g, np.float32), np.full(n, s, np.float32), mode, flags, min_gain, SEED, before)
        assert ref["bad"] == [0, 0]
        RC.poisson_compare(f"{model} at offset {before}", y.reshape(-1), ref)


@pytest.mark.parametrize("model", ["PoissonNoise", "PoissonGaussianNoise"])
def test_a_raised_error_leaves_the_offset(model):
    import deepinv_amd as dinv

    rng = _rng(OFFSETS[1])
    x = torch.ones(2, 1, 8, 8, device=DEV)
    x[1, 0, 3, 3] = -1.0
    # a negative input; a non-positive gain (the Poisson-Gaussian model raises it to min_gain instead)
    for gain in (1.0, -1.0) if model == "PoissonNoise" else (1.0,):
        nm = getattr(dinv.physics, model)(gain=gain, rng=rng)
        with pytest.raises(ValueError):
            nm(x if gain > 0 else x.abs())
        assert rng.get_offset() == OFFSETS[1] and rng.initial_seed() == SEED


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("cls", ["RandomMaskGenerator", "GaussianMaskGenerator", "EquispacedMaskGenerator", "PolyOrderMaskGenerator"])
def test_mask_generators_are_the_replay(offset, cls):
    import deepinv_amd as dinv

    rng = _rng(offset)
    B, C, T, H, W = 3, 2, 5, 4, 96
    gen = getattr(dinv.physics.generator, cls)((C, T, H, W), acceleration=4, device=DEV, rng=rng)
    pdf, accel, n_off = gen._sampling(W)
    pdf = None if pdf is None else pdf.cpu().numpy()
    lo, hi = gen._center(W)
    for before, m in _two_calls(rng, lambda: gen.step(batch_size=B)["mask"], RC.mask_advance(B, T), B * T * RC.MASK_ROW_COUNTERS):
        assert m.shape == (B, C, T, H, W)
        must, may, count = RC.mask_reference(B, T, W, gen.n_lines, lo, hi, gen.mode, pdf, accel, n_off, SEED, before)
        RC.mask_check(f"{cls} at offset {before}", m, B, C, T, H, W, must, may, count)
