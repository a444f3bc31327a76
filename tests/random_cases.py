"""Shared by tests/test_random_kernels_gpu.py (the gfx950 library) and tests/test_emu_random_cases.py (the same kernel sources on
the host emulation): the case table of csrc/random.hip - gaussian_noise_kernel, poisson_noise_kernel, mask_lines_kernel - per
element against a REPLAY of the random stream.  The kernels are counter based: every output is a function of (seed, offset,
index, inputs), and this file restates that function in numpy alone, in uint64 and fp64: Philox4x32-10 with the counter
(ctr_lo, ctr_hi, stream, round) and the key (seed_lo, seed_hi), the uniforms, the counter maps of the three calls, Box-Muller,
the Poisson draw from the literature (Knuth's multiplication below a rate of 10, Hoermann's PTRS with the paper's constants and
the true log pmf = -lambda + k log lambda - lgamma(k + 1) from there on) and the three mask rules.  The distribution tests
(tests/test_emu_random.py, test_emu_poisson.py, test_generators_gpu.py, test_poisson_gpu.py) check that the LAWS are the
reference's; this file checks that the STREAM is the documented one, which no chi-square can see.

The runner calls the C entry points on guarded buffers (tests/fft_cases.py Guarded), every call twice on fresh outputs with
identical bits, operands unchanged.

Counts.  What may differ between devices is the limit exp(-lambda) of the small rates and, where the rate is not an exact
quotient, the rate: the replay runs with both float32 neighbours of the correctly rounded limit (the count is non-increasing in
the limit) and, for an inexact rate, with the correctly rounded rate and its two neighbours; the device's output has to be one
of these outcomes.  (The kernel takes the limit in fp64 and rounds it once.  With expf it missed this rule on the MI355X in 1 of
4 195 305 elements of poisson-grid-flat: the device's expf was measured up to 6.1 ulp, at 8.5494995 three floats, away from the
correctly rounded value, and that element's fifth product lies one float below it.)
An element is OPEN when the two limits give different counts, or when its PTRS replay meets a floor argument within 8 fp64 ulp
of an integer or a V within 8 ulp of vr (left out of the comparison, reported by index); the share of open elements is asserted
at most OPEN_CAP per case from the reference alone.  A PTRS acceptance test whose margin is below the error of the fp64 formula
is decided with mpmath at 50 digits, and every one at a rate above 1e6.

Values.  Per element |out - ref| <= c U M with U = 2^-24, c counted in BOUNDS."""
from dataclasses import dataclass

import numpy as np
import torch
from scipy.special import gammaln

from fft_cases import GUARD, POISON, Guarded

U = 2.0 ** -24
F32, F64, U64 = np.float32, np.float64, np.uint64
INF, NAN = float("inf"), float("nan")
POISSON, POISSON_GAUSSIAN, POISSON_LOG = 0, 1, 2                  # include/deepinv_amd.h DINV_POISSON*
NORMALIZE, CLIP_POSITIVE = 1, 2
PTRS_FROM = 10.0
MAX_ROUNDS = 64
MASK_ROW_COUNTERS = 1024                                          # (4096 + 3) / 4 counters per (batch, time) row
MAXW = 4096
OPEN_CAP = 1e-4
MP_ABOVE = 1e6                                                    # every log test above this rate is decided with mpmath
# the error of  -l + k log l - lgamma(k + 1)  against  log(V inv_alpha / (a / us^2 + b))  in fp64, in units of
# 2^-53 (k |log l| + lgamma(k + 1) + l): log l (1, times k), the product (1), gammaln (4: scipy documents no bound, its
# Lanczos / Stirling code is a handful of operations), the two sums (2), and the left side - six operations on a value below
# the terms on the right (6) -: 14, taken as 16
LOG_TEST_ROUNDINGS = 16

# ------------------------------------------------------------------ the bounds: c of |out - ref| <= c U M, counted
# Function errors from the HIP math API reference, "Single precision mathematical functions" (the table tests/loop_algebra_cases.py
# cites for expf): logf, sqrtf, sinf, cosf 1 ULP each, 1 ulp = 2 U relative.  (For the record, after each entry: the worst error /
# bound on the MI355X over the table, as tests/test_random_kernels_gpu.py prints it.)
# One normal deviate z = r cos t (or sin), r = sqrt(-2 log u): logf 2 on |log u|, halved by the root: 1; sqrtf: 2; the angle
# t = 2 pi u <= 2 pi: the float constant is 2 pi (1 + 0.47 U): 2.94 U absolute, the product's rounding half an ulp of [4, 8): 4 U,
# together below 7 U absolute on the angle and so on cos / sin; cosf / sinf: 2; the product r cos t: 1.  13 U r.
_DEVIATE = 1 + 2 + 7 + 2 + 1
BOUNDS = {
    "gaussian": _DEVIATE + 1,           # fmaf(s, z, x): the deviate's 13 on |s| r, one rounding on |x| + |s| r.  0.49 (gaussian-n8389811)
    "poisson_count": 0,                 # a count below 2^24 is exact; above, (float)k is the correctly rounded one: exact as well
    "poisson_scaled": 1,                # k g: one product.  0.932 (poisson-normalize-g0.3)
    # k g + n0 s as an fma of one product: 13 on |s| r, two roundings on k g + |s| r.  0.423 (poisson-gaussian-clip-g0.3)
    "poisson_gaussian": _DEVIATE + 2,
    # -logf(k / g) / s: (float)k and the quotient, 2 on the argument and so absolute on the log; logf 2 on |log|; the division
    # by s 1 on |log|: below 4 U (1 + |log(k / g)|) / s
    "poisson_log": 4,                   # 0.615 (poisson-log-1024)
}


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the replay: generator and uniforms
_M0, _M1, _W0, _W1, _LO = U64(0xD2511F53), U64(0xCD9E8D57), U64(0x9E3779B9), U64(0xBB67AE85), U64(0xFFFFFFFF)
_S32 = U64(32)


def philox_block(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11; Random123): four counter words and two key words, as uint64 arrays of 32-bit values"""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(v, dtype=U64)) for v in counter)
    k0, k1 = (np.atleast_1d(np.asarray(v, dtype=U64)) for v in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def philox(seed, ctr, stream, rnd=0):
    """the kernels' layout (header comment of csrc/random.hip): counter (ctr_lo, ctr_hi, stream, round), key (seed_lo, seed_hi)"""
    ctr = np.atleast_1d(np.asarray(ctr, dtype=U64))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox_block((ctr & _LO, ctr >> _S32, np.full_like(ctr, stream), np.full_like(ctr, rnd)),
                        (U64(seed & 0xFFFFFFFF), U64(seed >> 32)))


def counters(offset, index):
    """offset + index modulo 2^64"""
    with np.errstate(over="ignore"):
        return np.atleast_1d(np.asarray([int(offset) & 0xFFFFFFFFFFFFFFFF], dtype=U64) + np.asarray(index, dtype=U64))


def u01(r):
    """(0, 1] in float32: (r >> 8) 2^-24 + 2^-25; the product is exact, the sum rounds once"""
    return (r >> U64(8)).astype(F32) * F32(2.0 ** -24) + F32(2.0 ** -25)


def box_muller64(a, b):
    """(r cos t, r sin t, r) in fp64 from two words"""
    ua, ub = u01(a).astype(F64), u01(b).astype(F64)
    r = np.sqrt(-2.0 * np.log(ua))
    t = 2.0 * np.pi * ub
    return r * np.cos(t), r * np.sin(t), r


# ------------------------------------------------------------------ the replay: Gaussian noise
def gaussian_deviates(n, seed, offset):
    """(z, r) of elements 0..n-1: quad q owns counter offset + q of stream 0, its words the elements 4q..4q+3"""
    nq = cdiv(n, 4)
    w = philox(seed, counters(offset, np.arange(nq, dtype=U64)), 0)
    z0, z1, r01 = box_muller64(w[0], w[1])
    z2, z3, r23 = box_muller64(w[2], w[3])
    return np.stack([z0, z1, z2, z3], 1).reshape(-1)[:n], np.stack([r01, r01, r23, r23], 1).reshape(-1)[:n]


def gaussian_reference(n, x, sigma, seed, offset):
    """(ref, M) of y = x + sigma z: x None or [n], sigma [n] (per element), both fp64"""
    z, r = gaussian_deviates(n, seed, offset)
    x = np.zeros(n) if x is None else x
    return x + sigma * z, np.abs(x) + np.abs(sigma) * r


def gaussian_advance(n):
    return 4 * cdiv(cdiv(n, 4), 4)


def poisson_advance(n):
    return 4 * cdiv(n, 4)


def mask_advance(B, T):
    return 4 * cdiv(B * T * MASK_ROW_COUNTERS + B, 4)


# ------------------------------------------------------------------ the replay: the Poisson draw
def _knuth(lam, seed, ctr):
    """multiplication in float32 (a product chain has no contraction): the counts for the upper and the lower float32
    neighbour of the correctly rounded exp(-lambda): (k_lo, k_hi)"""
    limit = np.exp(-lam.astype(F64)).astype(F32)
    lim_hi, lim_lo = np.nextafter(limit, F32(INF)), np.nextafter(limit, F32(0))
    n = lam.size
    prod = np.ones(n, F32)
    k = [np.zeros(n), np.zeros(n)]
    done = [np.zeros(n, bool), np.zeros(n, bool)]
    for rnd in range(MAX_ROUNDS):
        idx = np.nonzero(~done[1])[0]
        if idx.size == 0:
            break
        w = philox(seed, ctr[idx], 4, rnd)
        p = prod[idx]
        kk = [k[0][idx], k[1][idx]]
        dd = [done[0][idx], done[1][idx]]
        for e in range(4):
            p = p * u01(w[e])
            for j, lim in ((0, lim_hi[idx]), (1, lim_lo[idx])):
                dd[j] |= ~(p > lim)
                kk[j] += ~dd[j]
        prod[idx] = p
        for j in (0, 1):
            k[j][idx], done[j][idx] = kk[j], dd[j]
    return k[0], k[1]


def _mp_accepts(V, inv_alpha, a, us, b, k, l):
    import mpmath as mp

    with mp.workdps(50):
        V, inv_alpha, a, us, b, k, l = (mp.mpf(float(v)) for v in (V, inv_alpha, a, us, b, k, l))
        return bool(mp.log(V * inv_alpha / (a / (us * us) + b)) <= -l + k * mp.log(l) - mp.loggamma(k + 1))


def _ptrs(lam, seed, ctr, stats):
    """Hoermann, "The transformed rejection method for generating Poisson random variables", Insurance: Mathematics and
    Economics 12 (1993) 39-45, algorithm PTRS, in fp64 without contraction: (k, open).  With stats["first"] = {} the candidate and
    the margin log pmf - lhs of every element's first-round acceptance test are recorded there (NaN where the round has none)"""
    l = lam.astype(F64)
    slam = np.sqrt(l)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    inv_alpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    n = l.size
    k, done, opened = np.floor(l), np.zeros(n, bool), np.zeros(n, bool)
    for rnd in range(MAX_ROUNDS):
        idx = np.nonzero(~done)[0]
        if idx.size == 0:
            break
        w = philox(seed, ctr[idx], 4, rnd)
        li, bi, ai, ia, vri = l[idx], b[idx], a[idx], inv_alpha[idx], vr[idx]
        Uc = (w[0].astype(F64) + 0.5) * 2.0 ** -32 - 0.5
        V = (w[1].astype(F64) + 0.5) * 2.0 ** -32
        us = 0.5 - np.abs(Uc)
        t = (2.0 * ai / us + bi) * Uc
        x = t + li + 0.43
        kk = np.floor(x)
        skip = (us < 0.013) & (V > us)                   # rejected whatever k is
        squeeze = (us >= 0.07) & (V <= vri)
        # a floor that 8 ulp move: next to an integer, or, where every double is an integer, a sum that does not round to l alone
        ulp = np.spacing(x)
        near = np.where(ulp >= 1.0, np.abs(t) + 0.43 >= 0.25 * np.spacing(li), np.minimum(x - kk, kk + 1.0 - x) <= 8 * ulp)
        near |= (us >= 0.07) & (np.abs(V - vri) <= 8 * np.spacing(vri))
        opened[idx] |= near & ~skip
        test = ~skip & ~squeeze & ~(kk < 0)
        accept = squeeze.copy()
        ti = np.nonzero(test)[0]
        if ti.size:
            kt, lt = kk[ti], li[ti]
            lg = gammaln(kt + 1.0)
            loglt = np.log(lt)
            lhs = np.log(V[ti] * ia[ti] / (ai[ti] / (us[ti] * us[ti]) + bi[ti]))
            rhs = -lt + kt * loglt - lg
            ok = lhs <= rhs
            err = LOG_TEST_ROUNDINGS * 2.0 ** -53 * (kt * np.abs(loglt) + lg + lt)
            stats["log_tests"] += ti.size
            if rnd == 0 and "first" in stats:
                stats["first"]["k"], stats["first"]["margin"] = np.full(n, NAN), np.full(n, NAN)
                stats["first"]["k"][idx[ti]], stats["first"]["margin"][idx[ti]] = kt, rhs - lhs
            stats["margin"] = min(stats["margin"], float(np.min(np.abs(lhs - rhs))))
            for j in np.nonzero((np.abs(lhs - rhs) <= err) | (lt > MP_ABOVE))[0]:
                i = ti[j]
                ok[j] = _mp_accepts(V[i], ia[i], ai[i], us[i], bi[i], kt[j], lt[j])
                stats["mpmath"] += 1
            accept[ti] = ok
        acc = idx[accept]
        k[acc], done[acc] = kk[accept], True
    return k, opened


def poisson_counts(lam, seed, ctr, stats=None):
    """the counts of the float32 rates lam at the counters ctr: (k_lo, k_hi, open) in fp64; NaN for a NaN or negative rate,
    the rate itself for 0 and +inf, as the kernel defines them"""
    stats = stats if stats is not None else new_stats()
    lam = np.asarray(lam, dtype=F32)
    k_lo = np.full(lam.size, NAN)
    k_hi = k_lo.copy()
    opened = np.zeros(lam.size, bool)
    with np.errstate(invalid="ignore"):
        same = (lam == 0) | (lam == INF)
        small = (lam > 0) & (lam < F32(PTRS_FROM))
        large = (lam >= F32(PTRS_FROM)) & (lam < INF)
    k_lo[same] = k_hi[same] = lam[same]
    if small.any():
        k_lo[small], k_hi[small] = _knuth(lam[small], seed, ctr[small])
        opened[small] = k_lo[small] != k_hi[small]
    if large.any():
        k_lo[large], opened[large] = _ptrs(lam[large], seed, ctr[large], stats)
        k_hi[large] = k_lo[large]
    return k_lo, k_hi, opened


def new_stats():
    return {"log_tests": 0, "mpmath": 0, "margin": INF}


def _is_pow2(g):
    m, _ = np.frexp(g.astype(F64))
    return np.isfinite(g) & (m == 0.5)


def poisson_reference(x, gain, sigma, mode, flags, min_gain, seed, offset, stats=None):
    """what dinv_poisson_noise may write for the float32 inputs x [n] with the per-element float32 gain and sigma [n]:
    {"cands": [(ref, bound), ...] in fp64, "open": the elements whose count the reference leaves open, "excluded": those left out
    of the comparison (PTRS next to a discontinuity), "bad": the two flags}"""
    stats = stats if stats is not None else new_stats()
    x, g, s = (np.asarray(v, dtype=F32) for v in (x, gain, sigma))
    n = x.size
    ctr = counters(offset, np.arange(n, dtype=U64))
    with np.errstate(all="ignore"):
        if mode == POISSON_GAUSSIAN:
            g = np.where(np.isnan(g), g, np.maximum(g, F32(min_gain)))
        bad = [0, 0]
        if mode == POISSON_LOG:
            arg = (-x * s).astype(F64)
            lam = (g.astype(F64) * np.exp(arg)).astype(F32)
            exact = np.zeros(n, bool)
        else:
            lam = x / g
            exact = _is_pow2(g)
            if flags & CLIP_POSITIVE:
                lam = np.where(np.isnan(lam), lam, np.maximum(lam, F32(0)))
            else:
                bad[0] = int(bool((x < 0).any()))
            bad[1] = int(bool((~(g > 0)).any()))
        rates = [lam]
        inexact = ~exact & np.isfinite(lam) & (lam > 0)
        if inexact.any():
            rates += [np.where(inexact, np.nextafter(lam, F32(0)), lam), np.where(inexact, np.nextafter(lam, F32(INF)), lam)]
        counts, opened, excluded = [], None, None
        for j, rate in enumerate(rates):
            sel = np.ones(n, bool) if j == 0 else inexact
            k_lo, k_hi, op = poisson_counts(rate[sel], seed, ctr[sel], stats)
            if j == 0:
                width = k_hi - k_lo
                assert not (width[np.isfinite(width)] > 1).any(), "a bracket wider than one count"
                opened, excluded = op, op & (k_lo == k_hi)             # PTRS-open elements have one count: those are left out
                base = (k_lo, k_hi)
                counts += [k_lo, k_hi]
            else:
                for kk, b0 in ((k_lo, base[0]), (k_hi, base[1])):
                    full = b0.copy()
                    full[sel] = kk
                    counts.append(full)
                ex = np.zeros(n, bool)
                ex[sel] = op & (k_lo == k_hi)
                excluded = excluded | ex
        g64, s64 = g.astype(F64), s.astype(F64)
        if mode == POISSON_GAUSSIAN:
            w = philox(seed, ctr, 5)
            n0, _, r = box_muller64(w[0], w[1])
        cands = []
        for k in counts:
            kf = k.astype(F32).astype(F64)                                 # (float)k of a double: correctly rounded
            if mode == POISSON_LOG:
                lg = np.log(kf / g64)
                ref, bound = -lg / s64, BOUNDS["poisson_log"] * U * (1 + np.abs(lg)) / np.abs(s64)
            elif mode == POISSON_GAUSSIAN:
                ref = kf * g64 + n0 * s64
                bound = BOUNDS["poisson_gaussian"] * U * (np.abs(kf * g64) + np.abs(s64) * r)
            elif flags & NORMALIZE:
                ref = kf * g64
                bound = BOUNDS["poisson_scaled"] * U * np.abs(ref)
            else:
                ref, bound = kf, np.zeros(n)
            cands.append((ref, bound))
    return {"cands": cands, "open": opened, "excluded": excluded, "bad": bad, "stats": stats}


def poisson_compare(tag, out, ref):
    """every element that is not left out equals one of the outcomes or lies within its bound; the share of open elements is
    below the cap; returns the worst error / bound"""
    n = out.size
    out = out.astype(F64)
    share = float(ref["open"].sum()) / max(n, 1)
    st = ref["stats"]
    left = np.nonzero(ref["excluded"])[0]
    print(f"{tag}: {int(ref['open'].sum())} of {n} elements open (share {share:.3g}), left out: {left.tolist()[:16]}; "
          f"{st['log_tests']} log tests, smallest margin {st['margin']:.3g}, {st['mpmath']} decided with mpmath")
    assert share <= OPEN_CAP, f"{tag}: {share:.3g} of the elements are open, above {OPEN_CAP}"
    best = np.full(n, INF)
    with np.errstate(all="ignore"):
        for r, b in ref["cands"]:
            same = (out == r) | (np.isnan(out) & np.isnan(r))
            ratio = np.where(same, 0.0, np.where(b > 0, np.abs(out - r) / b, INF))
            ratio = np.where(np.isnan(ratio), INF, ratio)
            best = np.minimum(best, ratio)
    best[ref["excluded"]] = 0.0
    worst, at = float(best.max(initial=0.0)), int(best.argmax()) if n else 0
    print(f"{tag}: worst element {at} error / bound {worst:.3g}")
    if worst > 1.0:
        wrong = np.nonzero(best > 1.0)[0]
        raise AssertionError(f"{tag}: {wrong.size} of {n} elements are none of the replayed outcomes, the first at {wrong[:8].tolist()}: "
                             f"{out[wrong[:4]].tolist()} for {[float(r[wrong[0]]) for r, _ in ref['cands']]}")
    return worst


# ------------------------------------------------------------------ the replay: mask lines
def _mask_uniforms(rows, W, stream, seed, offset):
    """u [rows, W]: row r, column w: counter offset + r 1024 + (w >> 2), word w & 3"""
    nq = cdiv(W, 4)
    with np.errstate(over="ignore"):
        idx = (np.arange(rows, dtype=U64)[:, None] * U64(MASK_ROW_COUNTERS) + np.arange(nq, dtype=U64)[None, :]).reshape(-1)
    w = philox(seed, counters(offset, idx), stream)
    return np.stack([u01(v) for v in w], 1).reshape(rows, 4 * nq)[:, :W]


def mask_reference(B, T, W, n_lines, c_lo, c_hi, mode, pdf, accel, n_offsets, seed, offset):
    """(must, may, count) over [B T, W]: columns that have to be set, columns that may take either value, and the number of set
    columns per row where it is fixed (mode 0), else None"""
    rows = B * T
    centre = (np.arange(W) >= c_lo) & (np.arange(W) < c_hi)
    must = np.tile(centre, (rows, 1))
    may = np.zeros((rows, W), bool)
    count = None
    if mode == 2:
        return _mask_uniforms(rows, W, 3, seed, offset) <= np.asarray(pdf, dtype=F32)[None, :], may, None
    if mode == 0:
        p = np.asarray(pdf, dtype=F32).astype(F64)
        pos = p > 0
        n_eff = min(int(n_lines), int(pos.sum()))
        count = n_eff + int((centre & ~pos).sum())
        if n_eff == int(pos.sum()):
            return must | pos[None, :], may, count
        if n_eff == 0:
            return must, may, count
        u = _mask_uniforms(rows, W, 1, seed, offset)[:, pos].astype(F64)
        with np.errstate(divide="ignore"):
            lp, L = np.log(p[pos])[None, :], -np.log(u)
            key = lp - np.log(L)
            # the fp32 key: logf(p) 2 U |log p|; logf(u) 2 U relative on L, so 2 U absolute on log L; logf(L) 2 U |log L|; the
            # difference 1 U |key|
            delta = U * (2 * np.abs(lp) + 2 + 2 * np.abs(np.log(L)) + np.abs(key))
        delta = np.where(np.isfinite(delta), delta, 0.0)
        order = np.argsort(-key, axis=1)
        nth = order[:, n_eff - 1]
        kn, dn = key[np.arange(rows), nth][:, None], delta[np.arange(rows), nth][:, None]
        sure, unsure = key > kn + (delta + dn), np.abs(key - kn) <= delta + dn
        must[:, pos] |= sure
        may[:, pos] = unsure & ~centre[pos][None, :]
        return must, may, count
    # equispaced: offset_b = word 0 of (offset + b, stream 2) modulo n_offsets; columns round(start + k accel) below W - 1
    w0 = philox(seed, counters(offset, np.arange(B, dtype=U64)), 2)[0]
    off = (w0 % U64(n_offsets)).astype(np.int64) if n_offsets > 0 else np.zeros(B, np.int64)
    kmax = int((W - 1) / accel) + 2
    ks = np.arange(kmax, dtype=F64)
    for b in range(B):
        for t in range(T):
            start = np.fmod(float(t + off[b]), accel)
            v = start + ks * accel
            sets = []
            for vv in (v - 1e-9, v, v + 1e-9):              # the device contracts start + k accel to an fma
                live = vv < W - 1
                col = np.rint(vv.astype(F32)).astype(np.int64)
                live &= (col >= 0) & (col < W)
                line = np.zeros(W, bool)
                line[col[live]] = True
                sets.append(line)
            row = b * T + t
            must[row] |= sets[0] & sets[1] & sets[2]
            may[row] = (sets[0] | sets[1] | sets[2]) & ~must[row]
    return must, may, count


# ------------------------------------------------------------------ the launchers' grid rules, restated (csrc/random.hip)
GAUSS_CAP, POISSON_CAP, POISSON_Y_CAP = 8192, 16384, 65535


def gaussian_blocks(n):
    return min(cdiv(cdiv(n, 4), 256), GAUSS_CAP)


def poisson_grid(batch, per):
    by = min(batch, POISSON_Y_CAP)
    return max(min(cdiv(per, 256), POISSON_CAP // by), 1), by


# ------------------------------------------------------------------ the case tables
SEEDS = [(77, 0), (0x1234567811223344, 2 ** 32 - 3), (0xFFFFFFFF00000001, 2 ** 33 + 12345), (2 ** 63 + 5, 2 ** 32 - 7000),
         (1234, 16), (0x8000000000000000, 2 ** 64 - 2 ** 20)]


@dataclass(frozen=True)
class Gauss:
    n: int
    form: str = "scalar"          # scalar | nullx | table1 | batch
    pick: int = 0                 # the (seed, offset) pair
    emu: bool = True

    @property
    def id(self):
        return f"gaussian-n{self.n}-{self.form}-s{self.pick}"


GAUSS_BATCH, GAUSS_PER = 5, 1001
GAUSS_BIG = 4 * (GAUSS_CAP * 256) + 4 * 300 + 3
GAUSS_SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1027]
GAUSS_TABLE = ([Gauss(n, "scalar", i % len(SEEDS)) for i, n in enumerate(GAUSS_SIZES)]
               + [Gauss(n, "nullx", (i + 1) % len(SEEDS)) for i, n in enumerate((1, 5, 1027))]
               + [Gauss(n, "table1", (i + 2) % len(SEEDS)) for i, n in enumerate((3, 1027))]
               + [Gauss(GAUSS_BATCH * GAUSS_PER, "batch", p) for p in (1, 2)]
               + [Gauss(GAUSS_BIG, "scalar", 3, emu=False)])

_TEN = F32(PTRS_FROM)
RATES = [0.0, -0.0, 1e-30, 0.01, 3.0, 9.99, float(np.nextafter(_TEN, F32(0))), 10.0, float(np.nextafter(_TEN, F32(20))), 10.01,
         12.0, 30.0, 1e3, 1e5, 1e6, 2e7, 3e38, INF, NAN, -1.0, -INF]


@dataclass(frozen=True)
class Pois:
    name: str
    mode: int = POISSON
    flags: int = 0
    gain: tuple = (1.0,)          # one value, or one per sample
    sigma: tuple = (0.0,)
    min_gain: float = 0.0
    batch: int = 1
    per: int = 0                  # 0: the rate table, flat
    pick: int = 0
    rates: str = "table"          # table | mixed | log
    emu: bool = True

    @property
    def id(self):
        return f"poisson-{self.name}"


def _cycle(values, n):
    return tuple(values[i % len(values)] for i in range(n))


POIS_TABLE = [
    Pois("plain", pick=1),
    Pois("clip", flags=CLIP_POSITIVE, pick=2),
    Pois("normalize-g0.5", flags=NORMALIZE, gain=(0.5,), pick=3),
    Pois("normalize-clip-g4", flags=NORMALIZE | CLIP_POSITIVE, gain=(4.0,), pick=0),
    Pois("normalize-g0.3", flags=NORMALIZE, gain=(0.3,), pick=4),                  # an inexact quotient: three candidate rates
    Pois("gaussian-g0.5", POISSON_GAUSSIAN, gain=(0.5,), sigma=(0.25,), pick=5),
    Pois("gaussian-clip-g0.3", POISSON_GAUSSIAN, CLIP_POSITIVE, gain=(0.3,), sigma=(1.5,), pick=1),
    Pois("gaussian-min-gain", POISSON_GAUSSIAN, gain=(0.0,), sigma=(0.1,), min_gain=0.25, pick=2),
    Pois("gaussian-zero-gain", POISSON_GAUSSIAN, gain=(0.0,), sigma=(0.1,), min_gain=0.0, pick=2),       # the flag alone
    Pois("tables-normalize", flags=NORMALIZE, gain=(0.5, 1.0, 2.0, 0.25), batch=4, per=757, pick=3, rates="mixed"),
    Pois("tables-gaussian", POISSON_GAUSSIAN, gain=(0.5, 1.0, 2.0, 0.3), sigma=(0.0, 0.1, 1.0, 2.0), batch=4, per=757, pick=0,
         rates="mixed"),
    Pois("log-1024", POISSON_LOG, gain=(1024.0,), sigma=(0.02,), pick=4, rates="log"),
    Pois("log-7", POISSON_LOG, gain=(7.0,), sigma=(0.5,), pick=5, rates="log"),
    # geometry, mixed rates.  x cap, flat; x cap at 16384 / 64; 16384 / by = 0: one workgroup in x, strided; the y cap and the b loop
    Pois("grid-flat", batch=1, per=POISSON_CAP * 256 + 1001, pick=3, rates="mixed", emu=False),
    Pois("grid-b64", flags=NORMALIZE, gain=_cycle((0.5, 1.0, 2.0), 64), batch=64, per=65536 + 257, pick=1, rates="mixed", emu=False),
    Pois("grid-b16385", flags=NORMALIZE, gain=_cycle((1.0, 0.5, 2.0), 16385), batch=16385, per=259, pick=2, rates="mixed", emu=False),
    Pois("grid-b65538", gain=_cycle((1.0,), 65538), batch=65538, per=3, pick=3, rates="mixed"),
]
POIS_BIG = [c.id for c in POIS_TABLE if c.batch * c.per > 200_000]


@dataclass(frozen=True)
class Mask:
    name: str
    mode: int
    W: int
    B: int = 3
    C: int = 2
    T: int = 2
    H: int = 3
    n_lines: int = 0
    centre: tuple = (0, 0)
    pdf: str = ""                 # gauss (zero on the centre) | bernoulli
    accel: float = 1.0
    n_offsets: int = 0
    pick: int = 0
    emu: bool = True

    @property
    def id(self):
        return f"mask-mode{self.mode}-{self.name}-W{self.W}"


MASK_WIDTHS = [1, 3, 255, 256, 257, 320, MAXW]


def _centre(W, frac=0.08):
    nc = int(frac * W)
    return (W // 2 - nc // 2, W // 2 - nc // 2 + nc)


def _mask_table():
    t = []
    for i, W in enumerate(MASK_WIDTHS):
        B, T, H = (2, 2, 1) if W == MAXW else (3, 2, 3)
        c = _centre(W)
        free = W - (c[1] - c[0])
        t.append(Mask("typical", 0, W, B, 2, T, H, n_lines=max(free // 4, min(free, 1)), centre=c, pdf="gauss", pick=i % len(SEEDS)))
        t.append(Mask("bernoulli", 2, W, B, 2, T, H, centre=c, pdf="bernoulli", pick=(i + 1) % len(SEEDS)))
        t.append(Mask("integer", 1, W, B, 2, 7, H, centre=c, accel=4.0, n_offsets=4, pick=(i + 2) % len(SEEDS)))
        t.append(Mask("fraction", 1, W, B, 2, 7, H, centre=c, accel=3.7 + W / 65536.0, n_offsets=4, pick=(i + 3) % len(SEEDS)))
    for W in (3, 257, 320):
        c = _centre(W)
        free = W - (c[1] - c[0])
        t.append(Mask("none", 0, W, n_lines=0, centre=c, pdf="gauss", pick=1))
        t.append(Mask("all", 0, W, n_lines=free, centre=c, pdf="gauss", pick=2))
        t.append(Mask("five-more", 0, W, n_lines=free + 5, centre=c, pdf="gauss", pick=3))
        t.append(Mask("no-centre", 0, W, n_lines=max(W // 8, 1), centre=(W // 2, W // 2), pdf="gauss", pick=4))
        t.append(Mask("all-centre", 0, W, n_lines=4, centre=(0, W), pdf="gauss", pick=5))
        t.append(Mask("no-offsets", 1, W, T=5, centre=c, accel=4.0, n_offsets=0, pick=1))
    t.append(Mask("lone", 0, 320, B=1, C=1, T=1, H=1, n_lines=40, centre=_centre(320), pdf="gauss", pick=1))    # H W = 320: 256 and a rest
    t.append(Mask("time", 1, 64, B=16, C=1, T=8, H=2, centre=(31, 33), accel=(8 * (2 - 64)) / (2 * 8 - 64), n_offsets=9, pick=3))
    return t


MASK_TABLE = _mask_table()


# Elements whose first PTRS acceptance test is nearly a tie: counters of seed TIGHT_SEED at the rate 10, found by a search
# over the first 1.7e8 of them.  A chi-square cannot see a log pmf that is off by 1e-5; these elements change their count when it
# is off by less: for every candidate k = 2..9 (the table of log k!) two elements on either side of the tie with a margin below
# 2e-5, and for k = 10..15 (the Stirling series) up to four on either side (at 15: below the tie only) with a margin below 0.4 of the k^-3 term's double,
# 2 / (360 k^3) - what a wrong sign of that term moves the log pmf by - and above 1e-9, a thousand times the series' truncation.
# tests/test_emu_random_cases.py asserts these properties from the replay alone.
TIGHT_SEED, TIGHT_RATE = 77, 10.0
TIGHT = (115433763, 151451279, 77776424, 77616840, 167317150, 149605640, 157522103, 23796307, 21171573, 167372493, 68892537, 116193490,
         66375766, 16318699, 8255555, 122735372, 122669496, 46371761, 87654481, 89919205, 99968086, 157768436, 82758204, 136944267,
         106377906, 57402998, 81886569, 53683528, 96122447, 14225473, 165785334, 140871925, 92253304, 101438189, 59922749, 54146206,
         27542940, 69870082, 80566278, 140727039, 88681042, 143924695, 57379319, 137177423, 52501405, 36698075, 5709633, 6441939,
         123935745, 149777799, 98300065, 123690241, 8821376, 30940127, 41616341, 108861954, 143658600, 47897938, 136729612, 135249747,
         104253264, 128716726, 153214618, 11400022, 97199029, 164295633, 133056071, 757292, 102860525, 164458133, 52161724, 82724230,
         84109484, 59002271)


def tight_margins():
    """(k, margin) of the first-round acceptance test of every element of TIGHT, from the replay"""
    stats = new_stats()
    stats["first"] = {}
    ctr = np.asarray(TIGHT, dtype=U64)
    poisson_counts(np.full(ctr.size, TIGHT_RATE, F32), TIGHT_SEED, ctr, stats)
    return stats["first"]["k"], stats["first"]["margin"]


def stirling_term(k):
    """twice the k^-3 term of the Stirling series of log k!"""
    return 2.0 / (360.0 * k ** 3)


@dataclass(frozen=True)
class Tight:
    emu: bool = True
    id: str = "poisson-tight-margins"


TABLE = GAUSS_TABLE + POIS_TABLE + [Tight()] + MASK_TABLE
assert len({c.id for c in TABLE}) == len(TABLE), "duplicate case ids"


def _seed(cid):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(cid)) % (2 ** 31)


def mask_pdf(c):
    """float32 column probabilities of a mask case"""
    W, (lo, hi) = c.W, c.centre
    col = np.arange(W, dtype=F64)
    if c.pdf == "gauss":
        p = np.exp(-(0.5 / (W / 10.0) ** 2) * (col - W / 2) ** 2) + 0.125
        p[lo:hi] = 0
        if W >= 255:
            p[5] = p[W - 7] = 0                           # zero-probability columns outside the centre
        return (p / max(p.sum(), 1e-300)).astype(F32)
    if c.pdf == "bernoulli":
        p = np.clip((1 - np.abs(np.linspace(-1, 1, W))) ** 4 + 0.05, 0, 1)
        p[lo:hi] = 1
        if W >= 3:
            p[0], p[W - 1] = 0.0, 1.0
        return p.astype(F32)
    return None


def poisson_inputs(c):
    """(x [n] float32, gain [n], sigma [n], batch, per) of a Poisson case: the rates of the table, or mixed rates - half uniform
    below 10, half log-uniform in [10, 1e6], the edges among them - times the sample's gain"""
    rng = np.random.default_rng(_seed(c.id))
    if c.per == 0:
        batch, per = 1, 150 * len(RATES) + 3
    else:
        batch, per = c.batch, c.per
    n = batch * per
    g = np.repeat(np.asarray(_cycle(c.gain, batch), dtype=F32), per)
    s = np.repeat(np.asarray(_cycle(c.sigma, batch), dtype=F32), per)
    if c.rates == "log":
        x = np.linspace(0.0, 400.0 if c.gain[0] > 100 else 12.0, n).astype(F32)
        x[7::97] = NAN
        x[3] = INF                                        # rate 0: a count of 0, +inf out
    elif c.rates == "table":
        x = np.asarray(RATES, dtype=F32)[np.arange(n) % len(RATES)]
        with np.errstate(all="ignore"):
            x = np.where(_is_pow2(g) & np.isfinite(x), x * g, x).astype(F32)          # the rate itself where the quotient is exact
    else:
        lam = np.where(rng.random(n) < 0.5, rng.random(n) * 10.0, 10.0 ** (1.0 + 5.0 * rng.random(n))).astype(F32)
        edges = np.asarray([0.0, 1e-30, 9.99, 10.0, 10.01, 12.0, 1e6] + RATES[6:9:2], dtype=F32)
        at = rng.integers(0, n, 4 * edges.size)
        lam[at] = edges[np.arange(at.size) % edges.size]
        with np.errstate(all="ignore"):
            gg = np.where(g > 0, g, F32(1))
            x = (lam * gg).astype(F32)                    # exact for the gains that are powers of two
    return x, g, s, batch, per


# ------------------------------------------------------------------ the runner
class Runner:
    """the C entry points over one library: `lib` (ctypes, with the prototypes of deepinv_amd.hip.random), `device` of its
    buffers, `stream()` -> the stream argument"""

    def __init__(self, lib, device, stream):
        self.lib, self.device, self._stream = lib, torch.device(device), stream

    def err(self):
        return self.lib.dinv_last_error().decode()

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def gaussian(self, n, per, x, sigma, sigma_f, seed, offset, y):
        return self.lib.dinv_gaussian_noise(n, per, x, sigma, sigma_f, seed, offset, y, self._stream())

    def poisson(self, n, per, x, gain, gain_f, sigma, sigma_f, mode, flags, min_gain, seed, offset, bad, y):
        return self.lib.dinv_poisson_noise(n, per, x, gain, gain_f, sigma, sigma_f, mode, flags, min_gain, seed, offset, bad, y,
                                           self._stream())

    def mask(self, B, C, T, H, W, n_lines, lo, hi, mode, pdf, accel, n_offsets, seed, offset, mask):
        return self.lib.dinv_mri_mask_lines(B, C, T, H, W, n_lines, lo, hi, mode, pdf, accel, n_offsets, seed, offset, mask,
                                            self._stream())


def _p(g):
    return None if g is None else g.t.data_ptr()


def _copy(r, a):
    """a guarded device copy of the float32 numpy array a, and its bits"""
    a = np.ascontiguousarray(a, dtype=F32)
    g = Guarded(a.size, r.device)
    g.t.copy_(torch.from_numpy(a))
    return g, g.bits().clone()


def _zeros_i32(r, n):
    g = Guarded(n, r.device)
    g.full[GUARD:GUARD + n] = 0
    return g


def _ok(tag, r, rc, outs, operands):
    assert rc == 0, f"{tag}: error {rc}: {r.err()}"
    r.sync()
    for name, g in outs.items():
        assert g.guards_intact(), f"{tag}: write outside {name}"
        bad = g.bits() == POISON
        assert not bool(bad.any()), f"{tag}: {int(bad.sum())} words of {name} hold the guard pattern: never written"
    for name, (g, before) in operands.items():
        assert g.guards_intact() and torch.equal(g.bits(), before), f"{tag}: the call modified {name}"


def twice(tag, once):
    a, b = once(), once()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{tag}: two identical calls differ in {k}"
    return a


def _ratio(tag, got, ref, measure, c):
    got = got.astype(F64)
    assert not np.isnan(got).any(), f"{tag}: NaN in the result"
    err, bound = np.abs(got - ref), c * U * measure
    zero = bound == 0
    assert bool((err[zero] == 0).all()), f"{tag}: an element with a zero measure is not exact"
    ratio = np.where(zero, 0.0, err / np.maximum(bound, 1e-300))
    worst, at = float(ratio.max()), int(ratio.argmax())
    print(f"{tag}: worst element {at} error / bound {worst:.3g} ({worst * c:.3g} U against c = {c})")
    assert worst <= 1.0, f"{tag}: element {at} is {worst:.3g} times its bound of {c} U M: {got[at]!r} for {ref[at]!r}"
    return worst


# ---- Gaussian noise
def gaussian_inputs(c):
    """(x or None, sigma per element, the call's per_sample, sigma table or None, sigma scalar)"""
    rng = np.random.default_rng(_seed(c.id))
    n = c.n
    x = None if c.form == "nullx" else rng.standard_normal(n).astype(F32)
    if c.form == "batch":
        table = np.asarray([0.5, 0.0, 1.5, 0.01, 2.0], dtype=F32)
        return x, np.repeat(table, GAUSS_PER), GAUSS_PER, table, 0.0
    if c.form == "table1":
        table = np.asarray([0.37], dtype=F32)
        return x, np.full(n, table[0]), n, table, 0.0
    return x, np.full(n, F32(0.37)), n, None, float(F32(0.37))


def run_gaussian(r, c):
    seed, offset = SEEDS[c.pick]
    x, sig, per, table, sig_f = gaussian_inputs(c)
    ops = {}
    if x is not None:
        ops["x"] = _copy(r, x)
    if table is not None:
        ops["sigma"] = _copy(r, table)

    def once():
        y = Guarded(c.n, r.device)
        rc = r.gaussian(c.n, per, _p(ops["x"][0]) if x is not None else None, _p(ops["sigma"][0]) if table is not None else None,
                        sig_f, seed, offset, _p(y))
        _ok(c.id, r, rc, {"y": y}, ops)
        return {"y": y.bits().clone()}

    got = twice(c.id, once)["y"].view(torch.float32).numpy()
    ref, M = gaussian_reference(c.n, None if x is None else x.astype(F64), sig.astype(F64), seed, offset)
    return _ratio(c.id, got, ref, M, BOUNDS["gaussian"])


# ---- Poisson family
def run_poisson(r, c):
    seed, offset = SEEDS[c.pick]
    x, g, s, batch, per = poisson_inputs(c)
    n = x.size
    tables = len(c.gain) > 1 or len(c.sigma) > 1
    ops = {"x": _copy(r, x)}
    if tables:
        ops["gain"], ops["sigma"] = _copy(r, g[::per]), _copy(r, s[::per])
    want_bad = c.mode != POISSON_LOG and not (c.flags & CLIP_POSITIVE)

    def once():
        y = Guarded(n, r.device)
        bad = _zeros_i32(r, 2) if want_bad else None
        rc = r.poisson(n, per, _p(ops["x"][0]), _p(ops["gain"][0]) if tables else None, 0.0 if tables else float(F32(c.gain[0])),
                       _p(ops["sigma"][0]) if tables else None, 0.0 if tables else float(F32(c.sigma[0])), c.mode, c.flags,
                       c.min_gain, seed, offset, _p(bad), _p(y))
        _ok(c.id, r, rc, {"y": y}, ops)
        out = {"y": y.bits().clone()}
        if want_bad:
            assert bad.guards_intact()
            out["bad"] = bad.full[GUARD:GUARD + 2].cpu()
        return out

    res = twice(c.id, once)
    ref = poisson_reference(x, g, s, c.mode, c.flags, c.min_gain, seed, offset)
    if want_bad:
        assert res["bad"].tolist() == ref["bad"], f"{c.id}: flags {res['bad'].tolist()}, expected {ref['bad']}"
    return poisson_compare(c.id, res["y"].view(torch.float32).numpy(), ref)


def run_tight(r, c):
    """one call per element of TIGHT, at its own counter: the count is the replay's"""
    x = np.full(1, TIGHT_RATE, F32)
    ops = {"x": _copy(r, x)}
    for ctr in TIGHT:
        tag = f"{c.id} counter {ctr}"

        def once():
            y = Guarded(1, r.device)
            rc = r.poisson(1, 1, _p(ops["x"][0]), None, 1.0, None, 0.0, POISSON, 0, 0.0, TIGHT_SEED, ctr, None, _p(y))
            _ok(tag, r, rc, {"y": y}, ops)
            return {"y": y.bits().clone()}

        got = float(twice(tag, once)["y"].view(torch.float32)[0])
        k_lo, k_hi, opened = poisson_counts(x, TIGHT_SEED, np.asarray([ctr], dtype=U64))
        assert not opened[0] and k_lo[0] == k_hi[0]
        assert got == k_lo[0], f"{tag}: {got} for the replayed {k_lo[0]}"
    print(f"{c.id}: {len(TIGHT)} elements with nearly tied acceptance tests equal the replay")
    return 0.0


# ---- mask lines
def mask_check(tag, m, B, C, T, H, W, must, may, count):
    """m [B, C, T, H, W] (numpy) against the replayed rows"""
    assert set(np.unique(m).tolist()) <= {0.0, 1.0}, f"{tag}: values other than 0 and 1"
    lines = m[:, 0, :, 0, :]
    assert np.array_equal(m, np.broadcast_to(lines[:, None, :, None, :], m.shape)), f"{tag}: a channel or image row differs from the line"
    got = lines.reshape(B * T, W) == 1.0
    wrong = (must & ~got) | (got & ~must & ~may)
    assert not wrong.any(), (f"{tag}: {int(wrong.any(1).sum())} of {B * T} rows differ from the replay, the first at (row, column) "
                             f"{np.argwhere(wrong)[:4].tolist()}")
    if count is not None:
        assert (got.sum(1) == count).all(), f"{tag}: {got.sum(1).tolist()[:8]} columns per row, expected {count}"
    print(f"{tag}: {B * T} rows equal the replay, {int(may.sum())} columns left open")


def run_mask(r, c):
    seed, offset = SEEDS[c.pick]
    pdf = mask_pdf(c)
    ops = {"pdf": _copy(r, pdf)} if pdf is not None else {}
    size = c.B * c.C * c.T * c.H * c.W

    def once():
        m = Guarded(size, r.device)
        rc = r.mask(c.B, c.C, c.T, c.H, c.W, c.n_lines, c.centre[0], c.centre[1], c.mode, _p(ops["pdf"][0]) if ops else None,
                    c.accel, c.n_offsets, seed, offset, _p(m))
        _ok(c.id, r, rc, {"mask": m}, ops)
        return {"mask": m.bits().clone()}

    m = twice(c.id, once)["mask"].view(torch.float32).numpy().reshape(c.B, c.C, c.T, c.H, c.W)
    must, may, count = mask_reference(c.B, c.T, c.W, c.n_lines, c.centre[0], c.centre[1], c.mode, pdf, c.accel, c.n_offsets, seed, offset)
    mask_check(c.id, m, c.B, c.C, c.T, c.H, c.W, must, may, count)
    return 0.0


def run_case(r, c):
    """runs case c on runner r and returns the worst |error| / bound (0 for the cases that are exact)"""
    return {Gauss: run_gaussian, Pois: run_poisson, Tight: run_tight, Mask: run_mask}[type(c)](r, c)


# ------------------------------------------------------------------ refusals: non-zero status and not a word written
def run_rejections(r):
    B = {k: Guarded(2 * MAXW + 8, r.device) for k in ("x", "y", "sigma", "pdf", "mask", "bad")}
    P = {k: _p(g) for k, g in B.items()}

    def untouched(what):
        r.sync()
        for name, g in B.items():
            assert g.untouched(), f"{what}: {name} was written"

    def refused(what, rc):
        assert rc != 0, f"{what}: accepted"
        assert r.err(), f"{what}: no message"
        untouched(what)

    def nothing(what, rc):
        assert rc == 0, f"{what}: error {rc}: {r.err()}"
        untouched(what)

    refused("gaussian n < 0", r.gaussian(-1, 1, P["x"], None, 1.0, 1, 0, P["y"]))
    refused("gaussian per_sample 0", r.gaussian(64, 0, P["x"], P["sigma"], 1.0, 1, 0, P["y"]))
    refused("gaussian per_sample -5", r.gaussian(64, -5, P["x"], P["sigma"], 1.0, 1, 0, P["y"]))
    refused("gaussian null y", r.gaussian(64, 64, P["x"], None, 1.0, 1, 0, None))
    nothing("gaussian n = 0", r.gaussian(0, 1, P["x"], None, 1.0, 1, 0, P["y"]))
    pz = lambda n, per, mode, flags, x=P["x"], y=P["y"]: r.poisson(n, per, x, None, 1.0, None, 0.0, mode, flags, 0.0, 1, 0, P["bad"], y)
    refused("poisson per_sample does not divide n", pz(64, 3, POISSON, 0))
    refused("poisson per_sample 0", pz(64, 0, POISSON, 0))
    refused("poisson mode 3", pz(64, 64, 3, 0))
    refused("poisson mode -1", pz(64, 64, -1, 0))
    refused("poisson flag 4", pz(64, 64, POISSON, 4))
    refused("poisson flags 7", pz(64, 64, POISSON, 7))
    refused("poisson null x", pz(64, 64, POISSON, 0, x=None))
    refused("poisson null y", pz(64, 64, POISSON, 0, y=None))
    nothing("poisson n = 0", pz(0, 8, POISSON, 0))
    mk = lambda Bn, W, mode, pdf, accel, lo=0, hi=0, n_lines=1: r.mask(Bn, 1, 1, 1, W, n_lines, lo, hi, mode, pdf, accel, 2, 1, 0, P["mask"])
    refused("mask width 4097", mk(1, MAXW + 1, 0, P["pdf"], 1.0))
    refused("mask mode 3", mk(1, 64, 3, P["pdf"], 1.0))
    refused("mask mode -1", mk(1, 64, -1, P["pdf"], 1.0))
    refused("mask mode 0 without pdf", mk(1, 64, 0, None, 1.0))
    refused("mask mode 2 without pdf", mk(1, 64, 2, None, 1.0))
    refused("mask mode 1 acceleration 0", mk(1, 64, 1, None, 0.0))
    refused("mask mode 1 acceleration -4", mk(1, 64, 1, None, -4.0))
    refused("mask centre_lo > centre_hi", mk(1, 64, 0, P["pdf"], 1.0, lo=9, hi=8))
    refused("mask centre_hi > width", mk(1, 64, 0, P["pdf"], 1.0, lo=0, hi=65))
    refused("mask null mask", r.mask(1, 1, 1, 1, 64, 1, 0, 0, 0, P["pdf"], 1.0, 0, 1, 0, None))
    nothing("mask batch = 0", mk(0, 64, 0, P["pdf"], 1.0))
