"""ctypes wrapper of the Gaussian-mixture patch prior of csrc/patch_gmm.hpp (entry points in csrc/dense.hip; include/deepinv_amd.h,
dinv_gmm_*): component scores, classification and negative log-likelihood of patches on the fp32 matrix cores, and the EPLL
half-quadratic step (classify, estimate, aggregate) in three launches; and the sums of an expectation-maximisation step
(csrc/gmm_moments.hpp): responsibilities in one launch (:func:`posterior_rows`), the centred weighted moments of every component
in two (:func:`accumulate_moments`), and the M-step formulas on the downloaded fp64 sums (:func:`em_finalise`, pure torch).  The
launch goes to the current stream of the operands' device.  fp32 only.

The model is handed to the kernels in its eigenbasis (:class:`Operands`): ``Sigma_k = Q_k diag(lam_k) Q_k^T`` from one fp64
``eigh`` on the host, rounded to fp32 once, so that the regularisation ``Sigma_k + r I`` of a half-quadratic step is a runtime
scalar and no matrix is rebuilt between steps.

No autograd: the kernels have no backward, and a tensor that requires grad is refused."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import torch

from . import check, declare_once, lib, ptr, require_hip, stream_ptr

SCORES, ARGMAX, NLL = 0, 1, 2


def _declare(l):
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    l.dinv_gmm_scores.argtypes = [vp, i32, i64, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, i32, vp, vp]
    l.dinv_gmm_epll_workspace_bytes.restype = sz
    l.dinv_gmm_epll_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    l.dinv_gmm_epll_step.argtypes = [vp, i64, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]
    l.dinv_gmm_posterior.argtypes = [vp, i64, vp, vp, vp, vp, i32, i32, vp, vp, vp]
    l.dinv_gmm_moments_workspace_bytes.restype = sz
    l.dinv_gmm_moments_workspace_bytes.argtypes = [i64, i32, i32, i32]
    l.dinv_gmm_moments.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]


def _l():
    return declare_once(lib(), _declare)


@dataclass
class Operands:
    """the device operands of the kernels: ``Wt`` [K dp, d] the stacked ``Q_k^T``, ``m`` [K dp] = ``Q_k^T mu_k``, ``lam`` [K dp]
    (dp = d rounded up to a multiple of 4, :func:`pad_rows`), ``logw`` [K]; ``lam_min`` the smallest eigenvalue as rounded to
    fp32 (``lam_min + r > 0`` is what every use needs)"""
    Wt: torch.Tensor
    m: torch.Tensor
    lam: torch.Tensor
    logw: torch.Tensor
    K: int
    d: int
    lam_min: float


def eigen_pack(cov: torch.Tensor, mu: torch.Tensor, weights: torch.Tensor):
    """(Wt [K d, d], m [K d], lam [K d], logw [K]) in fp64 on the host from the covariances [K, d, d], means [K, d] and weights
    [K]: ``eigh`` of the symmetrised covariance, eigenvalues ascending"""
    cov = cov.detach().to("cpu", torch.float64)
    K, d, d2 = cov.shape
    if d != d2 or tuple(mu.shape) != (K, d) or tuple(weights.shape) != (K,):
        raise ValueError(f"expected cov [K, d, d], mu [K, d] and weights [K], got {tuple(cov.shape)}, {tuple(mu.shape)}, "
                         f"{tuple(weights.shape)}")
    lam, Q = torch.linalg.eigh(0.5 * (cov + cov.transpose(1, 2)))
    Wt = Q.transpose(1, 2).contiguous()                                    # [K, d (eigenvector i), d]
    m = torch.bmm(Wt, mu.detach().to("cpu", torch.float64)[:, :, None])[:, :, 0]
    logw = torch.log(weights.detach().to("cpu", torch.float64))
    return Wt.reshape(K * d, d), m.reshape(K * d), lam.reshape(K * d), logw


def padded_dim(d: int) -> int:
    """rows per component in the kernels' operands: d rounded up to a multiple of 4 (csrc/patch_gmm.hpp, gmm_dp)"""
    return (d + 3) // 4 * 4


def pad_rows(Wt, m, lam, K, d):
    """[K d, ...] -> [K dp, ...]: the padding rows of a component hold Wt = 0, m = 0, lam = 1"""
    dp = padded_dim(d)
    if dp == d:
        return Wt, m, lam
    W2, m2, l2 = Wt.new_zeros(K, dp, d), m.new_zeros(K, dp), lam.new_ones(K, dp)
    W2[:, :d], m2[:, :d], l2[:, :d] = Wt.reshape(K, d, d), m.reshape(K, d), lam.reshape(K, d)
    return W2.reshape(K * dp, d), m2.reshape(-1), l2.reshape(-1)


def pack(cov, mu, weights, device, regularized: bool = True) -> Operands:
    """the operands of a model on ``device``.  ``regularized=False`` says that the model will be used with r = 0: a non-positive
    eigenvalue (after rounding to fp32) is then a ValueError here."""
    Wt, m, lam, logw = (t.float() for t in eigen_pack(cov, mu, weights))
    K, d = cov.shape[0], cov.shape[1]
    lam_min = float(lam.min())
    Wt, m, lam = pad_rows(Wt, m, lam, K, d)
    if not regularized and not lam_min > 0:
        raise ValueError(f"the covariances are not positive definite in fp32 (smallest eigenvalue {lam_min:.3g}): the unregularised "
                         "model needs lam > 0")
    return Operands(Wt.to(device), m.to(device), lam.to(device), logw.to(device), K, d, lam_min)


def _refuse_grad(*tensors):
    for t in tensors:
        if t is not None and t.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("the Gaussian-mixture kernels have no backward: gradients through GaussianMixtureModel / EPLL "
                                      "are not implemented (detach the input or run under torch.no_grad())")


def _input(x, what):
    if x.dtype != torch.float32:
        raise TypeError(f"the Gaussian-mixture kernels are fp32: {what} has dtype {x.dtype}; convert it with .float()")
    return x.contiguous()


def _reg(ops: Operands, r, B, device):
    """the device array [B] of fp32 regularisations (None: r = 0) after the check of lam + r > 0 on host values"""
    if r is None:
        if not ops.lam_min > 0:
            raise ValueError(f"smallest eigenvalue {ops.lam_min:.3g} with r = 0: lam + r must be positive")
        return None
    if not isinstance(r, torch.Tensor):
        r = torch.full((B,), float(r), dtype=torch.float32)
    if r.numel() != B:
        raise ValueError(f"expected {B} regularisation values, got {r.numel()}")
    if not r.is_cuda or r.device != device:
        r = r.detach().to("cpu", torch.float32).reshape(B)
        if not float(r.min()) + ops.lam_min > 0:
            raise ValueError(f"smallest eigenvalue {ops.lam_min:.3g} with r = {float(r.min()):.3g}: lam + r must be positive")
        return r.to(device)
    return r.detach().float().reshape(B).contiguous()       # already on the device: lam + r > 0 is the caller's contract


_OUT = {SCORES: torch.float32, ARGMAX: torch.int32, NLL: torch.float32}


def _scores(ops, src, image, n, C, H, W, p, patches, r, epilogue, with_weights):
    out = torch.empty((patches, ops.K) if epilogue == SCORES else (patches,), dtype=_OUT[epilogue], device=src.device)
    if patches == 0:
        return out
    check(_l().dinv_gmm_scores(ptr(src), image, n, C, H, W, p, ptr(ops.Wt), ptr(ops.m), ptr(ops.lam),
                               ptr(ops.logw if with_weights else None), ops.K, ops.d, ptr(r), epilogue, ptr(out),
                               stream_ptr(src.device)))
    return out


def scores_rows(ops: Operands, x: torch.Tensor, r=None, epilogue: int = SCORES, with_weights: bool = True) -> torch.Tensor:
    """rows ``x`` [N, d] under the model: SCORES -> fp32 [N, K], ARGMAX -> int32 [N], NLL -> fp32 [N]; ``r`` None or one value"""
    dev = require_hip(x, ops.Wt)
    _refuse_grad(x)
    if x.dim() != 2 or x.shape[1] != ops.d:
        raise ValueError(f"expected rows [N, {ops.d}], got shape {tuple(x.shape)}")
    x = _input(x, "the input")
    return _scores(ops, x, 0, x.shape[0], 0, 0, 0, 0, x.shape[0], _reg(ops, r, 1, dev), epilogue, with_weights)


def patch_grid(shape, p: int, d: int):
    B, C, H, W = shape
    if C * p * p != d:
        raise ValueError(f"patches of {C} x {p} x {p} = {C * p * p} entries, the model has dimension {d}")
    if H < p or W < p:
        raise ValueError(f"a {H} x {W} image holds no {p} x {p} patch")
    return B, C, H, W, H - p + 1, W - p + 1


def scores_image(ops: Operands, x: torch.Tensor, p: int, r=None, epilogue: int = SCORES, with_weights: bool = True) -> torch.Tensor:
    """every p x p patch of the images ``x`` [B, C, H, W], in the order (b, y0, x0), under the model; ``r`` None or [B]"""
    dev = require_hip(x, ops.Wt)
    _refuse_grad(x)
    if x.dim() != 4:
        raise ValueError(f"expected images [B, C, H, W], got shape {tuple(x.shape)}")
    B, C, H, W, PH, PW = patch_grid(x.shape, p, ops.d)
    x = _input(x, "the image")
    return _scores(ops, x, 1, B, C, H, W, p, B * PH * PW, _reg(ops, r, B, dev), epilogue, with_weights)


def epll_step(ops: Operands, x: torch.Tensor, p: int, r, a, cb=None, bias=None) -> torch.Tensor:
    """one half-quadratic step: ``a[b] x~ + cb[b] bias`` with ``x~`` the average of the patch estimates under the most likely
    component (module docstring of csrc/patch_gmm.hpp).  ``r`` [B] host or device, ``a`` / ``cb`` [B] device fp32."""
    dev = require_hip(x, ops.Wt, bias, a, cb)
    _refuse_grad(x, bias)
    if x.dim() != 4:
        raise ValueError(f"expected images [B, C, H, W], got shape {tuple(x.shape)}")
    B, C, H, W, PH, PW = patch_grid(x.shape, p, ops.d)
    x = _input(x, "the image")
    if bias is not None:
        if bias.shape != x.shape:
            raise ValueError(f"the bias has shape {tuple(bias.shape)}, the image {tuple(x.shape)}")
        bias = _input(bias, "the bias")
    out = torch.empty_like(x)
    if B == 0:
        return out
    for t, name in ((a, "a"), (cb, "cb")):
        if t is not None and (t.dtype != torch.float32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError(f"{name} must be {B} contiguous fp32 values on the device")
    r = _reg(ops, r, B, dev)
    l = _l()
    nbytes = l.dinv_gmm_epll_workspace_bytes(B, C, H, W, p)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(l.dinv_gmm_epll_step(ptr(x), B, C, H, W, p, ptr(ops.Wt), ptr(ops.m), ptr(ops.lam), ptr(ops.logw), ops.K, ops.d, ptr(r),
                               ptr(a), ptr(cb), ptr(bias), ptr(out), ptr(ws), nbytes, stream_ptr(x.device)))
    return out


# ---------------------------------------------------------------------- expectation-maximisation
def _rows(ops_d: int, x, dev_of):
    require_hip(x, dev_of)
    _refuse_grad(x)
    if x.dim() != 2 or x.shape[1] != ops_d:
        raise ValueError(f"expected rows [N, {ops_d}], got shape {tuple(x.shape)}")
    return _input(x, "the input")


def posterior_rows(ops: Operands, x: torch.Tensor):
    """the E-step on rows ``x`` [N, d] under the unregularised model, one launch: ``(beta [N, K], nll [N])`` with
    ``beta_nk = exp(score_nk - lse_n)`` and ``nll_n = -lse_n``, bitwise :func:`scores_rows` with ``NLL``"""
    x = _rows(ops.d, x, ops.Wt)
    _reg(ops, None, 1, x.device)
    N = x.shape[0]
    beta = torch.empty((N, ops.K), dtype=torch.float32, device=x.device)
    nll = torch.empty((N,), dtype=torch.float32, device=x.device)
    if N:
        check(_l().dinv_gmm_posterior(ptr(x), N, ptr(ops.Wt), ptr(ops.m), ptr(ops.lam), ptr(ops.logw), ops.K, ops.d, ptr(beta),
                                      ptr(nll), stream_ptr(x.device)))
    return beta, nll


@dataclass
class Moments:
    """the running fp64 device accumulators of one EM step: ``S0`` [K], ``S1`` [K, d], ``S2`` [K, d, d] (the sums of
    :func:`accumulate_moments`, centred at its ``c``) and ``obj`` [1], the sum of the negative log-likelihoods"""
    S0: torch.Tensor
    S1: torch.Tensor
    S2: torch.Tensor
    obj: torch.Tensor
    flat: torch.Tensor             # the one buffer the four are views of, so that a step downloads them in one copy

    @classmethod
    def of(cls, flat: torch.Tensor, K: int, d: int):
        S0, S1, S2, obj = flat.split([K, K * d, K * d * d, 1])
        return cls(S0, S1.view(K, d), S2.view(K, d, d), obj, flat)

    @classmethod
    def zeros(cls, K: int, d: int, device):
        return cls.of(torch.zeros(K + K * d + K * d * d + 1, dtype=torch.float64, device=device), K, d)

    def cpu(self):
        """the accumulators on the host, by one copy"""
        return Moments.of(self.flat.cpu(), *self.S1.shape)


def accumulate_moments(acc: Moments, x: torch.Tensor, beta: torch.Tensor, c: torch.Tensor, nll: torch.Tensor = None,
                       chunk_rows: int = 0) -> Moments:
    """adds the sums of one batch to ``acc``, two launches: ``S0_k += sum_n beta_nk``, ``S1_k += sum_n beta_nk (x_n - c_k)``,
    ``S2_k += sum_n beta_nk (x_n - c_k)(x_n - c_k)^T`` and - with ``nll`` - ``obj += sum_n nll_n``.  ``x`` [N, d], ``beta`` [N, K],
    ``c`` [K, d] fp32 on the device; ``chunk_rows`` 0 (automatic) or a multiple of 32 forces the rows per fp32 partial sum."""
    if acc.S1.dim() != 2:
        raise ValueError(f"the accumulator S1 is [K, d], got shape {tuple(acc.S1.shape)}")
    K, d = acc.S1.shape
    got = tuple(tuple(t.shape) for t in (acc.S0, acc.S2, acc.obj))
    if got != ((K,), (K, d, d), (1,)):
        raise ValueError(f"the accumulators are S0 [{K}], S1 [{K}, {d}], S2 [{K}, {d}, {d}] and obj [1], got S0, S2, obj of shapes {got}")
    x = _rows(d, x, acc.S0)
    require_hip(x, acc.S0, acc.S1, acc.S2, acc.obj, beta, c, nll)
    N = x.shape[0]
    if tuple(beta.shape) != (N, K) or tuple(c.shape) != (K, d) or (nll is not None and tuple(nll.shape) != (N,)):
        raise ValueError(f"expected beta [{N}, {K}], c [{K}, {d}] and nll [{N}], got {tuple(beta.shape)}, {tuple(c.shape)}"
                         + ("" if nll is None else f", {tuple(nll.shape)}"))
    beta, c = _input(beta, "beta"), _input(c, "c")
    nll = None if nll is None else _input(nll, "nll")
    for t in (acc.S0, acc.S1, acc.S2, acc.obj):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise TypeError("the accumulators are contiguous fp64 tensors (Moments.zeros)")
    if N == 0:
        return acc
    l = _l()
    nbytes = l.dinv_gmm_moments_workspace_bytes(N, K, d, chunk_rows)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    check(l.dinv_gmm_moments(ptr(x), ptr(beta), ptr(c), ptr(nll), N, K, d, chunk_rows, ptr(acc.S0), ptr(acc.S1), ptr(acc.S2),
                             ptr(acc.obj), ptr(ws), nbytes, stream_ptr(x.device)))
    return acc


def em_finalise(S0, S1, S2, c, n: int, cov_regularization: float):
    """the M-step in fp64 from the centred sums: ``(weights [K], mu [K, d], cov [K, d, d])``.  The raw moments are recovered,
    ``sum beta x = S1 + S0 c`` and ``sum beta x x^T = S2 + c S1^T + S1 c^T + S0 c c^T``, and the reference's formulas applied to them
    literally (deepinv/optim/utils.py:403-410 and 361-363): the mass clamped from below at 1e-5, ``mu = . / w``,
    ``cov = . / w - mu mu^T``, ``weights = w / n`` and ``+ cov_regularization I`` - so a clamped component follows the reference."""
    S0, S1, S2, c = (t.detach().to(torch.float64) for t in (S0, S1, S2, c))
    first = S1 + S0[:, None] * c
    cS1 = c[:, :, None] * S1[:, None, :]
    second = S2 + cS1 + cS1.transpose(1, 2) + S0[:, None, None] * c[:, :, None] * c[:, None, :]
    w = torch.maximum(S0, torch.tensor(1e-5).to(S0))                  # (an fp32 1e-5, as the reference builds it)
    mu = first / w[:, None]
    cov = second / w[:, None, None] - mu[:, :, None] * mu[:, None, :]
    cov = cov + cov_regularization * torch.eye(c.shape[1])[None].to(cov)        # (an identity of cov's dtype: not rounded)
    return w / n, mu, cov


def multiplicity(H: int, W: int, p: int) -> torch.Tensor:
    """[H, W] int64: how many p x p patches cover each pixel, the closed form of gmm_aggregate_kernel"""
    def axis(n):
        i = torch.arange(n)
        return torch.clamp(i, max=n - p) - torch.clamp(i - p + 1, min=0) + 1
    return axis(H)[:, None] * axis(W)[None, :]


LOG_2PI = math.log(2 * math.pi)
