"""Gaussian-mixture patch prior and Expected Patch Log-Likelihood reconstruction (reference deepinv/optim/utils.py:137-312
``GaussianMixtureModel`` with ``fit``, deepinv/optim/epll.py ``EPLL``) on the kernels of csrc/patch_gmm.hpp and
csrc/gmm_moments.hpp.

One change from the reference: a covariance is decomposed once, ``Sigma_k = Q_k diag(lam_k) Q_k^T`` (fp64 ``eigh`` on the host),
and the regularised model ``Sigma_k + r I`` of a half-quadratic step is the same operands with the runtime scalar ``r``: nothing is
inverted or rebuilt between the five betas, and the images of a batch may carry different ``sigma`` and ``beta``.  The parameter
names are the reference's, so its state dicts load with ``strict=True``; the inverse and log-determinant tensors are derived from
the eigendecomposition."""
from __future__ import annotations

import torch
import torch.nn as nn

from ..hip import gmm as G
from ..physics.forward import Denoising
from .linear import conjugate_gradient


def _per_image(v, B, name):
    """``v`` (float, list or tensor of 1 or B values) as B fp32 values on the host, as the reference's ``_handle_sigma`` lays a
    noise level out per image"""
    t = v.detach().to("cpu") if isinstance(v, torch.Tensor) else torch.as_tensor(v)
    t = t.to(torch.float32).reshape(-1)
    if t.numel() == 1:
        t = t.expand(B)
    if t.numel() != B:
        raise ValueError(f"{name} has {t.numel()} values for a batch of {B}")
    return t.contiguous()


class GaussianMixtureModel(nn.Module):
    r"""Gaussian mixture model: its component log-likelihoods, negative log-likelihood and classification on the fp32 matrix
    cores, and their estimation from data by expectation-maximisation (:meth:`fit`): per batch the responsibilities in one
    launch and the centred weighted moments of every component in two, the M-step formulas in fp64 on the host once per
    iteration.

    The kernels read a packed copy of the parameters that is rebuilt when they change.  Change them through ``set_cov``,
    ``set_weights``, ``load_state_dict`` or by rebinding ``.data`` (as the reference's ``fit`` does); after an in-place write through
    ``.data`` call :meth:`invalidate`, or the kernels keep scoring against the old model.

    :param int n_components: number of components
    :param int dimension: data dimension
    :param str device: device of the parameters
    """

    def __init__(self, n_components: int, dimension: int, device="cpu"):
        super().__init__()
        self._covariance_regularization = None
        self.n_components = n_components
        self.dimension = dimension
        eye = 0.1 * torch.eye(dimension, device=device)[None, :, :].tile(n_components, 1, 1)
        self._weights = nn.Parameter(torch.ones((n_components,), device=device), requires_grad=False)
        self.set_weights(self._weights)
        self.mu = nn.Parameter(torch.zeros((n_components, dimension), device=device), requires_grad=False)
        self._cov = nn.Parameter(eye.clone(), requires_grad=False)
        self._cov_inv = nn.Parameter(eye.clone(), requires_grad=False)
        self._cov_inv_reg = nn.Parameter(eye.clone(), requires_grad=False)
        self._cov_reg = nn.Parameter(eye.clone(), requires_grad=False)
        self._logdet_cov = nn.Parameter(self._weights.clone(), requires_grad=False)
        self._logdet_cov_reg = nn.Parameter(self._weights.clone(), requires_grad=False)
        self._eig = None          # (key, lam fp64 [K, d], Q fp64 [K, d, d]) of the current covariance
        self._ops = None          # (key, hip.gmm.Operands) of the current covariance, means and weights
        self._mu_host = None      # (key, the means on the host): fit keeps the copy it uploaded
        self.set_cov(self._cov)

    # ------------------------------------------------------------------ the eigendecomposition and what derives from it
    @staticmethod
    def _key(*tensors):
        return tuple((t.data_ptr(), t._version, t.device, tuple(t.shape)) for t in tensors)

    def _eigh(self):
        key = self._key(self._cov)
        if self._eig is None or self._eig[0] != key:
            cov = self._cov.detach().to("cpu", torch.float64)
            lam, Q = torch.linalg.eigh(0.5 * (cov + cov.transpose(1, 2)))
            self._eig = (key, lam, Q)
        return self._eig[1], self._eig[2]

    def _derive(self, r):
        """(inverse, log-determinant) of Sigma_k + r I in the parameters' dtype; a non-positive lam + r leaves NaN / inf, as
        ``logdet`` and ``inv`` of the reference would"""
        lam, Q = self._eigh()
        lr = lam + float(r)
        inv = torch.matmul(Q / lr[:, None, :], Q.transpose(1, 2))
        logdet = torch.where(lr > 0, torch.log(lr.clamp_min(1e-300)), torch.full_like(lr, float("nan"))).sum(1)
        return inv.to(self._cov), logdet.to(self._cov)

    def _reg32(self):
        """the regularisation as the reference applies it: multiplied into an fp32 identity, so rounded to fp32"""
        return float(torch.tensor(float(self._covariance_regularization), dtype=torch.float32))

    def invalidate(self):
        """Drops the cached eigendecomposition and kernel operands.  The caches notice ``set_cov`` / ``set_weights`` /
        ``load_state_dict``, a rebound ``.data`` and in-place operations on a parameter itself; they cannot notice an in-place
        write made through ``.data`` (``gmm.mu.data[0] = v``, ``gmm._cov.data.mul_(2)``), which bumps no version counter.  Call
        this after such a write."""
        self._eig = self._ops = self._mu_host = None

    def operands(self, regularized: bool) -> G.Operands:
        """the kernels' operands on the parameters' device, rebuilt when a parameter changed (see :meth:`invalidate` for the one
        kind of change that has to be announced)"""
        key = self._key(self._cov, self.mu, self._weights)
        if self._ops is None or self._ops[0] != key:
            self._ops = (key, G.pack(self._cov, self.mu, self._weights, self._cov.device, regularized=True))
        ops = self._ops[1]
        if not regularized and not ops.lam_min > 0:
            raise ValueError(f"the covariances are not positive definite in fp32 (smallest eigenvalue {ops.lam_min:.3g}): the "
                             "unregularised model needs lam > 0")
        return ops

    # ------------------------------------------------------------------ the reference's setters and getters
    def set_cov(self, cov: torch.Tensor):
        r"""Sets the covariances [n_components, dimension, dimension] and maintains their log-determinants and inverses."""
        self._cov.data = cov.detach().to(self._cov).clone()
        self._cov_inv.data, self._logdet_cov.data = self._derive(0.0)
        if self._covariance_regularization:
            self._set_reg_tensors()

    def _set_reg_tensors(self):
        r = self._reg32()
        eye = torch.eye(self.dimension, device=self._cov.device, dtype=self._cov.dtype)[None, :, :]
        self._cov_reg.data = self._cov.detach().clone() + r * eye
        self._cov_inv_reg.data, self._logdet_cov_reg.data = self._derive(r)

    def set_cov_reg(self, reg: float):
        r"""Sets the covariance regularisation ``Sigma_k + reg I`` used with ``cov_regularization=True``."""
        self._covariance_regularization = reg
        self._set_reg_tensors()

    def get_cov(self):
        return self._cov.clone()

    def get_cov_inv_reg(self):
        return self._cov_inv_reg.clone()

    def set_weights(self, weights: torch.Tensor):
        r"""Sets the weights, normalised to sum to one; they must be non-negative with a positive sum."""
        if torch.min(weights) < 0.0 or torch.sum(weights) <= 0.0:
            raise ValueError("Weights is not allowed to have negative elements, and requires at least one strictly positive value.")
        self._weights.data = (weights / torch.sum(weights)).detach().to(self._weights)

    def get_weights(self):
        return self._weights.clone()

    def load_state_dict(self, *args, **kwargs):
        r"""Loads the reference's state dict and re-derives the maintained tensors from the covariances."""
        out = super().load_state_dict(*args, **kwargs)
        self.set_cov(self._cov)
        self.set_weights(self._weights)
        return out

    # ------------------------------------------------------------------ expectation-maximisation
    def _batch(self, batch, rows: int = None):
        """a batch of the dataloader (its first ``rows`` rows) as fp32 rows [n, dimension] beside the parameters
        (``x.to(self.mu)``)"""
        x = batch[0] if isinstance(batch, (tuple, list)) else batch
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"fit: a batch is a tensor [n, {self.dimension}] or a tuple or list whose first element is one, got "
                            f"{type(x).__name__}")
        if x.dim() != 2 or x.shape[1] != self.dimension:
            raise ValueError(f"fit: a batch holds rows [n, {self.dimension}], got shape {tuple(x.shape)}")
        x = x.detach()[:rows].to(self.mu)
        if x.dtype != torch.float32:
            raise TypeError(f"fit: the kernels are fp32 and a batch takes the parameters' dtype, {x.dtype}: convert the model with "
                            ".float()")
        return x

    def _set_mu(self, mu_host):
        """rebinds the means to the upload of ``mu_host`` and keeps the host copy for the next M-step"""
        mu_host = mu_host.detach().to("cpu", self.mu.dtype).contiguous()
        self.mu.data = mu_host.to(self.mu.device)
        self.invalidate()
        self._mu_host = (self._key(self.mu), mu_host)

    def _EM_step(self, dataloader, verbose: bool = False, cov_regularization: float = 0.0):
        """one EM iteration: per batch three launches into the fp64 device accumulators, then one download and the M-step on
        the host; ``(weights, mu, cov + cov_regularization I, objective)`` in fp64 on the host.  ``verbose`` is accepted in the
        reference's position and prints nothing: ``fit`` reports per iteration."""
        ops = self.operands(False)
        c = self.mu.detach().float().contiguous()
        if self._mu_host is None or self._mu_host[0] != self._key(self.mu):      # means set by someone else: one small download
            self._mu_host = (self._key(self.mu), self.mu.detach().cpu())
        c_host = self._mu_host[1]
        acc = G.Moments.zeros(self.n_components, self.dimension, c.device)
        n = 0
        for batch in dataloader:
            x = self._batch(batch)
            n += x.shape[0]
            beta, nll = G.posterior_rows(ops, x)
            G.accumulate_moments(acc, x, beta, c, nll)
        if n == 0:
            raise ValueError("fit: the dataloader yielded no rows")
        host = acc.cpu()
        weights, mu, cov = G.em_finalise(host.S0, host.S1, host.S2, c_host, n, cov_regularization)
        return weights, mu, cov, float(host.obj) / n

    def fit(self, dataloader, max_iters: int = 100, stopping_criterion: float = None, data_init: bool = True,
            cov_regularization: float = 1e-5, verbose: bool = False):
        r"""Batched expectation-maximisation, the reference's ``fit`` (deepinv/optim/utils.py:314-412).

        :param dataloader: any iterable of batches ``[n, dimension]``, or of tuples or lists whose first element is one; it is
            iterated once per iteration, and batches are moved to the parameters' device
        :param int max_iters: maximum number of iterations
        :param float stopping_criterion: stop when the objective decreases by less than this; ``None``: ``max_iters`` iterations
        :param bool data_init: initialise the means with the first ``n_components`` rows (a shorter first batch is filled up
            with ``randn * std + mean`` of its rows); ``False`` starts from the current parameters
        :param float cov_regularization: added to the diagonal of every new covariance
        :param bool verbose: print the objective of every iteration
        """
        if dataloader is None:
            raise NotImplementedError("GaussianMixtureModel.fit needs an iterable of [n, d] batches; fitting from nothing is not "
                                      "implemented")
        if data_init:
            first = self._batch(next(iter(dataloader)), self.n_components)
        G.require_hip(self.mu)
        if data_init:
            mu, n0 = self.mu.detach().clone(), first.shape[0]
            mu[:n0] = first
            if n0 < self.n_components:
                mu[n0:] = torch.randn_like(mu[n0:]) * torch.std(first, 0, keepdim=True) + torch.mean(first, 0, keepdim=True)
            self._set_mu(mu)
        objective = 1e100
        for step in range(max_iters):
            weights, mu, cov, objective_new = self._EM_step(dataloader, verbose, cov_regularization)
            self.set_weights(weights)
            self._set_mu(mu)
            self.set_cov(cov)
            if verbose:
                print(f"Step {step + 1}, Objective {objective_new:.4f}")
            if stopping_criterion:
                if objective - objective_new < stopping_criterion:
                    return
            objective = objective_new

    # ------------------------------------------------------------------ evaluation
    def _r(self, cov_regularization):
        if not cov_regularization:
            return None
        if self._covariance_regularization is None:
            raise ValueError("cov_regularization=True needs set_cov_reg(reg) first")
        return self._reg32()

    def component_log_likelihoods(self, x: torch.Tensor, cov_regularization: bool = False):
        r"""log-likelihood of every row of ``x`` [N, dimension] under every component (without the weights): [N, n_components]"""
        r = self._r(cov_regularization)
        return G.scores_rows(self.operands(r is not None), x, r, G.SCORES, with_weights=False)

    def forward(self, x: torch.Tensor):
        r"""negative log-likelihood of every row of ``x`` [N, dimension]"""
        return G.scores_rows(self.operands(False), x, None, G.NLL)

    def classify(self, x: torch.Tensor, cov_regularization: bool = False):
        """index of the most likely component of every row of ``x`` (the lowest index on a tie): int64 [N]"""
        r = self._r(cov_regularization)
        return G.scores_rows(self.operands(r is not None), x, r, G.ARGMAX).long()


_DOWNLOADS = ("download", "GMM_BSDS_gray", "GMM_BSDS_color", "GMM_lodopab_small")


class EPLL(nn.Module):
    r"""Expected Patch Log-Likelihood reconstruction (Zoran and Weiss) by approximated half-quadratic splitting, as the
    reference's ``deepinv.optim.EPLL``, vectorised over the batch: every image carries its own ``sigma`` and ``beta``.

    :param GaussianMixtureModel GMM: the patch prior; ``None`` creates one with ``n_components`` components of dimension
        ``patch_size**2 * channels``.
    :param str, None pretrained: ``None``, or the path of a ``.pt`` state dict.  This package fetches nothing from the network:
        the reference's download names raise.
    """

    def __init__(self, GMM: GaussianMixtureModel = None, n_components: int = 200, pretrained: str | None = None,
                 patch_size: int = 6, channels: int = 1, device="cpu"):
        super().__init__()
        self.GMM = GaussianMixtureModel(n_components, patch_size ** 2 * channels, device=device) if GMM is None else GMM
        self.patch_size = patch_size
        if pretrained:
            if not pretrained.endswith(".pt"):
                known = pretrained in _DOWNLOADS or pretrained.startswith("GMM_lodopab_small")
                raise ValueError(f"pretrained={pretrained!r}: " + ("deepinv_amd has no network fetch of pretrained weights; "
                                 "pass the path of a .pt state dict" if known else "expected None or the path of a .pt file"))
            self.load_state_dict(torch.load(pretrained, map_location="cpu"))

    def forward(self, y, physics, sigma=None, x_init=None, betas=None, batch_size: int = -1):
        r"""``batch_size`` is accepted and ignored: by its definition it has no effect on the output, and no patch matrix exists
        here whose memory it would bound."""
        x = physics.A_adjoint(y) if x_init is None else x_init
        if sigma is None:
            if hasattr(physics.noise_model, "sigma"):
                sigma = physics.noise_model.sigma
            else:
                raise ValueError("Noise level sigma has to be provided if not present in the physics model.")
        B = y.shape[0]
        sigma = _per_image(sigma, B, "sigma")
        if betas is None:
            betas = [c / sigma ** 2 for c in (1.0, 4.0, 8.0, 16.0, 32.0)]
        else:
            betas = [_per_image(beta, B, "beta") for beta in betas]
        Aty = physics.A_adjoint(y)
        for beta in betas:
            x = self._reconstruction_step(Aty, x, sigma ** 2, beta, physics)
        return x

    def negative_log_likelihood(self, x: torch.Tensor) -> torch.Tensor:
        r"""negative log-likelihood of patches ``x`` [B, patches, ...] under the mixture: [B, patches]"""
        B, n_patches = x.shape[0:2]
        return self.GMM(x.reshape(B * n_patches, -1)).view(B, n_patches)

    def _reconstruction_step(self, Aty, x, sigma_sq, beta, physics):
        """one half-quadratic step with per-image fp32 host vectors ``sigma_sq`` and ``beta`` (epll.py:167-232)"""
        ops = self.GMM.operands(True)
        r = 1.0 / beta                                        # fp32, as set_cov_reg(1.0 / beta) rounds it
        a = (beta * sigma_sq).double()                        # beta sigma^2 of rhs = A^T y + beta sigma^2 x~
        closed = isinstance(physics, Denoising) and _is_identity(physics)
        if closed:
            # A = I: (1 + beta sigma^2) x = rhs, folded into the two scalars of the aggregation's epilogue
            scal = torch.stack([a / (1.0 + a), 1.0 / (1.0 + a)]).float().to(x.device)
            return G.epll_step(ops, x, self.patch_size, r, scal[0], scal[1], Aty)
        a_dev = a.float().to(x.device)
        rhs = G.epll_step(ops, x, self.patch_size, r, a_dev, None, Aty)
        scale = a_dev.view(-1, *([1] * (x.dim() - 1)))
        return conjugate_gradient(lambda im: physics.A_adjoint(physics.A(im)) + scale * im, rhs, max_iter=1e2, tol=1e-5)


def _is_identity(physics):
    """a Denoising physics whose operator is the identity: the default mask 1 of the decomposable form"""
    mask = getattr(physics, "mask", None)
    return isinstance(mask, torch.Tensor) and mask.numel() == 1 and not mask.is_complex() and float(mask) == 1.0
