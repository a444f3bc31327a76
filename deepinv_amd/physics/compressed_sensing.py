"""Compressed sensing with a dense iid Gaussian matrix (reference deepinv/physics/compressed_sensing.py).  ``A``, ``A_adjoint``
and ``A_dagger`` are one launch each of csrc/dense.hip (hip/dense.py): the same contraction ``out[i, r] = sum_k in[i, k] M[r, k]``
with ``M`` the buffers ``_A``, ``_A_adjoint`` and ``_A_dagger`` in turn.  ``_A_adjoint`` is a transposed view of ``_A``, as in the
reference, and the kernel reads it in place: the device holds one copy of the matrix.

:class:`_GaussianMatrix` holds everything but the scalar type: the fp32 operator here and the complex64 one of phase retrieval
(physics/phase_retrieval.py) are what it is subclassed to."""
from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from ..hip import dense as hden
from .forward import LinearPhysics
from .functional import dst1  # noqa: F401  (the reference exports dst1 from this module too)


class _GaussianMatrix(LinearPhysics):
    """A dense iid Gaussian matrix as a linear operator: the buffers ``_A``, ``_A_dagger``, ``_A_adjoint`` and
    ``initial_random_state`` of the reference's ``CompressedSensing``, with ``_A_adjoint`` kept a view of ``_A``, and the
    ``channelwise`` reshapes around one product.  A subclass sets the scalar type:

    * ``_dtype``, the one dtype it runs in, and ``_refusal``, what it says to any other;
    * ``_pinv_dtype``, in which the pseudo-inverse is computed once at construction, on the host;
    * ``_product(x, M, ...)``, the kernel ``out[i, r] = sum_k x[i, k] M[r, k]``."""

    _dtype = _pinv_dtype = _refusal = _product = None

    def __init__(self, m: int, img_size, channelwise: bool = False, dtype: torch.dtype = None, device="cpu",
                 rng: torch.Generator = None, **kwargs):
        super().__init__(device=device, **kwargs)
        if dtype != self._dtype:
            raise NotImplementedError(self._refusal.format(dtype=dtype))
        self.name = f"CS_m{m}"
        self.img_size = img_size
        self.channelwise = channelwise
        self.dtype = dtype
        if rng is None:
            self.rng = torch.Generator(device=device)
        else:
            if torch.device(rng.device).type != torch.device(device).type or (
                    torch.device(device).index is not None and rng.device.index is not None
                    and rng.device.index != torch.device(device).index):
                raise ValueError("The random generator is not on the same device as the physics. Got random generator on "
                                 f"{rng.device} and the physics on {device}.")
            self.rng = rng
        self.register_buffer("initial_random_state", self.rng.get_state())
        n = int(np.prod(img_size[1:])) if channelwise else int(np.prod(img_size))
        _A = torch.randn((m, n), device=device, dtype=dtype, generator=self.rng) / np.sqrt(m)
        # once, on the host: no device solver library is needed
        _A_dagger = torch.linalg.pinv(_A.detach().cpu().to(self._pinv_dtype)).to(dtype).to(device)
        self.register_buffer("_A", _A)
        self.register_buffer("_A_dagger", _A_dagger)
        self._tie_adjoint()
        # a complex module is moved only: Module.to casts real buffers alone
        self.to(device=device) if dtype.is_complex else self.to(device=device, dtype=dtype)

    def _tie_adjoint(self):
        # _A_adjoint stays a view of _A, as in the reference: the kernel reads it in place and the device holds one copy of the
        # matrix.  A move, a cast or a load of the module handles every buffer on its own and would part the two.
        if "_A" in self._buffers:
            self.register_buffer("_A_adjoint", self._buffers["_A"].conj().T)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self._tie_adjoint()
        return self

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # the state of a generator of another device type has another size (a state dict written on the CPU, loaded into an
        # operator on the GPU): take it as it is instead of failing on the shape
        key = prefix + "initial_random_state"
        if key in state_dict and state_dict[key].shape != self.initial_random_state.shape:
            self.initial_random_state = state_dict[key].clone().to(self.initial_random_state.device)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._tie_adjoint()

    def _rows(self, x: Tensor):
        """``x`` as the rows that the matrix multiplies, and the function that puts the product in the shape of the measurements"""
        N, C = x.shape[:2]
        if self.channelwise:
            return x.reshape(N * C, -1), lambda y: y.view(N, C, -1)
        return x.reshape(N, -1), lambda y: y

    def A(self, x: Tensor, **kwargs) -> Tensor:
        x, shaped = self._rows(x)
        return shaped(type(self)._product(x, self._A))

    def _back(self, y, M):
        y = y.type(self.dtype)
        N = y.shape[0]
        C, H, W = self.img_size[0], self.img_size[1], self.img_size[2]
        if self.channelwise:
            y = y.reshape(N * C, -1)
        return type(self)._product(y, M).reshape(N, C, H, W)

    def A_adjoint(self, y: Tensor, **kwargs) -> Tensor:
        return self._back(y, self._A_adjoint)

    def A_dagger(self, y: Tensor, **kwargs) -> Tensor:
        return self._back(y, self._A_dagger)


class CompressedSensing(_GaussianMatrix):
    r"""
    Random iid Gaussian sampling matrix :math:`A_{i,j} \sim \mathcal{N}(0, \frac{1}{m})` of :math:`m \times n`, ``n`` the number
    of elements of the signal (of one channel when ``channelwise``).  Same signature, buffers (``_A``, ``_A_dagger``,
    ``_A_adjoint``, ``initial_random_state``) and state-dict keys as the reference, so ``load_state_dict`` of a reference state
    dict works.  The cost is :math:`O(mn)`: above 32 x 32 use :class:`deepinv_amd.physics.StructuredRandom`.

    The pseudo-inverse is computed once at construction, on the host in float64, and rounded to fp32.
    ``dtype`` other than ``torch.float`` raises ``NotImplementedError`` (``cfloat`` belongs to phase retrieval).

    :param int m: number of measurements.
    :param tuple img_size: shape (C, H, W) of inputs.
    :param bool channelwise: channels are processed independently with the same matrix.
    :param torch.dtype dtype: ``torch.float``.
    :param str device: device of the matrix.
    :param torch.Generator rng: generator of the matrix, on ``device``.
    """

    _dtype, _pinv_dtype = torch.float, torch.float64
    _refusal = ("CompressedSensing runs in torch.float on the dense fp32 kernel, got dtype {dtype} "
                "(complex matrices belong to phase retrieval)")
    _product = staticmethod(hden.apply)

    def __init__(self, m: int, img_size, channelwise: bool = False, dtype: torch.dtype = torch.float, device="cpu",
                 rng: torch.Generator = None, **kwargs):
        super().__init__(m, img_size, channelwise, dtype, device, rng, **kwargs)
