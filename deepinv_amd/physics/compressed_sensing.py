"""Compressed sensing with a dense iid Gaussian matrix (reference deepinv/physics/compressed_sensing.py).  ``A``, ``A_adjoint``
and ``A_dagger`` are one launch each of csrc/dense.hip (hip/dense.py): the same contraction ``out[i, r] = sum_k in[i, k] M[r, k]``
with ``M`` the buffers ``_A``, ``_A_adjoint`` and ``_A_dagger`` in turn.  ``_A_adjoint`` is a transposed view of ``_A``, as in the
reference, and the kernel reads it in place: the device holds one copy of the matrix."""
from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from ..hip import dense as hden
from .forward import LinearPhysics
from .functional import dst1  # noqa: F401  (the reference exports dst1 from this module too)


class CompressedSensing(LinearPhysics):
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

    def __init__(self, m: int, img_size, channelwise: bool = False, dtype: torch.dtype = torch.float, device="cpu",
                 rng: torch.Generator = None, **kwargs):
        super().__init__(device=device, **kwargs)
        if dtype != torch.float:
            raise NotImplementedError(f"CompressedSensing runs in torch.float on the dense fp32 kernel, got dtype {dtype} "
                                      "(complex matrices belong to phase retrieval)")
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
        _A_dagger = torch.linalg.pinv(_A.detach().cpu().double()).to(dtype).to(device)
        self.register_buffer("_A", _A)
        self.register_buffer("_A_dagger", _A_dagger)
        self.register_buffer("_A_adjoint", self._A.conj().T)
        self.to(device=device, dtype=dtype)

    def _apply(self, fn, *args, **kwargs):
        # a move or cast of the module handles every buffer on its own: tie _A_adjoint to _A again, so that it stays a view as
        # in the reference and the device holds one copy of the matrix
        super()._apply(fn, *args, **kwargs)
        if "_A" in self._buffers and "_A_adjoint" in self._buffers:
            self._buffers["_A_adjoint"] = self._buffers["_A"].conj().T
        return self

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # the state of a generator of another device type has another size (a state dict written on the CPU, loaded into an
        # operator on the GPU): take it as it is instead of failing on the shape
        key = prefix + "initial_random_state"
        if key in state_dict and state_dict[key].shape != self.initial_random_state.shape:
            self.initial_random_state = state_dict[key].clone().to(self.initial_random_state.device)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def A(self, x: Tensor, **kwargs) -> Tensor:
        N, C = x.shape[:2]
        x = x.reshape(N * C, -1) if self.channelwise else x.reshape(N, -1)
        y = hden.apply(x, self._A)
        return y.view(N, C, -1) if self.channelwise else y

    def _back(self, y, M):
        y = y.type(self.dtype)
        N = y.shape[0]
        C, H, W = self.img_size[0], self.img_size[1], self.img_size[2]
        if self.channelwise:
            y = y.reshape(N * C, -1)
        return hden.apply(y, M).reshape(N, C, H, W)

    def A_adjoint(self, y: Tensor, **kwargs) -> Tensor:
        return self._back(y, self._A_adjoint)

    def A_dagger(self, y: Tensor, **kwargs) -> Tensor:
        return self._back(y, self._A_dagger)
