"""Single-pixel camera: the subsampled 2-D Walsh-Hadamard operator ``A = diag(mask) H2`` (reference
deepinv/physics/singlepixel.py).  ``H2`` and every operator built on it are one call each into csrc/hadamard.hip
(hip/hadamard.py); the mask builders below run once per operator on the host and reproduce the reference's masks element for
element.

The orderings, from their definitions: natural (Sylvester) row ``r`` of ``H_n`` has ``popcount``-independent sequency; the
row with ``k`` sign changes is ``r = bitreverse(gray(k))`` with ``gray(k) = k ^ (k >> 1)``.  ``sequency`` keeps the first ``m``
entries of that order over the column-major flattening of the plane, ``cake_cutting`` walks the same order through a
boustrophedon of the ``sqrt(n) x sqrt(n)`` product table, ``zig_zag`` and ``xy`` rank the 2-D sequency pairs along
anti-diagonals and along ``xy + (x^2 + y^2) / 4`` and map them back to natural order.
"""
from __future__ import annotations

import math
import warnings

import numpy as np
import torch
from torch import Tensor

from ..hip import hadamard as hh
from .forward import DecomposablePhysics


# --------------------------------------------------------------------------- transforms
def hadamard_1d(u: Tensor, normalize: bool = True) -> Tensor:
    r""":math:`H_n u` along the last axis (natural order), divided by :math:`\sqrt n` when ``normalize``
    (singlepixel.py:9-27)."""
    return hh.fwht(u, last_axis=True, normalize=normalize)


def hadamard_2d(x: Tensor) -> Tensor:
    """orthonormal 2-D transform of the last two axes (singlepixel.py:30-43) as one launch for planes up to 128 x 128"""
    return hh.fwht(x)


def _index(order, device):
    return torch.as_tensor(np.asarray(order), dtype=torch.long, device=device)


def hadamard_shift(x: Tensor, dim: int) -> Tensor:
    """natural -> sequency order along ``dim`` (singlepixel.py:46-61)"""
    return x.index_select(dim, _index(sequency_order(x.shape[dim]), x.device))


def hadamard_ishift(x: Tensor, dim: int) -> Tensor:
    """sequency -> natural order along ``dim`` (singlepixel.py:64-80)"""
    return x.index_select(dim, _index(np.argsort(sequency_order(x.shape[dim])), x.device))


def hadamard_2d_shift(x: Tensor) -> Tensor:
    return hadamard_shift(hadamard_shift(x, -2), -1)


def hadamard_2d_ishift(x: Tensor) -> Tensor:
    return hadamard_ishift(hadamard_ishift(x, -1), -2)


# --------------------------------------------------------------------------- Gray code and sequency order
def gray_code(n: int) -> np.ndarray:
    """the reflected Gray codes of 0 .. max(n, 2) - 1 as rows of bits, most significant first (singlepixel.py:442-459)"""
    count = max(int(n), 2)
    nbits = max((count - 1).bit_length(), 1)
    count = 1 << nbits
    k = np.arange(count)
    g = k ^ (k >> 1)
    return ((g[:, None] >> np.arange(nbits - 1, -1, -1)[None, :]) & 1).astype(np.float64)


def gray_decode(n: int) -> int:
    """the integer whose Gray code is ``n``: the prefix XOR of its bits (singlepixel.py:462-476)"""
    shift = n >> 1
    while shift:
        n ^= shift
        shift >>= 1
    return n


def reverse(n: int, numbits: int) -> int:
    """``n`` with its ``numbits`` low bits in reverse order (singlepixel.py:479-492)"""
    out = 0
    for i in range(numbits):
        out |= ((n >> i) & 1) << (numbits - 1 - i)
    return out


def get_permutation_list(n: int, device="cpu") -> Tensor:
    """bit reversal of the Gray-decoded index (singlepixel.py:495-513)"""
    nbits = int(math.log2(n))
    return torch.tensor([reverse(gray_decode(k), nbits) for k in range(n)], dtype=torch.long, device=device)


def sequency_order(n: int) -> np.ndarray:
    """natural-order row index of the Walsh function with ``k`` sign changes, ``k = 0 .. n - 1``: the bit reversal of the Gray
    code of ``k`` (singlepixel.py:516-528)"""
    bits = gray_code(n)
    weights = 1 << np.arange(bits.shape[1])        # column 0 is the most significant Gray bit: reversed, it weighs 1
    return (bits.astype(np.int64) @ weights).astype(np.int32)


# --------------------------------------------------------------------------- masks
def _column_major(H: int, W: int, flat):
    """(row, column) of entries of the column-major flattening of an H x W plane"""
    flat = np.asarray(flat)
    return flat % H, flat // H


def _select(img_size, flat) -> Tensor:
    _, H, W = img_size
    i, j = _column_major(H, W, flat)
    mask = torch.zeros((1, *img_size))
    mask[:, :, i, j] = 1.0
    return mask


def sequency_mask(img_size, m: int) -> Tensor:
    """the first ``m`` rows of the ``H W`` sequency order, over the column-major flattening (singlepixel.py:115-138)"""
    _, H, W = img_size
    return _select(img_size, sequency_order(H * W)[:m])


def cake_cutting_seq(i: int, p: int) -> list:
    """row ``i`` of the product table ``i k``, ``k = 1 .. p``: ascending for odd ``i``, descending for even
    (singlepixel.py:141-161)"""
    row = [i * k for k in range(1, p + 1)]
    return row if i % 2 == 1 else row[::-1]


def cake_cutting_order(n: int) -> np.ndarray:
    """(singlepixel.py:164-177)"""
    p = int(np.sqrt(n))
    seq = [v for i in range(1, p + 1) for v in cake_cutting_seq(i, p)]
    return np.argsort(seq)


def cake_cutting_mask(img_size, m: int) -> Tensor:
    """(singlepixel.py:180-210)"""
    _, H, W = img_size
    if H != W:
        warnings.warn("Image height and width must be equal for cake cutting mask.")
    n = H * W
    return _select(img_size, sequency_order(n)[cake_cutting_order(n)][:m])


def diagonal_index_matrix(H: int, W: int) -> Tensor:
    """rank of every entry of an H x W grid along its anti-diagonals, each walked from the bottom up (singlepixel.py:213-236)"""
    I, J = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    order = np.lexsort(((-I).ravel(), (I + J).ravel()))
    rank = np.empty(H * W, dtype=np.int64)
    rank[order] = np.arange(H * W)
    return torch.from_numpy(rank).view(H, W)


def _from_sequency(keep: Tensor, channels: int) -> Tensor:
    """a boolean [H, W] selection of 2-D sequency pairs -> the [1, C, H, W] float mask in natural order"""
    return hadamard_2d_ishift(keep.float().unsqueeze(0).repeat(1, channels, 1, 1))


def zig_zag_mask(img_size, m: int) -> Tensor:
    """(singlepixel.py:239-258)"""
    C, H, W = img_size
    return _from_sequency(diagonal_index_matrix(H, W) < m, C)


def xy_mask(img_size, m: int) -> Tensor:
    """(singlepixel.py:261-289); the fp32 key and its unstable sort decide the ties between (x, y) and (y, x), so they are the
    reference's"""
    C, H, W = img_size
    X, Y = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    key = X * Y + (X ** 2 + Y ** 2) / 4
    key /= key.max()
    order = torch.argsort(key.view(-1))
    rank = torch.empty(H * W, dtype=torch.long)
    rank[order] = torch.arange(1, H * W + 1)
    return _from_sequency(rank.view(H, W) <= m, C)


_MASKS = {"sequency": sequency_mask, "cake_cutting": cake_cutting_mask, "zig_zag": zig_zag_mask, "xy": xy_mask}


class SinglePixelCamera(DecomposablePhysics):
    r"""Single-pixel camera with ``fast=True``: :math:`A = \mathrm{diag}(mask)\,H_2`, the first ``m`` modes of the 2-D
    Walsh-Hadamard transform in the chosen ``ordering`` (singlepixel.py:292-439).  ``U`` is the identity and
    ``V = V^\top = H_2``; every operator is one fused library call (hip/hadamard.py).

    ``fast=False``, the dense iid :math:`\pm 1/\sqrt m` matrix through an SVD, is not covered: it is :math:`O(mn)` per call
    (the reference advises against it above 32 x 32) and would need a GEMM library this package does not have.
    """

    def __init__(self, m: int, img_size, fast: bool = True, ordering: str = "sequency", device="cpu",
                 dtype: torch.dtype = torch.float32, rng: torch.Generator = None, **kwargs):
        super().__init__(device=device, **kwargs)
        self.name = f"spcamera_m{m}"
        self.img_size = img_size
        self.fast = fast
        if rng is None:
            self.rng = torch.Generator(device=device)
        else:
            if rng.device != torch.device(device):
                raise ValueError("The random generator is not on the same device as the Physics Generator. Got random "
                                 f"generator on {rng.device} and the Physics Generator on {device}.")
            self.rng = rng
        self.register_buffer("initial_random_state", self.rng.get_state())
        if not fast:
            raise NotImplementedError(
                "SinglePixelCamera(fast=False) is the dense iid binary matrix through an SVD: O(mn) per call, which the "
                "reference itself advises against above 32 x 32, and it needs a GEMM library deepinv_amd does not have. "
                "Use fast=True (the subsampled Hadamard transform on the HIP kernels).")
        _, H, W = img_size
        if H != 1 << int(math.log2(H)):
            raise ValueError("image height must be a power of 2")
        if W != 1 << int(math.log2(W)):
            raise ValueError("image width must be a power of 2")
        if ordering not in _MASKS:
            raise ValueError(f"Unknown ordering {ordering}. Available options are: `sequency`, `cake_cutting`, `zig_zag`, `xy`.")
        self.register_buffer("mask", _MASKS[ordering](img_size, m).to(device))
        self.to(device=device, dtype=dtype)

    # The fused calls treat the mask as a constant of the operator.  A mask that records a gradient takes the composed
    # mask / V / V_adjoint expressions of the base class, whose arithmetic autograd follows.
    def _mask_needs_grad(self):
        return torch.is_grad_enabled() and isinstance(self.mask, Tensor) and self.mask.requires_grad

    def A(self, x, mask=None, **kwargs):
        self.update_parameters(mask=mask, **kwargs)
        return DecomposablePhysics.A(self, x) if self._mask_needs_grad() else hh.forward(x, self.mask)

    def A_adjoint(self, y, mask=None, **kwargs):
        self.update_parameters(mask=mask, **kwargs)
        return DecomposablePhysics.A_adjoint(self, y) if self._mask_needs_grad() else hh.adjoint(y, self.mask)

    def A_adjoint_A(self, x, mask=None, **kwargs):
        self.update_parameters(mask=mask, **kwargs)
        return DecomposablePhysics.A_adjoint_A(self, x) if self._mask_needs_grad() else hh.adjoint_forward(x, self.mask)

    def A_A_adjoint(self, y, mask=None, **kwargs):
        self.update_parameters(mask=mask, **kwargs)
        return DecomposablePhysics.A_A_adjoint(self, y) if self._mask_needs_grad() else hh.forward_adjoint(y, self.mask)

    def prox_l2(self, z, y, gamma, **kwargs):
        r""":math:`H_2\big((mask\,y + H_2 z/\gamma) / (mask^2 + 1/\gamma)\big)`: the reference's
        :math:`V(V^\top(V(mask\,y) + z/\gamma)/\dots)` with :math:`V^\top V = I` taken out (forward.py:1212-1234).

        A Tensor ``gamma`` (the trainable ``stepsize`` of an unfolded HQS, a per-sample vector) takes the composed expression of
        the base class over the ``V`` / ``V_adjoint`` kernels, so its gradient flows and no host synchronisation reads it.
        As in the reference, ``prox_l2`` takes no ``mask=`` keyword: it uses the operator's current mask."""
        if self._mask_needs_grad() and not isinstance(gamma, Tensor):
            gamma = torch.tensor(float(gamma), device=self.mask.device)      # the base class's tensor-arithmetic branch
        if isinstance(gamma, Tensor):
            return DecomposablePhysics.prox_l2(self, z, y, gamma, **kwargs)
        return hh.prox_l2(z, y, self.mask, gamma)

    def A_dagger(self, y, mask=None, **kwargs):
        self.update_parameters(mask=mask, **kwargs)
        if self._mask_needs_grad():
            keep = self.mask > 1e-5       # the reciprocal of a kept entry only: 1 / 0 in the dropped branch would make the gradient NaN
            inv = torch.where(keep, torch.where(keep, self.mask, torch.ones_like(self.mask)).reciprocal(), torch.zeros_like(self.mask))
            return self.V(y * inv)
        return hh.dagger(y, self.mask)

    def V_adjoint(self, x):
        return hadamard_2d(x)

    def V(self, y):
        return hadamard_2d(y)

    def U_adjoint(self, x):
        return x

    def U(self, x):
        return x
