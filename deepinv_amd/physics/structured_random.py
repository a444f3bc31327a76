"""Structured random operator ``A = prod_i (F D_i)`` with ``F`` the orthonormal DST-I of the last axis and ``D_i`` real diagonals
(reference deepinv/physics/structured_random.py).  With the default transform the whole of ``A`` or ``A_adjoint`` - pad, every
(diagonal, transform) layer, trim - is ONE launch of csrc/dst.hip for any number of layers: a row is loaded once, stays in LDS
through all layers and is stored once."""
from __future__ import annotations

import math

import torch
from torch import Tensor

from ..hip import dst as hd
from .forward import LinearPhysics
from .functional import dst1


def compare(img_size: tuple, output_size: tuple) -> str:
    """the sampling mode of (C, H, W) -> (C, H, W) shapes: ``equisampling``, ``oversampling`` or ``undersampling``
    (structured_random.py:10-28)"""
    if img_size[1] == output_size[1] and img_size[2] == output_size[2]:
        return "equisampling"
    elif img_size[1] <= output_size[1] and img_size[2] <= output_size[2]:
        return "oversampling"
    elif img_size[1] >= output_size[1] and img_size[2] >= output_size[2]:
        return "undersampling"
    raise ValueError("Does not support different sampling schemes on height and width.")


def _changes(img_size, output_size):
    dh, dw = abs(img_size[1] - output_size[1]), abs(img_size[2] - output_size[2])
    return math.ceil(dh / 2), math.floor(dh / 2), math.ceil(dw / 2), math.floor(dw / 2)


def padding(tensor: Tensor, img_size: tuple, output_size: tuple) -> Tensor:
    """centred zero pad of the last two axes by the difference of the two shapes: ``ceil`` of half of it on the top / left,
    ``floor`` on the bottom / right (structured_random.py:31-52)"""
    top, bottom, left, right = _changes(img_size, output_size)
    return torch.nn.functional.pad(tensor, (left, right, top, bottom), mode="constant", value=0)


def trimming(tensor: Tensor, img_size: tuple, output_size: tuple) -> Tensor:
    """the inverse selection of :func:`padding` (structured_random.py:55-79)"""
    top, bottom, left, right = _changes(img_size, output_size)
    tensor = tensor[..., top:tensor.shape[-2] - bottom, :]
    return tensor[..., left:tensor.shape[-1] - right]


def generate_diagonal(shape: tuple, mode: str, dtype=torch.float, device="cpu", generator: torch.Generator | None = None):
    """a random diagonal (structured_random.py:82-105).  ``rademacher`` is the reference's own expression,
    ``where(rand(shape) > 0.5, -1, 1)`` drawn on ``device``; ``uniform_phase`` is complex and belongs to phase retrieval."""
    if generator is None:
        generator = torch.Generator(device)
    if mode == "uniform_phase":
        raise NotImplementedError("uniform_phase diagonals are complex (phase retrieval); deepinv_amd's StructuredRandom is real")
    if mode != "rademacher":
        raise ValueError(f"Unsupported mode: {mode}")
    diag = torch.where(torch.rand(shape, device=device, generator=generator) > 0.5, -1.0, 1.0)
    return diag.to(device)


class StructuredRandom(LinearPhysics):
    r"""
    :math:`A(x) = \prod_{i=1}^N (F D_i) x` with :math:`F` a structured transform of the last axis and :math:`D_i` diagonal
    matrices; ``n_layers = N + 0.5`` applies one more :math:`F` first.  Same signature as the reference.

    With a ``(C, H, W)`` image, oversampling zero-pads and undersampling crops, centred; with any other ``img_size`` there is
    no pad or trim and any leading dimensions are allowed.

    Differences from the reference, both at construction rather than at the first call:

    * the diagonals must have the working size, the larger of ``img_size`` and ``output_size``, and a mismatch raises
      ``ValueError`` here; the reference fails later with a broadcast error (with default diagonals its oversampling mode always
      does, so oversampling needs ``diagonals=`` of the output size there and here);
    * complex diagonals raise ``NotImplementedError``.

    The default transform takes the fused kernel: one launch per ``A`` / ``A_adjoint`` for any ``n_layers``, fp32, rows of at most
    :data:`deepinv_amd.hip.dst.MAX_N` elements.  A user-supplied ``transform_func`` / ``transform_func_inv`` runs the composed
    expression with those callables.

    :param tuple img_size: input shape.
    :param tuple output_size: output shape.
    :param float n_layers: number of layers :math:`N`, or :math:`N + 0.5`.
    :param Callable transform_func: default :func:`deepinv_amd.physics.functional.dst1`.
    :param Callable transform_func_inv: default :func:`deepinv_amd.physics.functional.dst1`.
    :param list diagonals: diagonals of the working size (a list of tensors or a stacked tensor); default Rademacher draws.
    :param str device: device of the physics.
    :param torch.Generator rng: generator of the default diagonals.
    """

    def __init__(self, img_size, output_size, n_layers=1, transform_func=dst1, transform_func_inv=dst1, diagonals=None,
                 device="cpu", rng: torch.Generator = None, **kwargs):
        super().__init__(device=device, **kwargs)
        self.mode = compare(img_size, output_size) if len(img_size) == 3 else None
        self.img_size = img_size
        self.output_size = output_size
        self.n_layers = n_layers
        self.transform_func = transform_func
        self.transform_func_inv = transform_func_inv
        L = math.floor(n_layers)
        if self.mode is None:
            work = tuple(img_size)
        else:
            work = tuple(max(a, b) for a, b in zip(img_size, output_size))
        if diagonals is None:
            if self.mode == "oversampling" and L > 0:
                raise ValueError(f"oversampling needs diagonals= of the output size {tuple(output_size)}: the default ones have "
                                 f"the image size {tuple(img_size)} (the reference fails with a broadcast error at the first call)")
            shape = (L, *img_size)
            diagonals = torch.stack([generate_diagonal(shape=tuple(img_size), mode="rademacher", dtype=torch.float, generator=rng,
                                                       device=device) for _ in range(L)], dim=0) if L else torch.zeros(shape, device=device)
        elif isinstance(diagonals, list):
            diagonals = torch.stack(diagonals, dim=0) if len(diagonals) else torch.zeros((0, *work), device=device)
        if diagonals.is_complex():
            raise NotImplementedError("complex diagonals belong to phase retrieval; deepinv_amd's StructuredRandom is real")
        if L > 0 and (diagonals.shape[0] < L or tuple(diagonals.shape[1:]) != work):
            raise ValueError(f"the diagonals must have shape [{L}, {', '.join(map(str, work))}] (the working size: the larger of "
                             f"img_size and output_size), got {tuple(diagonals.shape)}")
        self.register_buffer("diagonals", diagonals)
        self.to(device)

    # ------------------------------------------------------------------ the fused path
    def _fused(self):
        return self.transform_func is dst1 and self.transform_func_inv is dst1 and self.diagonals.dtype == torch.float32

    def _geometry(self, adjoint):
        """(in_hw, out_hw, work_hw, top, left, diag_rows) of hip/dst.py for A (or A_adjoint)"""
        if self.mode is None:
            n = int(self.img_size[-1])
            rows = 1
            for s in self.img_size[:-1]:
                rows *= int(s)
            return (1, n), (1, n), (1, n), 0, 0, rows
        C, H, W = (int(s) for s in self.img_size)
        _, Ho, Wo = (int(s) for s in self.output_size)
        top, _, left, _ = _changes(self.img_size, self.output_size)
        work = (max(H, Ho), max(W, Wo))
        a, b = ((Ho, Wo), (H, W)) if adjoint else ((H, W), (Ho, Wo))
        return a, b, work, top, left, C * work[0]

    def _run(self, x, adjoint):
        L = math.floor(self.n_layers)
        half = self.n_layers - L == 0.5
        geom = self._geometry(adjoint)
        (h_in, w_in), (h_out, w_out) = geom[0], geom[1]
        if self.mode is None:
            if x.shape[-1] != w_in:
                raise ValueError(f"expected a last dimension of {w_in}, got shape {tuple(x.shape)}")
            # rows of the flattened input: the diagonal row of a row is its index modulo the rows of img_size
            lead, x3 = x.shape[:-1], x.reshape(-1, 1, w_in)
        else:
            if x.dim() < 3 or tuple(x.shape[-2:]) != (h_in, w_in) or x.shape[-3] != self.img_size[0]:
                raise ValueError(f"expected an input [..., {self.img_size[0]}, {h_in}, {w_in}], got shape {tuple(x.shape)}")
            lead, x3 = x.shape[:-2], x.reshape(-1, h_in, w_in)
        if L + half == 0:
            return padding(x, self.img_size, self.output_size) if h_out > h_in or w_out > w_in else trimming(x, self.img_size, self.output_size)
        out = hd.structured_apply(x3, self.diagonals[:L], geom, L, half, adjoint)
        return out.reshape(*lead, w_out) if self.mode is None else out.reshape(*lead, h_out, w_out)

    # ------------------------------------------------------------------ operators
    def A(self, x: Tensor, *args, **kwargs) -> Tensor:
        if self._fused():
            return self._run(x, False)
        if self.mode == "oversampling":
            x = padding(x, self.img_size, self.output_size)
        if self.n_layers - math.floor(self.n_layers) == 0.5:
            x = self.transform_func(x)
        for i in range(math.floor(self.n_layers)):
            x = self.diagonals[i] * x
            x = self.transform_func(x)
        if self.mode == "undersampling":
            x = trimming(x, self.img_size, self.output_size)
        return x

    def A_adjoint(self, y: Tensor, *args, **kwargs) -> Tensor:
        if self._fused():
            return self._run(y, True)
        if self.mode == "undersampling":
            y = padding(y, self.img_size, self.output_size)
        for i in range(math.floor(self.n_layers)):
            y = self.transform_func_inv(y)
            y = torch.conj(self.diagonals[-i - 1]) * y
        if self.n_layers - math.floor(self.n_layers) == 0.5:
            y = self.transform_func_inv(y)
        if self.mode == "oversampling":
            y = trimming(y, self.img_size, self.output_size)
        return y
