"""ctypes wrapper of csrc/cstructured.hip: ``B = prod_i (F D_i) [F]`` with ``F`` the orthonormal 2-D DFT and complex64 diagonals,
or its adjoint, with a pointwise epilogue - the operator of StructuredRandomPhaseRetrieval (include/deepinv_amd.h,
dinv_cstructured_apply).  complex64 only: an input of another dtype raises, it is not cast.

Two paths compute the same thing:

* fused: one launch for any number of layers, a workgroup holds a whole working plane in LDS.  Taken whenever
  :func:`fits` says that the two buffers and the tables of the plane fit the LDS of a workgroup;
* composed: ``hip.fft.fftn`` / ``ifftn`` per layer with the pad, the diagonals, the trim and the epilogue as torch expressions on
  the device.  Taken by every larger plane.

The fused call is a ``torch.autograd.Function`` under the autograd rule of hip/epilogue.py, with the swapped geometry and the
flipped ``adjoint`` flag as the adjoint; the composed path is differentiated by autograd through its own ops.  The diagonals and the real array of
an epilogue are buffers of the operator: no gradient flows to them."""
from __future__ import annotations

import ctypes

import torch
import torch.nn.functional as F

from . import FftPlan, check, declare_once, fft_plan, lib, ptr, require_hip, stream_ptr
from . import fft as hfft
from . import epilogue as ep
from .epilogue import ABS2, NONE, WEIGHT, operand


def _declare(l):
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    plan = ctypes.POINTER(FftPlan)
    l.dinv_cstructured_fits.restype = ctypes.c_int
    l.dinv_cstructured_fits.argtypes = [i32, i32]
    l.dinv_cstructured_apply.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, i64, i32, i32, i32, i32, f32,
                                         plan, vp, plan, vp, vp]


def _l():
    return declare_once(lib(), _declare)


def fits(H: int, W: int) -> bool:
    """whether a working plane of H x W takes the fused kernel: its two buffers and the tables of both axes fit the LDS of a
    workgroup.  Larger planes take the composed path."""
    return bool(_l().dinv_cstructured_fits(int(H), int(W)))


def _epilogue(z, epilogue, aux, eps):
    if epilogue == NONE:
        return z
    if epilogue == ABS2:
        return z.real * z.real + z.imag * z.imag
    if epilogue == WEIGHT:
        return z * aux
    return z * (1 - torch.sqrt(aux / ((z.real * z.real + z.imag * z.imag) + eps)))


def _composed(x, diag, geom, layers, half, adjoint, epilogue, aux, eps):
    (h_in, w_in), (h_out, w_out), (H, W), top, left, planes = geom
    x = operand(x, "the input")
    if (h_in, w_in) != (H, W):
        x = F.pad(x, (left, W - w_in - left, top, H - h_in - top))
    if layers:
        d = operand(diag, "the diagonals").reshape(layers, planes, H, W)
        x = x.reshape(-1, planes, H, W)
    if not adjoint:
        if half:
            x = hfft.fftn(x)
        for i in range(layers):
            x = hfft.fftn(d[i] * x)
    else:
        for i in range(layers):
            x = torch.conj(d[layers - 1 - i]) * hfft.ifftn(x)
        if half:
            x = hfft.ifftn(x)
    x = x.reshape(-1, H, W)
    if (h_out, w_out) != (H, W):
        x = x[:, top:top + h_out, left:left + w_out]
    if aux is not None:
        aux = aux.reshape(x.shape)
    return _epilogue(x, epilogue, aux, eps).contiguous()


def _fused(x, diag, geom, layers, half, adjoint, epilogue, aux, eps):
    (h_in, w_in), (h_out, w_out), (H, W), top, left, dplanes = geom
    x = operand(x, "the input")
    planes = int(x.shape[0])
    out = torch.empty((planes, h_out, w_out), dtype=torch.float32 if epilogue == ABS2 else torch.complex64, device=x.device)
    aux = ep.aux_operand(epilogue, aux, out.shape)
    if layers:
        diag = operand(diag, "the diagonals")
        if diag.numel() != layers * dplanes * H * W:
            raise ValueError(f"the diagonals hold {diag.numel()} values, expected {layers} x {dplanes} x {H} x {W}")
    if planes == 0:
        return out
    pw, tw = fft_plan(W, x.device)
    ph, th = fft_plan(H, x.device)
    check(_l().dinv_cstructured_apply(ptr(x), ptr(out), ptr(diag) if layers else None, ptr(aux), planes, h_in, w_in, h_out, w_out, H, W,
                                      top, left, dplanes, layers, half, int(adjoint), epilogue, float(eps), ctypes.byref(pw), ptr(tw),
                                      ctypes.byref(ph), ptr(th), stream_ptr(x.device)))
    return out


class _CStructured(torch.autograd.Function):
    """B (adjoint = False) or B^H as one launch, through the epilogue; backward is the other one"""

    @staticmethod
    def forward(x, diag, geom, layers, half, adjoint, epilogue, aux, eps):
        return _fused(x, diag, geom, layers, half, adjoint, epilogue, aux, eps)

    @staticmethod
    def setup_context(ctx, inputs, output):
        x, diag, ctx.geom, ctx.layers, ctx.half, ctx.adjoint, epilogue, aux, _ = inputs
        ep.setup_context(ctx, output, x, diag, epilogue, aux)

    @staticmethod
    def backward(ctx, g):
        diag = ctx.saved_tensors[1]
        i, o, w, top, left, planes = ctx.geom
        back = (o, i, w, top, left, planes)
        run = lambda v, geom, adjoint, e, a: _CStructured.apply(v, diag, geom, ctx.layers, ctx.half, adjoint, e, a, 0.0)
        gx = ep.backward(ctx, g, run=lambda v, e, a: run(v, ctx.geom, ctx.adjoint, e, a),
                         adjoint=lambda v: run(v, back, not ctx.adjoint, NONE, None))
        return gx, None, None, None, None, None, None, None, None


def apply(x, diag, geom, layers: int, half: bool, adjoint: bool, epilogue: int = NONE, aux=None, eps: float = 1e-12):
    """x is [planes, H_in, W_in] complex64; geom = (in_hw, out_hw, work_hw, top, left, diag_planes): the side x has, the side the
    result has, the working side (the larger of the two), the offsets of the smaller side in it and the planes of one diagonal
    (plane p uses diagonal plane p % diag_planes).  diag is [layers, diag_planes, H_work, W_work] complex64."""
    require_hip(x, diag if layers else None, aux)
    (h_in, w_in), _, (H, W) = geom[0], geom[1], geom[2]
    if x.dim() != 3 or tuple(x.shape[1:]) != (h_in, w_in):
        raise ValueError(f"expected an input [planes, {h_in}, {w_in}], got shape {tuple(x.shape)}")
    if layers + int(bool(half)) < 1:
        raise ValueError("the operator needs at least one transform")
    if fits(H, W):
        return _CStructured.apply(x, diag, geom, int(layers), int(bool(half)), bool(adjoint), int(epilogue), aux, float(eps))
    return _composed(x, diag, geom, int(layers), int(bool(half)), bool(adjoint), int(epilogue), aux, float(eps))
