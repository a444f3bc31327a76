"""ctypes wrapper of the ptychography kernels of csrc/cstructured.hip: ``B = [F diag(p_l)]_l`` with ``F`` the orthonormal 2-D DFT and
``p_l`` the probe at position ``l``, its adjoint ``sum_l conj(p_l) F^-1 y_l`` and the normal operation
``x -> sum_l conj(p_l) F^-1 f(F p_l x, aux_l)`` with the pointwise stage ``f`` between the transforms (include/deepinv_amd.h,
dinv_ptycho_apply).  complex64 only: an input of another dtype raises, it is not cast.  The probe ``[L, H, W]`` is float32 or
complex64 and is read where it lies: no converted copy is kept.

Two paths compute the same thing:

* fused: a workgroup holds a plane in LDS; the forward is one launch, the adjoint and the normal operation are one launch when a
  single group of positions covers all ``L`` and two (partial sums, then a fixed-order reduce) otherwise.  Taken whenever
  :func:`deepinv_amd.hip.cstructured.fits` says that the plane fits;
* composed: ``hip.fft.fftn`` / ``ifftn`` over ``[B, L, H, W]`` with the probe product, the sum and the epilogue as torch expressions
  on the device.  Taken by every larger plane.

``group`` is the number of positions a workgroup sums in registers: 0 lets the library fill the device, a positive value forces it
(values above ``L`` mean ``L``).  Results are bit-identical from call to call for a given group size.

The fused call is a ``torch.autograd.Function`` under the autograd rule of hip/epilogue.py, with the ``ADJOINT`` operation as the
adjoint and the ``NORMAL`` one for ``2 B^H (z g)``, the backward of ``ABS2``.  The probe and the real
array of an epilogue are buffers of the operator: no gradient flows to them."""
from __future__ import annotations

import ctypes

import torch

from . import FftPlan, check, declare_once, fft_plan, lib, ptr, require_hip, stream_ptr
from . import fft as hfft
from . import epilogue as ep
from .epilogue import ABS2, AMPLITUDE, NONE, WEIGHT, operand
from .cstructured import _epilogue, fits

FORWARD, ADJOINT, NORMAL = 0, 1, 2      # DINV_PTYCHO_*


def _declare(l):
    vp, i32, i64, sz, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float
    plan = ctypes.POINTER(FftPlan)
    l.dinv_ptycho_workspace_bytes.restype = sz
    l.dinv_ptycho_workspace_bytes.argtypes = [i64, i32, i32, i32, i32, i32]
    l.dinv_ptycho_apply.argtypes = [vp, vp, vp, i32, vp, i64, i32, i32, i32, i32, i32, f32, i32, plan, vp, plan, vp, vp, sz, vp]


def _l():
    return declare_once(lib(), _declare)


def groups(B: int, L: int, H: int, W: int, op: int, group: int = 0) -> int:
    """how many partial planes per image a fused call of these sizes writes: 1 means that the workgroup stores the result itself
    (one launch), more that a reduce launch follows"""
    if B < 1:
        return 1
    return max(_l().dinv_ptycho_workspace_bytes(B, L, H, W, op, group) // (8 * B * H * W), 1)


def _probe(probe: torch.Tensor, H: int, W: int) -> torch.Tensor:
    if probe.dtype not in (torch.float32, torch.complex64):
        raise TypeError(f"the probe must be float32 or complex64, got {probe.dtype}")
    if probe.dim() < 3 or tuple(probe.shape[-2:]) != (H, W) or probe.numel() != probe.shape[-3] * H * W:
        raise ValueError(f"expected a probe stack [L, {H}, {W}], got shape {tuple(probe.shape)}")
    return probe.resolve_conj().contiguous()


def _shapes(x, probe, op):
    H, W = int(probe.shape[-2]), int(probe.shape[-1])
    L = int(probe.shape[-3])
    want = (L, H, W) if op == ADJOINT else (H, W)
    if x.dim() != len(want) + 1 or tuple(x.shape[1:]) != want:
        raise ValueError(f"expected an input [batch, {', '.join(map(str, want))}], got shape {tuple(x.shape)}")
    return int(x.shape[0]), L, H, W


def _check_epilogue(op, epilogue):
    if op == ADJOINT and epilogue != NONE:
        raise ValueError("the adjoint has no epilogue")
    if op == NORMAL and epilogue not in (WEIGHT, AMPLITUDE):
        raise ValueError("the normal operation takes the WEIGHT or the AMPLITUDE stage between its transforms")


def _composed(x, probe, op, epilogue, aux, eps):
    x = operand(x, "the input")
    B, L, H, W = _shapes(x, probe, op)
    p = probe.reshape(1, L, H, W)
    if aux is not None:
        aux = aux.reshape(B, L, H, W)
    if op == ADJOINT:
        return (torch.conj(p) * hfft.ifftn(x)).sum(dim=1).contiguous()
    z = _epilogue(hfft.fftn((p * x.unsqueeze(1)).contiguous()), epilogue, aux, eps)
    if op == FORWARD:
        return z.contiguous()
    return (torch.conj(p) * hfft.ifftn(z.contiguous())).sum(dim=1).contiguous()


def _fused(x, probe, op, epilogue, aux, eps, group):
    x = operand(x, "the input")
    B, L, H, W = _shapes(x, probe, op)
    if op == FORWARD:
        out = torch.empty((B, L, H, W), dtype=torch.float32 if epilogue == ABS2 else torch.complex64, device=x.device)
    else:
        out = torch.empty((B, H, W), dtype=torch.complex64, device=x.device)
    aux = ep.aux_operand(epilogue, aux, (B, L, H, W))
    if B == 0:
        return out
    l = _l()
    nbytes = l.dinv_ptycho_workspace_bytes(B, L, H, W, op, group)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    pw, tw = fft_plan(W, x.device)
    ph, th = fft_plan(H, x.device)
    check(l.dinv_ptycho_apply(ptr(x), ptr(out), ptr(probe), int(probe.is_complex()), ptr(aux), B, L, H, W, op, epilogue, float(eps),
                              group, ctypes.byref(pw), ptr(tw), ctypes.byref(ph), ptr(th), ptr(ws), nbytes, stream_ptr(x.device)))
    return out


class _Ptycho(torch.autograd.Function):
    """one operation of the fused path; backward is the adjoint operation, or the normal one for ABS2"""

    @staticmethod
    def forward(x, probe, op, epilogue, aux, eps, group):
        return _fused(x, probe, op, epilogue, aux, eps, group)

    @staticmethod
    def setup_context(ctx, inputs, output):
        x, probe, ctx.op, epilogue, aux, _, ctx.group = inputs
        ep.setup_context(ctx, output, x, probe, epilogue, aux)

    @staticmethod
    def backward(ctx, g):
        _, probe, aux = ctx.saved_tensors
        run = lambda v, op, e=NONE, a=None: _Ptycho.apply(v, probe, op, e, a, 0.0, ctx.group)
        if ctx.op == NORMAL:
            # B^H diag(w) B is Hermitian for real weights
            gx = run(g, NORMAL, WEIGHT, aux)
        else:
            # FORWARD through its epilogue, or ADJOINT, which has none
            gx = ep.backward(ctx, g, run=lambda v, e, a: run(v, FORWARD, e, a),
                             adjoint=lambda v: run(v, ADJOINT if ctx.op == FORWARD else FORWARD),
                             normal=lambda v, w: run(v, NORMAL, WEIGHT, w))
        return gx, None, None, None, None, None, None


def apply(x, probe, op: int = FORWARD, epilogue: int = NONE, aux=None, eps: float = 1e-12, group: int = 0):
    """``probe`` is ``[L, H, W]`` float32 or complex64.  ``op = FORWARD``: x ``[B, H, W]`` complex64 -> ``[B, L, H, W]`` through the
    epilogue (real for ``ABS2``); ``ADJOINT``: x ``[B, L, H, W]`` -> ``[B, H, W]``; ``NORMAL``: x ``[B, H, W]`` -> ``[B, H, W]`` with
    ``epilogue`` (``WEIGHT`` or ``AMPLITUDE``) and ``aux`` ``[B, L, H, W]`` real between the transforms."""
    require_hip(x, probe, aux)
    op, epilogue, group = int(op), int(epilogue), int(group)
    if op not in (FORWARD, ADJOINT, NORMAL):
        raise ValueError(f"unknown operation {op}")
    _check_epilogue(op, epilogue)
    if group < 0:
        raise ValueError(f"group must be 0 (automatic) or the positions per workgroup, got {group}")
    probe = _probe(probe, *probe.shape[-2:])
    _shapes(x, probe, op)
    if fits(*probe.shape[-2:]):
        return _Ptycho.apply(x, probe, op, epilogue, aux, float(eps), group)
    return _composed(x, probe, op, epilogue, aux, float(eps))
