"""DRUNet forward + backward on the HIP kernels (2-D), for training through ``deepinv.unfolded``
(deepinv/unfolded/unfolded.py:116-226 with a DRUNet prior, deepinv/models/drunet.py:39-263).

The reference differentiates the 64 convolutions with autograd (ATen / cuDNN kernels).  Here the whole network is ONE
``torch.autograd.Function`` (models/unet_autograd.py: the walk shared with ``dim=3``; this module supplies its 2-D operations):

* forward: the same kernels as inference (bf16-split 3x3 / 2x2 convolutions, direct fp32 kernel for the thin head and
  tail), every ResBlock input and post-ReLU activation kept for the backward pass;
* data gradients: the forward kernels again, on re-packed weights - d/dx of a 3x3 convolution is the 3x3 convolution
  with the transposed, spatially flipped filter; d/dx of the 2x2 stride-2 convolution is the 2x2 stride-2 transposed
  convolution with the same filter, and vice versa;
* weight gradients: ``dinv_conv_wgrad`` (csrc/drunet_bwd.hip, fp32 matrix cores, deterministic);
* ReLU backward and the skip-connection sums: ``dinv_relu_backward`` / ``dinv_lincomb``.

Gradients are returned for the input image, the noise-level map (the trainable ``g_param`` of unfolded PnP) and every
convolution weight.  Double backward is not supported.

ReLU masks: the bf16-split convolutions are fp32-class (a few 1e-6 relative), which is enough to flip ``relu'(z)`` for
the handful of pre-activations that lie within that distance of zero; one flipped mask entry changes one row of a
weight gradient by ~1/sqrt(pixels) (measured: 5e-3 .. 1e-2 on the 256 / 512-channel levels at 2 x 12 x 16 pixels, against
7e-7 without flips; data gradients are unaffected: 3e-6).  The FORWARD pass of the training path therefore runs on the
fp32 matrix cores by default (direct kernels, 3e-7 per layer: the masks are those of an fp32 reference);
``DINV_DRUNET_TRAIN_PRECISION=bf16s`` uses the inference kernels instead (faster forward, mask flips at the 1e-6 level).
The backward pass always uses the bf16-split kernels for the data gradients (no ReLU decision depends on them)."""
from __future__ import annotations


import torch

from ..hip import drunet as K
from ..hip import elementwise as ew
from . import unet_autograd
from .unet_autograd import _flip_t, _pad_w, _r64


def supported(model) -> bool:
    """any 4-level 2-D DRUNet: channel counts that are not multiples of 64 (what the 2x2 kernels take) are zero-padded -
    padded channels stay exactly zero through convolutions, ReLUs and residual adds, their gradients are sliced away"""
    return model.dim == 2 and len(model.nc) == 4


def _fp32_forward(model) -> bool:
    v = getattr(model, "train_forward_precision", "fp32")
    if v not in ("fp32", "bf16split"):
        raise ValueError(f"train_forward_precision must be fp32 or bf16split, got {v}")
    return v == "fp32"


def _conv3(g, w, x, relu=False, res1=None, fp32=False, flip=False, gate=None):
    """y = [relu](conv3x3(x, w)) (+ res1) on activation buffers; bf16-split kernel where the shapes allow it.
    flip: convolve with the transposed, tap-reversed filter (the data gradient of the same layer); packs are cached per
    weight tensor and version (hip/drunet.py: cached_pack).  gate: the forward pass's ReLU output whose sign masks the
    result (ReLU backward fused into the epilogue of the data-gradient convolution)"""
    cout, cin = (w.shape[1], w.shape[0]) if flip else w.shape[:2]
    y = K.alloc(g, cout, x.device)
    src = lambda: _flip_t(w) if flip else w  # noqa: E731
    if cout % 64 == 0 and cin % 16 == 0 and not fp32:
        K.conv3x3_split(g, x, K.cached_pack(("c3s", flip), w, lambda: K.pack_split2d_weight(src())), cin, cout, y,
                        res1=gate if gate is not None else res1, relu=relu, gate=gate is not None)
    else:
        wpk, ci_p, co_p = K.cached_pack(("c3d", flip), w, lambda: K.pack_conv3x3_weight(src()))
        K.conv3x3(g, x, wpk, ci_p, co_p, y, cout_valid=cout, res1=res1, relu=relu)
        if gate is not None:
            K.relu_backward(gate, y)
    return y


def _stride_packs(w, up, fp32):
    """packs of a 2x2 stride-2 filter, cached per weight tensor and version: the bf16-split kernel where the shapes allow it, the
    direct kernel with `fp32`"""
    precision = None if fp32 else "bf16split"
    return K.cached_pack(("s2", up, precision), w, lambda: K.stride_packs(w, up=up, precision=precision))


class Ops2d:
    """what models/unet_autograd.py walks with, for 2-D: activation tensors [C/8, cs, 8] of `K.alloc`, weights zero-padded to
    multiples of 64 channels up front (their gradients are sliced back), the ResBlock / stride-2 / transposed convolutions of the
    forward pass in fp32 arithmetic unless `train_forward_precision` says otherwise, the thin head and tail as their shapes allow"""
    fp32_ends = False

    def __init__(self, model, xin, train):
        B, _, H, Wd = xin.shape
        self.g = [K.geom(B, H >> i, Wd >> i) for i in range(4)]
        self.fp32 = _fp32_forward(model)

    @staticmethod
    def weight(name, p):
        if name == "m_head.weight":
            return _pad_w(p, _r64(p.shape[0]), p.shape[1])
        if name == "m_tail.weight":
            return _pad_w(p, p.shape[0], _r64(p.shape[1]))
        return _pad_w(p, _r64(p.shape[0]), _r64(p.shape[1]))

    @staticmethod
    def weight_grad(dw, shape):
        return dw[:shape[0], :shape[1]].contiguous()

    def pack(self, x, noise_channel):
        x = x.detach().contiguous().float()
        act = K.alloc(self.g[0], x.shape[1], x.device)
        if noise_channel:
            K.pack_input(self.g[0], x[:, :-1].contiguous(), x[:, -1:].contiguous(), act)
        else:
            K.pack_input(self.g[0], x, 0.0, act)
        return act

    def unpack(self, act, channels):
        g = self.g[0]
        y = torch.empty((g.batch, channels, g.height, g.width), device=act.device, dtype=torch.float32)
        K.unpack_output(g, act, channels, y)
        return y

    def conv3(self, i, w, x, relu=False, res=None, fp32=False, flip=False, gate=None):
        return _conv3(self.g[i], w, x, relu=relu, res1=res, fp32=fp32, flip=flip, gate=gate)

    def down(self, i, w, x, fp32=False):
        """2x2 stride-2 convolution with a [Cout,Cin,2,2] filter (also: data gradient of the transposed convolution)"""
        gi, go = self.g[i], self.g[i + 1]
        cout, cin = w.shape[:2]
        y = K.alloc(go, cout, x.device)
        K.launch_down(gi, go, x, _stride_packs(w, False, fp32), cin, cout, y)
        return y

    def up(self, i, w, x, fp32=False):
        """2x2 stride-2 transposed convolution with a [Cin,Cout,2,2] filter (also: data gradient of the strided one)"""
        gi, go = self.g[i + 1], self.g[i]
        cin, cout = w.shape[:2]
        y = K.alloc(go, cout, x.device)
        K.launch_up(gi, go, x, None, _stride_packs(w, True, fp32), cin, cout, y)
        return y

    @staticmethod
    def add(i, a, b):
        return ew.lincomb(1.0, a, 1.0, b)

    def wgrad3(self, i, gout, x, w):
        return K.conv_wgrad(self.g[i], self.g[i], gout, w.shape[0], x, w.shape[1], 9)

    def wgrad2(self, i, small, large, w):
        return K.conv_wgrad(self.g[i + 1], self.g[i], small, w.shape[0], large, w.shape[1], 4)


def forward_train(model, xin):
    """DRUNet(xin) recorded as one autograd node (all parameters of `model` are inputs of the node)"""
    return unet_autograd.forward(Ops2d, model, xin)
