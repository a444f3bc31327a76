"""DnCNN denoiser on the hand-written HIP convolution kernels (csrc/drunet*.hip) - inference and training, 2-D.

Module tree and parameter names are those of the reference (deepinv/models/dncnn.py: ``in_conv``, ``conv_list.{i}``,
``out_conv``), so reference ``state_dict``s load unchanged.  The ``nn.Conv2d`` modules only hold the parameters: no forward
of this class runs a PyTorch-ROCm (MIOpen) convolution, and an architecture the kernels do not cover raises at construction.

* head ``relu(in_conv(x))``: direct fp32 kernel with the bias in its epilogue (``dinv_conv3x3_bias``);
* body ``relu(conv_list[i](x1))``: Winograd F(4x4,3x3) on the fp32 matrix cores with the bias after the inverse transform
  (``dinv_conv3x3_winograd4_bias``) where nf % 64 == 0 and H, W % 4 == 0, else the direct kernel;
* tail ``out_conv(x1) + x``: vector-ALU kernel for up to 4 channels (``dinv_conv3x3_tail_bias``), the thin 16-wide MFMA
  kernel for 5-7, bias and residual fused into the store;
* with gradients: forward and backward as ONE ``torch.autograd.Function`` (``DnCNNFunction``).

``bias=False`` runs the bias-free entry points of DRUNet.  Activations live in the padded channel-blocked layout of
``hip/drunet.py``; the buffers of one (device, shape) are allocated once and ping-ponged, and nothing synchronises with the
host, so a PnP loop with this denoiser can be captured as a HIP graph (``FixedPoint.use_graph``).
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import hip as H
from ..hip import drunet as K
from .base import Denoiser
from .unet_autograd import _flip_t


def weights_init_kaiming(m):
    """deepinv/models/dncnn.py: Kaiming-normal weights (fan_in), biases keep PyTorch's default"""
    if m.__class__.__name__.find("Conv") != -1:
        nn.init.kaiming_normal_(m.weight.data, a=0, mode="fan_in")


class DnCNN(Denoiser):
    r"""DnCNN (Zhang et al. 2017, without batch normalisation), as ``deepinv.models.DnCNN``.

    :param int in_channels: input image channels (1..7)
    :param int out_channels: output image channels (must equal ``in_channels``: the output adds the input)
    :param int depth: number of convolutional layers (>= 2)
    :param bool bias: use bias in the convolutional layers
    :param int nf: number of channels per convolutional layer
    :param str, None pretrained: ``None`` (Kaiming initialisation) or a path to a state dict; ``"download*"`` needs network
        access and raises
    :param torch.device, str device: device to put the model on
    :param int, str dim: 2 only
    """

    def __init__(self, in_channels=3, out_channels=3, depth=20, bias=True, nf=64, pretrained=None,
                 pretrained_2d_isotropic=False, device=None, dim=2):
        super().__init__()
        dim = int(str(dim).lower().replace("d", "")) if not isinstance(dim, int) else dim
        if dim != 2:
            raise NotImplementedError(f"DnCNN(dim={dim}): only 2-D DnCNN runs on the HIP convolution kernels")
        if in_channels != out_channels:
            raise NotImplementedError(f"DnCNN({in_channels} -> {out_channels} channels): the fused tail adds the input image "
                                      "to the output, so in_channels must equal out_channels")
        if not 1 <= in_channels <= 7:
            raise NotImplementedError(f"DnCNN with {in_channels} channels: the packed input layout holds 1..7 image channels")
        if depth < 2:
            raise NotImplementedError(f"DnCNN(depth={depth}): needs at least the head and the tail layer (depth >= 2)")
        if nf < 1:
            raise ValueError(f"nf must be positive, got {nf}")
        self.in_channels, self.out_channels, self.nf, self.has_bias, self.dim = in_channels, out_channels, nf, bias, dim
        self.depth = depth
        self.in_conv = nn.Conv2d(in_channels, nf, kernel_size=3, stride=1, padding=1, bias=bias)
        self.conv_list = nn.ModuleList([nn.Conv2d(nf, nf, kernel_size=3, stride=1, padding=1, bias=bias)
                                        for _ in range(depth - 2)])
        self.out_conv = nn.Conv2d(nf, out_channels, kernel_size=3, stride=1, padding=1, bias=bias)
        self.nl_list = nn.ModuleList([nn.ReLU() for _ in range(depth - 1)])
        self._engine = None
        if pretrained is not None:
            if str(pretrained).startswith("download"):
                raise RuntimeError("no network access: pass pretrained=<path to .pth> or None")
            self.load_state_dict(torch.load(pretrained, map_location="cpu"), strict=True)
            self.eval()
        else:
            self.apply(weights_init_kaiming)
        if device is not None:
            self.to(device)

    def layers(self):
        return [self.in_conv, *self.conv_list, self.out_conv]

    def forward(self, x, sigma=None):
        """``out_conv(x1) + x``; ``sigma`` is not used (as in the reference)"""
        H.require_hip(x)
        if x.ndim != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"DnCNN expects [B, {self.in_channels}, H, W], got {tuple(x.shape)}")
        params = list(self.parameters())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return DnCNNFunction.apply(self, x, *params)
        return self._hip_forward(x)

    # ------------------------------------------------------------------ inference engine
    def _prepare(self, device):
        ver = K.weights_version(self)
        if self._engine is not None and self._engine["ver"] == ver and self._engine["device"] == device:
            return self._engine
        e = {"ver": ver, "device": device, "ws": {}}
        e["head"] = _direct_packs(self.in_conv, device)
        e["body"] = [_direct_packs(m, device, wino4=self.nf % 64 == 0) for m in self.conv_list]
        e["tail"] = _tail_pack(self.out_conv, device)
        self._engine = e
        return e

    def _workspace(self, e, B, Hh, W, device):
        key = (B, Hh, W)
        ws = e["ws"].get(key)
        if ws is None:
            e["ws"].clear()          # one image geometry at a time keeps the footprint bounded
            g = K.geom(B, Hh, W)
            ws = {"g": g, "in": K.alloc(g, 8, device), "a": K.alloc(g, self.nf, device), "b": K.alloc(g, self.nf, device),
                  "out": K.alloc(g, 8, device)}
            e["ws"][key] = ws
        return ws

    def _hip_forward(self, x):
        dev = x.device
        e = self._prepare(dev)
        B, C, Hh, W = x.shape
        ws = self._workspace(e, B, Hh, W, dev)
        g = ws["g"]
        K.pack_input(g, x.contiguous().float(), 0.0, ws["in"])      # channel C (the noise-map slot) = 0: nothing to add
        _layer(g, e["head"], ws["in"], ws["a"], self.nf, relu=True)
        cur, nxt = ws["a"], ws["b"]
        wino_ok = Hh % 4 == 0 and W % 4 == 0
        for pk in e["body"]:
            if pk.wino4 is not None and wino_ok:
                _winograd(g, pk, cur, nxt, self.nf)
            else:
                _layer(g, pk, cur, nxt, self.nf, relu=True)
            cur, nxt = nxt, cur
        _tail(g, e["tail"], cur, ws["in"], ws["out"], self.out_channels)
        y = torch.empty((B, C, Hh, W), device=dev, dtype=torch.float32)
        K.unpack_output(g, ws["out"], C, y)
        return y


# ---- layer helpers: a "pack" is a K.ConvPacks with the direct packs (64- / 32-wide cout tiles), the zero-padded fp32 bias
# (None for bias=False) and, for the body layers the F(4x4) kernel takes, its pack - no other: DnCNN launches no other kernel
def _direct_packs(m, device, wino4=False):
    w = m.weight.to(device)
    pk = K.conv_packs(w, m.bias.to(device) if m.bias is not None else None)
    return pk._replace(wino4=K.pack_winograd4_weight(w)) if wino4 else pk


def _tail_pack(m, device):
    """("valu", w_tail, bias) for <= 4 output channels, else ("thin", w_thin, bias16); bias None for bias=False"""
    w = m.weight.to(device)
    cout, cin = w.shape[:2]
    cin_p = (cin + 7) // 8 * 8
    if cout <= 4 and m.bias is not None:
        wp = torch.zeros((cout, cin_p, 3, 3), device=device, dtype=torch.float32)
        wp[:, :cin] = w.detach().float()
        return ("valu", K.pack_tail_weight(wp), K.pack_bias(m.bias.to(device), cout), cin_p)
    wt, cin_p = K.pack_thin_weight(w)
    return ("thin", wt, K.pack_bias(m.bias.to(device), 16) if m.bias is not None else None, cin_p)


def _layer(g, pk, x, y, cout, relu=False, res1=None):
    """y = [relu](conv(x) + b) (+res1) on the direct fp32 kernel (the bias-free kernel when there is no bias)"""
    if pk.bias is not None:
        K.conv3x3_bias(g, x, pk.pick(g), pk.bias, pk.cin_p, pk.cout_p, y, cout_valid=cout, res1=res1, relu=relu)
    else:
        K.conv3x3(g, x, pk.pick(g), pk.cin_p, pk.cout_p, y, cout_valid=cout, res1=res1, relu=relu)


def _winograd(g, pk, x, y, nf):
    wsp = K.winograd4_workspace(x.device)
    if pk.bias is not None:
        K.conv3x3_winograd4_bias(g, x, pk.wino4, pk.bias, nf, nf, y, relu=True, workspace=wsp)
    else:
        K.conv3x3_winograd4(g, x, pk.wino4, nf, nf, y, relu=True, workspace=wsp)


def _tail(g, tp, x, res, y, cout):
    """y = out_conv(x) (+ b) + res"""
    kind, w, b, cin_p = tp
    if kind == "valu":
        K.conv3x3_tail_bias(g, x, w, b, cin_p, cout, y, res=res)
    elif b is not None:
        K.conv3x3_bias(g, x, w, b, cin_p, 16, y, cout_valid=cout, res1=res)
    else:
        K.conv3x3(g, x, w, cin_p, 16, y, cout_valid=cout, res1=res)


class DnCNNFunction(torch.autograd.Function):
    """``y = DnCNN(x)`` with forward and backward on the HIP kernels; parameters passed explicitly (parameters() order:
    weight then bias of in_conv, conv_list.0, ..., out_conv).

    forward: the direct fp32 kernels for every layer (the ReLU masks are those of an fp32 reference), each
    post-ReLU activation kept; backward: data gradients by the flipped, transposed filters with the ReLU gate, weight gradients
    by ``dinv_conv_wgrad``, bias gradients by ``dinv_bias_grad`` (both deterministic), the input gradient including the
    residual.  Double backward is not supported."""

    @staticmethod
    def forward(ctx, model, x, *params):
        dev = x.device
        B, C, Hh, W = x.shape
        nf, has_b = model.nf, model.has_bias
        ws_, bs_ = [], []
        it = iter(params)
        for _ in model.layers():
            ws_.append(next(it).detach().float())
            bs_.append(next(it).detach().float() if has_b else None)
        g = K.geom(B, Hh, W)
        x_act = K.alloc(g, 8, dev)
        K.pack_input(g, x.detach().contiguous().float(), 0.0, x_act)
        acts = []
        cur = x_act
        for i in range(model.depth - 1):
            w = ws_[i]
            pk = _fwd_pack(w, bs_[i], "dnf")
            y = K.alloc(g, nf, dev)
            _layer(g, pk, cur, y, nf, relu=True)
            acts.append(y)
            cur = y
        out = K.alloc(g, 8, dev)
        _tail(g, _tail_pack(_Holder(ws_[-1], bs_[-1]), dev), cur, x_act, out, C)
        y = torch.empty((B, C, Hh, W), device=dev, dtype=torch.float32)
        K.unpack_output(g, out, C, y)
        ctx.model, ctx.g, ctx.W, ctx.acts, ctx.x_act = model, g, ws_, acts, x_act
        ctx.has_b = has_b
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        model, g, W, acts, x_act = ctx.model, ctx.g, ctx.W, ctx.acts, ctx.x_act
        nf, C, L = model.nf, model.in_channels, model.depth
        dev = gy.device
        need = ctx.needs_input_grad
        gy_act = K.alloc(g, 8, dev)
        K.pack_input(g, gy.contiguous().float(), 0.0, gy_act)
        dW, dB = [None] * L, [None] * L
        # layer l (0 = in_conv, L - 1 = out_conv): input act_in(l) = x_act for l = 0 else acts[l - 1]; s = gradient at its output
        s = gy_act
        for l in range(L - 1, -1, -1):
            cout = C if l == L - 1 else nf
            lin = x_act if l == 0 else acts[l - 1]
            cin = C if l == 0 else nf
            if need[2 + (2 if ctx.has_b else 1) * l]:
                dW[l] = K.conv_wgrad(g, g, s, cout, lin, cin, 9)
            if ctx.has_b and need[3 + 2 * l]:
                dB[l] = K.bias_grad(g, s, cout)
            if l == 0:
                break
            # data gradient through the flipped, transposed filter, then the ReLU gate of the layer below
            pk = _fwd_pack(W[l], None, "dnb", flip=True)
            nxt = K.alloc(g, nf, dev)
            _layer(g, pk, s, nxt, nf)
            K.relu_backward(acts[l - 1], nxt)
            s = nxt
        gx = None
        if need[1]:
            pk = _fwd_pack(W[0], None, "dnb", flip=True)
            gin = K.alloc(g, 8, dev)
            _layer(g, pk, s, gin, C, res1=gy_act)       # + the residual: d(out_conv(x1) + x)/dx
            gx = torch.empty_like(gy, dtype=torch.float32)
            K.unpack_output(g, gin, C, gx)
        ctx.acts = ctx.x_act = None
        grads = []
        for l in range(L):
            grads.append(dW[l])
            if ctx.has_b:
                grads.append(dB[l])
        return (None, gx, *grads)


class _Holder:
    """weight / bias pair in the shape of an nn.Conv2d for the pack helpers"""

    def __init__(self, w, b):
        self.weight, self.bias = w, b


def _fwd_pack(w, b, kind, flip=False):
    """direct-kernel packs of a (flipped) weight, cached per weight tensor and version; the bias is packed per call (a few floats)"""
    pk = K.cached_pack((kind, flip), w, lambda: K.conv_packs(_flip_t(w) if flip else w))
    return pk._replace(bias=K.pack_bias(b, pk.cout_p)) if b is not None else pk
