"""DRUNet with ``dim=3`` (Conv3d / ConvTranspose3d, deepinv/models/drunet.py:39-263) forward + backward on the 2-D HIP
kernels - BASELINE config 4's denoiser (unfolded PGD on 3-D multi-coil MRI, deepinv/unfolded/unfolded.py:116-226).

A volume of D slices lives in the padded channel-blocked activation layout as D + 2 consecutive "images" (one zero
slice at each end), so that

* a 3x3x3 convolution is ONE launch of the 2-D-tile kernels with the three depth taps inside the K loop (tap dz reads
  the input shifted by dz - 1 slices), ReLU / residual / zeroed padding slices in the epilogue: ``dinv_conv3x3x3_split``
  (bf16-split arithmetic) or ``dinv_conv3x3x3`` (fp32; layers of <= 16 output channels on the 16x16x4 MFMA tile);
* the 2x2x2 stride-2 convolution / transposed convolution are two launches of the 2-D kernels with the slice pairing
  z <-> 2 z + dz done inside the kernel (``dinv_conv_down2x2_bf16s_3d`` / ``dinv_conv_up2x2_bf16s_3d``);
* data gradients are the same operators on re-packed weights (flipped + transposed 3x3x3 filters; down <-> up);
* weight gradients are ``dinv_conv_wgrad`` per depth tap (shifted views) and ``dinv_conv_wgrad_3d`` for the 2x2x2 layers.

Activation buffers are allocated with channel counts rounded up to 64 and every kernel gets its weights zero-padded to
what IT needs (bf16-split kernels: Cin to 16, Cout to 64; fp32 direct kernel: Cin to 8, Cout to 32; weight gradients:
the true counts) - the small config-4 network has 16 / 32 / 64 / 128 channels; padded channels stay exactly zero
through convolutions, ReLUs and residual adds.
The forward pass of the 3x3x3 convolutions runs on the fp32 matrix cores when gradients are requested (same reasoning
as models/drunet_train.py: ReLU masks of an fp32 reference), on the bf16-split kernels otherwise."""
from __future__ import annotations


import torch

from ..hip import drunet as K
from ..hip import elementwise as ew
from . import unet_autograd
from .unet_autograd import _flip_t, _pad_w, _r16, _r64


def supported(model) -> bool:
    return model.dim == 3 and len(model.nc) == 4


_POOL: dict = {}        # (device, channels, level shape) -> released activation buffers
POOL_MAX_BYTES = None          # cap of the free list; None = 40 % of the device's memory (config 4's training step holds ~45 GB of
                               # activations for its backward pass: under the 16-GiB cap of rounds 3-5 sixty 655-MB buffers per step
                               # fell off the list and were zero-filled again, 5 ms of the 154-ms step)
_POOL_CAPS: dict = {}
CHECK_RECYCLED = False         # debugging aid (the GPU test switches it on): verify the invariant below on every reuse
_pool_bytes = 0
_pool_sig = None               # (device, B, D, H, W) of the last call: another problem shape drops the whole list


def _pool_cap(device):
    if POOL_MAX_BYTES is not None:
        return POOL_MAX_BYTES
    if device not in _POOL_CAPS:
        _POOL_CAPS[device] = int(0.4 * torch.cuda.get_device_properties(device).total_memory) if device.type == "cuda" else 16 << 30
    return _POOL_CAPS[device]


class Vol:
    """activation volume: tensor [C/8, cs, 8] with one guard plane in front, so that slice-shifted views stay inside.

    Buffers are recycled through a free list keyed by (device, channel count, level shape) instead of being zero-filled
    per layer (the fills were 6 % of config 4's training step): every kernel that writes a volume writes ALL of its
    in-range pixels (exact zeros on frames and padding slices) and nothing outside, so a released buffer still has
    zero guard planes, zero slack and zero padded channel blocks - the only things a fresh ``torch.zeros`` adds."""

    def __init__(self, lv, channels, device):
        self.lv = lv
        self.presplit = False         # holds (8 bf16 high parts | 8 bf16 low parts) per pixel and channel block instead of 8 fp32 values
        self.sig = _pool_sig          # buffers of an earlier problem shape are not recycled when they die later
        self.key = (torch.device(device), int(channels), lv.B, lv.D, lv.H, lv.W)
        free = _POOL.get(self.key)
        if free:
            global _pool_bytes
            self.t = free.pop()
            _pool_bytes -= self.t.numel() * 4
            if CHECK_RECYCLED:
                self._check_clean(channels)
        else:
            self.t = torch.zeros((_r64(channels) // 8, lv.g.cs, 8), device=device, dtype=torch.float32)

    def _check_clean(self, channels):
        """the invariant recycling rests on: frames, padding slices, guard planes, slack and padded channel blocks of a
        released buffer are exactly zero (only interior voxels of real channel blocks may hold anything)"""
        lv, t = self.lv, self.t.clone()
        b, d, h, w = lv.B, lv.D, lv.H, lv.W
        vol = t[:, lv.guard + lv.g.sl: lv.guard + lv.g.sl + lv.g.np].view(t.shape[0], b, d + 2, h + 2, -1, 8)
        vol[:(int(channels) + 7) // 8, :, 1:-1, 1:h + 1, 1:w + 1] = 0
        bad = int(torch.count_nonzero(t))
        if bad:
            raise AssertionError(f"recycled activation buffer {self.key}: {bad} non-zero values outside the interior")

    def __del__(self):
        global _pool_bytes
        try:
            t, key = self.t, self.key
            if self.sig == _pool_sig and _pool_bytes + t.numel() * 4 <= _pool_cap(t.device):
                _POOL.setdefault(key, []).append(t)
                _pool_bytes += t.numel() * 4
        except Exception:       # interpreter shutdown
            pass

    def view(self, dz=0):
        return self.t[:, self.lv.guard + dz * self.lv.g.plane:]


class Level:
    def __init__(self, B, D, H, W):
        self.B, self.D, self.H, self.W = B, D, H, W
        self.g = K.geom(B * (D + 2), H, W)
        self.guard = int(self.g.plane)
        self.g.cs = (self.g.cs + 2 * self.guard + 3) // 4 * 4


def release_buffers():
    """drop the recycled activation buffers (kept between calls of the SAME problem shape, at most POOL_MAX_BYTES; a call
    with another shape drops them by itself)"""
    global _pool_bytes
    _POOL.clear()
    _pool_bytes = 0


class Ops3d:
    """what models/unet_autograd.py walks with, for dim = 3: `Vol` activations on the free list, weights in their true shapes (each
    kernel gets them zero-padded to what IT needs).  The node also serves inference (no gradient requested): the 3x3x3 convolutions
    then follow `conv_precision` instead of `train_forward_precision`, and the ReLU temporary of a ResBlock travels pre-split."""

    def __init__(self, model, xin, train):
        B, _, D, H, Wd = xin.shape
        if D % 8 or H % 8 or Wd % 8:
            raise ValueError("3-D DRUNet on the HIP kernels needs depth, height and width to be multiples of 8")
        self.train = train
        # 3x3x3 convolutions in fp32 arithmetic (csrc/drunet.hip) or as bf16 split products: the training node follows
        # `train_forward_precision` (ReLU masks identical to an fp32 reference), inference follows `conv_precision`
        self.fp32 = self.fp32_ends = (getattr(model, "train_forward_precision", "fp32") if train else model.conv_precision) == "fp32"
        global _pool_sig
        if _pool_sig != (xin.device, B, D, H, Wd):       # buffers of another problem shape would never be reused: free them
            release_buffers()
            _pool_sig = (xin.device, B, D, H, Wd)
        self.lv = [Level(B, D >> i, H >> i, Wd >> i) for i in range(4)]

    @staticmethod
    def weight(name, p):
        return p

    @staticmethod
    def weight_grad(dw, shape):
        return dw

    def pack(self, x, noise_channel):
        """[B, C, D, H, W] -> slices [B (D+2), C, H, W] with zero end slices, in the activation layout"""
        lv = self.lv[0]
        B, C, D, H, Wd = x.shape
        x2 = torch.nn.functional.pad(x.detach().contiguous().float().permute(0, 2, 1, 3, 4), (0, 0, 0, 0, 0, 0, 1, 1))
        x2 = x2.reshape(B * (D + 2), C, H, Wd).contiguous()
        act = Vol(lv, C, x.device)
        if noise_channel:
            K.pack_input(lv.g, x2[:, :-1].contiguous(), x2[:, -1:].contiguous(), act.view())
        else:
            K.pack_input(lv.g, x2, 0.0, act.view())
        return act

    def unpack(self, act, channels):
        lv = self.lv[0]
        y2 = torch.empty((lv.B * (lv.D + 2), channels, lv.H, lv.W), device=act.t.device, dtype=torch.float32)
        K.unpack_output(lv.g, act.view(), channels, y2)
        return y2.view(lv.B, lv.D + 2, channels, lv.H, lv.W)[:, 1:-1].permute(0, 2, 1, 3, 4).contiguous()

    def conv3(self, i, w5, x: Vol, relu=False, res: Vol | None = None, fp32=False, flip=False, gate: Vol | None = None) -> Vol:
        """3x3x3 convolution, stride 1, zero padding 1, no bias; w5 [Cout, Cin, 3, 3, 3] (true channel counts).
        flip: convolve with the transposed, tap-reversed filter instead (the data gradient of the same layer);
        gate: the forward pass's ReLU output whose sign masks the result (ReLU backward).
        ONE launch either way (the depth taps are part of the kernel's K loop, ReLU and the zero padding slices in its
        epilogue): bf16-split arithmetic (csrc/drunet_split2d.hip) or fp32 (csrc/drunet.hip: thin head / tail layers and the
        mask-exact training forward; layers of <= 16 output channels on the 16x16x4 MFMA tile)"""
        lv = self.lv[i]
        cout, cin = (w5.shape[1], w5.shape[0]) if flip else w5.shape[:2]
        y = Vol(lv, cout, x.t.device)
        # inference: the ReLU temporary of a ResBlock (the one `relu` output; consumed only by the block's second convolution, of the
        # same channel counts) travels pre-split where the bf16-split kernels run the block; training keeps it in fp32 (the backward
        # pass reads its sign), and so does fp32 arithmetic (the fp32 kernels neither write nor read the split form)
        y.presplit = relu and not self.train and not fp32 and min(cout, cin) >= 16 and max(cout, cin) > 16
        # 16 -> 16 channels is ONE 16 x 16 x 4 MFMA tile of the fp32 thin kernel; the bf16-split kernel pads the outputs to its 64-row
        # tile (measured at config 4's level 0: 0.43 ms against 0.32 ms), so those layers take the fp32 kernel in every setting
        thin = cin <= 16 and cout <= 16
        if cin >= 16 and cout >= 16 and not fp32 and not thin:
            pk = K.cached_pack(("c3x3", flip), w5, lambda: K.pack_split3d_weight(_pad_w(_flip_t(w5) if flip else w5, _r64(cout), _r16(cin))))
            r1 = gate if gate is not None else res
            K.conv3x3x3_split(lv.g, x.view(), pk, _r16(cin), _r64(cout), y.view(), lv.D, res1=r1.view() if r1 is not None else None,
                              relu=relu, x_presplit=x.presplit, y_presplit=y.presplit, gate=gate is not None)
            return y
        assert not (x.presplit or y.presplit)
        pk, cip, cop = K.cached_pack(("c3f", flip), w5, lambda: K.pack_conv3x3x3_weight(_flip_t(w5) if flip else w5))
        if gate is not None and int(pk.shape[4]) == 16:          # thin kernel: ReLU backward in the epilogue
            assert res is None and not relu
            K.conv3x3x3(lv.g, x.view(), pk, cip, cop, y.view(), lv.D, cout_valid=cout, res1=gate.view(), gate=True)
            return y
        K.conv3x3x3(lv.g, x.view(), pk, cip, cop, y.view(), lv.D, cout_valid=cout, res1=res.view() if res is not None else None,
                    relu=relu)
        if gate is not None:
            K.relu_backward(gate.t, y.t)
        return y

    def down(self, i, w5, x: Vol, fp32=False) -> Vol:
        """2x2x2 stride-2 convolution, level i -> i + 1; w5 [Cout, Cin, 2, 2, 2].  Always bf16-split: there is no fp32 form"""
        lvi, lvo = self.lv[i], self.lv[i + 1]
        cout, cin = w5.shape[:2]
        y = Vol(lvo, cout, x.t.device)
        cop, cip = _r64(cout), _r16(cin)
        for dz in range(2):
            pk = K.cached_pack("down", w5, lambda dz=dz: K.pack_down_bf16s_weight(_pad_w(w5[:, :, dz], cop, cip)), sub=dz)
            K.down2x2_bf16s_3d(lvi.g, lvo.g, x.view(), pk, cip, cop, y.view(), lvo.D, dz, dz > 0)
        return y

    def up(self, i, w5, x: Vol, fp32=False) -> Vol:
        """2x2x2 stride-2 transposed convolution, level i + 1 -> i; w5 [Cin, Cout, 2, 2, 2].  Always bf16-split"""
        lvi, lvo = self.lv[i + 1], self.lv[i]
        cin, cout = w5.shape[:2]
        y = Vol(lvo, cout, x.t.device)
        cip, cop = _r16(cin), _r64(cout)
        for dz in range(2):
            pk = K.cached_pack("up", w5, lambda dz=dz: K.pack_up_bf16s_weight(_pad_w(w5[:, :, dz], cip, cop)), sub=dz)
            K.up2x2_bf16s_3d(lvi.g, lvo.g, x.view(), pk, cip, cop, y.view(), lvi.D, dz)
        return y

    def add(self, i, a: Vol, b: Vol) -> Vol:
        out = Vol(self.lv[i], a.key[1], a.t.device)
        ew.lincomb(1.0, a.t, 1.0, b.t, out=out.t)
        return out

    def wgrad3(self, i, gout: Vol, x: Vol, w5):
        """[Cout, Cin, 3, 3, 3] weight gradient of conv3 (S = dL/dy, L = x shifted by the depth tap)"""
        g = self.lv[i].g
        return K.conv_wgrad_3x3x3(g, gout.view(), w5.shape[0], x.view(-1), w5.shape[1], int(g.plane) * 8)

    def wgrad2(self, i, small: Vol, large: Vol, w5):
        """[m, n, 2, 2, 2] weight gradient of a 2x2x2 stride-2 layer (S on the half grid: level i + 1, L on the full grid: level i)"""
        lvs, lvl = self.lv[i + 1], self.lv[i]
        return torch.stack([K.conv_wgrad_3d(lvs.g, lvl.g, small.view(), w5.shape[0], large.view(), w5.shape[1], lvs.D, dz)
                            for dz in range(2)], dim=2)


def forward3d(model, xin):
    """DRUNet(dim=3)(xin) as one autograd node; xin = cat(volume, noise map) [B, C+1, D, H, W]"""
    return unet_autograd.forward(Ops3d, model, xin)
