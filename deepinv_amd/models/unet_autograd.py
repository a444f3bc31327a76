"""The DRUNet forward + backward walk, once, for the 2-D and the 3-D kernels (deepinv/models/drunet.py:39-263 differentiated by hand).

``UNetFunction`` is ONE ``torch.autograd.Function`` for the whole network: head, three (ResBlocks + stride-2 conv) stages, body,
three (skip add + transposed conv + ResBlocks) stages, tail - and the mirror image on the way back.  What a convolution, an add, a
weight gradient or a packed activation IS comes from an ops object built per call: ``drunet_train.Ops2d`` (activation tensors,
weights zero-padded to multiples of 64 up front) or ``drunet3d.Ops3d`` (``Vol`` buffers on a free list, true weight shapes).  An
ops class has

    Ops(model, xin, train)                  per call; .fp32 / .fp32_ends: fp32 arithmetic in the forward ResBlock, stride-2 and
                                            transposed convolutions / in the head and tail convolutions
    weight(name, p), weight_grad(dw, shape) a parameter as the ops use it, and its gradient back in the parameter's shape
    pack(x, noise_channel), unpack(act, c)  [B, C, ...] tensor <-> level-0 activation (noise_channel: the last channel is the noise map)
    conv3(i, w, x, relu, res, fp32, flip, gate)      3x3(x3) convolution on level i; flip: the data gradient of the layer
    down(i, w, x, fp32), up(i, w, x, fp32)  level i -> i + 1 / level i + 1 -> i (each is the data gradient of the other)
    add(i, a, b)
    wgrad3(i, gout, x, w), wgrad2(i, small, large, w)         weight gradients of conv3 / of a stride-2 layer between levels i + 1, i

The order of the layers, what is kept for the backward pass, when a weight gradient is taken and where the skip gradients are
added is decided here and nowhere else.  Activations are released by reference counting (``Vol.__del__`` recycles the buffer), so
the local names below are part of the memory footprint: nothing is held longer than the walk needs it."""
from __future__ import annotations

import torch


def _r64(c):
    return (c + 63) // 64 * 64


def _r16(c):
    return (c + 15) // 16 * 16


def _pad_w(w, d0, d1):
    if w.shape[0] == d0 and w.shape[1] == d1:
        return w
    out = torch.zeros((d0, d1, *w.shape[2:]), device=w.device, dtype=torch.float32)
    out[:w.shape[0], :w.shape[1]] = w
    return out


def _flip_t(w):
    """filter of the data-gradient convolution: [Cout, Cin, *k] -> [Cin, Cout, *k], taps reversed"""
    return w.flip(*range(2, w.ndim)).transpose(0, 1).contiguous()


def _blk(model, prefix, k):
    """parameter-name prefix of ResBlock k of a stage (with nb = 1 the body is a bare ResBlock: 'm_body', not 'm_body.0')"""
    return prefix if (prefix == "m_body" and model.nb == 1) else f"{prefix}.{k}"


class UNetFunction(torch.autograd.Function):
    """``y = DRUNet(xin)`` with ``xin = cat(image, noise map)``; parameters are passed explicitly (named_parameters order)"""

    @staticmethod
    def forward(ctx, Ops, model, xin, *params):
        names = [n for n, _ in model.named_parameters()]
        nb = model.nb
        train = any(ctx.needs_input_grad[2:])
        ops = Ops(model, xin, train)
        f32 = ops.fp32
        W = {n: ops.weight(n, p.detach().float()) for n, p in zip(names, params)}
        x_act = ops.pack(xin, True)
        saved = {"x_act": x_act, "res": {}, "down_in": {}, "up_in": {}}

        def res_chain(i, prefix, first, cur):
            for k in range(first, first + nb):
                a1 = ops.conv3(i, W[f"{_blk(model, prefix, k)}.res.0.weight"], cur, relu=True, fp32=f32)
                out = ops.conv3(i, W[f"{_blk(model, prefix, k)}.res.2.weight"], a1, res=cur, fp32=f32)
                if train:
                    saved["res"][f"{prefix}.{k}"] = (cur, a1)
                cur = out
            return cur

        x1 = ops.conv3(0, W["m_head.weight"], x_act, fp32=ops.fp32_ends)
        skips = [x1]
        cur = x1
        for i, name in enumerate(("m_down1", "m_down2", "m_down3")):
            r = res_chain(i, name, 0, cur)
            saved["down_in"][name] = r
            cur = ops.down(i, W[f"{name}.{nb}.weight"], r, fp32=f32)
            skips.append(cur)
        cur = res_chain(3, "m_body", 0, cur)
        for i, name in zip((2, 1, 0), ("m_up3", "m_up2", "m_up1")):
            s = ops.add(i + 1, cur, skips[i + 1])
            saved["up_in"][name] = s
            cur = ops.up(i, W[f"{name}.0.weight"], s, fp32=f32)
            cur = res_chain(i, name, 1, cur)
        s0 = ops.add(0, cur, x1)
        saved["tail_in"] = s0
        y_act = ops.conv3(0, W["m_tail.weight"], s0, fp32=ops.fp32_ends)
        y = ops.unpack(y_act, model.out_channels)
        if train:
            ctx.ops, ctx.model, ctx.names, ctx.W, ctx.saved = ops, model, names, W, saved
            ctx.shapes = {n: tuple(p.shape) for n, p in zip(names, params)}
            ctx.in_channels = xin.shape[1]
        return y

    @staticmethod
    def backward(ctx, gy):
        ops, model, names, W, saved = ctx.ops, ctx.model, ctx.names, ctx.W, ctx.saved
        nb = model.nb
        want_w = any(ctx.needs_input_grad[3:])
        dW = {}

        def wgrad3(name, i, gout, x):
            if want_w:
                dW[name] = ops.weight_grad(ops.wgrad3(i, gout, x, W[name]), ctx.shapes[name])

        def wgrad2(name, i, small, large):
            if want_w:
                dW[name] = ops.weight_grad(ops.wgrad2(i, small, large, W[name]), ctx.shapes[name])

        def res_back(i, prefix, first, gout):
            for k in range(first + nb - 1, first - 1, -1):
                x_in, a1 = saved["res"][f"{prefix}.{k}"]
                n1, n2 = f"{_blk(model, prefix, k)}.res.0.weight", f"{_blk(model, prefix, k)}.res.2.weight"
                wgrad3(n2, i, gout, a1)
                gt = ops.conv3(i, W[n2], gout, flip=True, gate=a1)      # ReLU backward in the epilogue (gate = the forward activation)
                wgrad3(n1, i, gt, x_in)
                gout = ops.conv3(i, W[n1], gt, res=gout, flip=True)
            return gout

        gy_act = ops.pack(gy, False)
        wgrad3("m_tail.weight", 0, gy_act, saved["tail_in"])
        gcur = ops.conv3(0, W["m_tail.weight"], gy_act, flip=True)
        gskip = {0: gcur}                     # s0 = u0 + x1
        for i, name in zip((0, 1, 2), ("m_up1", "m_up2", "m_up3")):
            gcur = res_back(i, name, 1, gcur)
            wgrad2(f"{name}.0.weight", i, saved["up_in"][name], gcur)       # [Cin (level i + 1), Cout (level i), 2, 2(, 2)]
            gcur = ops.down(i, W[f"{name}.0.weight"], gcur)     # d/ds of convT(s, wu) = conv_s2 with the same filter
            gskip[i + 1] = gcur               # s_{i+1} = (level i+1 result) + x_{i+2}
        gcur = ops.add(3, res_back(3, "m_body", 0, gcur), gskip[3])
        for i, name in zip((2, 1, 0), ("m_down3", "m_down2", "m_down1")):
            wgrad2(f"{name}.{nb}.weight", i, gcur, saved["down_in"][name])  # [Cout (level i + 1), Cin (level i), 2, 2(, 2)]
            gcur = ops.up(i, W[f"{name}.{nb}.weight"], gcur)    # d/dr of conv_s2(r, wd) = convT with the same filter
            gcur = ops.add(i, res_back(i, name, 0, gcur), gskip[i])
        wgrad3("m_head.weight", 0, gcur, saved["x_act"])
        gx = None
        if ctx.needs_input_grad[2]:
            gx = ops.unpack(ops.conv3(0, W["m_head.weight"], gcur, flip=True), ctx.in_channels)
        ctx.saved = None                      # free the activations
        grads = [dW.get(n) if need else None for n, need in zip(names, ctx.needs_input_grad[3:])]
        return (None, None, gx, *grads)


def forward(Ops, model, xin):
    """DRUNet(xin) recorded as one autograd node (all parameters of `model` are inputs of the node)"""
    return UNetFunction.apply(Ops, model, xin, *[p for _, p in model.named_parameters()])
