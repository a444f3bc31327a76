"""DnCNN's bias epilogues (csrc/drunet.hip, drunet_wino4.hip, drunet_tail.hip) and bias-gradient reduction (drunet_bwd.hip) on
the host emulation, through the ctypes wrappers of deepinv_amd/hip/drunet.py, against fp64 PyTorch; then the whole model
(deepinv_amd.models.DnCNN), forward and backward, against the reference deepinv.models.DnCNN on a depth-3 net.
Each bound is about 4x the worst error measured here."""
import pytest
import torch
import torch.nn.functional as F

from emu_backend import emu_backend
from oracle.ref_shim import reference_available

needs_reference = [pytest.mark.reference, pytest.mark.skipif(not reference_available(), reason="needs the reference deepinv")]


def rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def to_act(K, g, t):
    """NCHW -> padded channel-blocked activation buffer (zero frame, zero padding channels)"""
    B, C, H, W = t.shape
    a = K.alloc(g, C, "cpu")
    av = a[:, g.sl:g.sl + g.np].view(-1, B, g.hp, g.wp, 8)
    tp = torch.zeros(B, a.shape[0] * 8, H, W)
    tp[:, :C] = t
    av[:, :, 1:H + 1, 1:W + 1] = tp.view(B, -1, 8, H, W).permute(1, 0, 3, 4, 2)
    return a


def from_act(g, a, C):
    B, H, W = g.batch, g.height, g.width
    av = a[:, g.sl:g.sl + g.np].view(-1, B, g.hp, g.wp, 8)
    return av[:, :, 1:H + 1, 1:W + 1].permute(1, 0, 4, 2, 3).reshape(B, -1, H, W)[:, :C]


def frame_is_zero(g, a):
    av = a[:, g.sl:g.sl + g.np].view(-1, g.batch, g.hp, g.wp, 8)
    return (float(av[:, :, 0].abs().max()) == 0 and float(av[:, :, g.height + 1].abs().max()) == 0
            and float(av[:, :, :, 0].abs().max()) == 0 and float(av[:, :, :, g.width + 1:].abs().max()) == 0)


def data(B, cin, cout, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, 3, 3, generator=gen) / (3.0 * cin ** 0.5)
    b = torch.randn(cout, generator=gen)
    r = torch.randn(B, cout, H, W, generator=gen)
    return x, w, b, r


@pytest.mark.parametrize("B,H,W,cin,cout,mode", [(2, 9, 13, 16, 40, "relu"), (1, 7, 5, 8, 64, "plain"), (3, 6, 11, 24, 32, "res"),
                                                 (1, 12, 8, 64, 64, "relu")])
def test_direct_bias(B, H, W, cin, cout, mode):
    """dinv_conv3x3_bias on the 32- and 64-wide cout tiles: relu(conv + b), conv + b, conv + b + res1, odd sizes"""
    from deepinv_amd.hip import drunet as K

    x, w, b, r = data(B, cin, cout, H, W, H * W + cin)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref = ref.relu() if mode == "relu" else ref + r.double() if mode == "res" else ref
    with emu_backend():
        g = K.geom(B, H, W)
        for mt in (32, 64):
            wpk, ci, co = K.pack_conv3x3_weight(w, mt=mt) if cout % 64 == 0 or mt == 32 else K.pack_conv3x3_weight(w)
            y = K.alloc(g, cout, "cpu")
            K.conv3x3_bias(g, to_act(K, g, x), wpk, K.pack_bias(b, co), ci, co, y, cout_valid=cout,
                           res1=to_act(K, g, r) if mode == "res" else None, relu=mode == "relu")
            assert rel(from_act(g, y, cout), ref) < 1.2e-6          # measured 2.8e-7
            assert frame_is_zero(g, y)


@pytest.mark.parametrize("cout,res", [(5, True), (7, False), (16, True)])
def test_thin_bias(cout, res):
    """the thin 16-wide MFMA kernel with bias (DnCNN's tail for 5-7 channels): conv + b (+ res1)"""
    from deepinv_amd.hip import drunet as K

    B, H, W, cin = 2, 10, 7, 24
    x, w, b, r = data(B, cin, cout, H, W, cout)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1) + (r.double() if res else 0)
    with emu_backend():
        g = K.geom(B, H, W)
        wt, ci = K.pack_thin_weight(w)
        y = K.alloc(g, 16, "cpu")
        K.conv3x3_bias(g, to_act(K, g, x), wt, K.pack_bias(b, 16), ci, 16, y, cout_valid=cout, res1=to_act(K, g, r) if res else None)
        assert rel(from_act(g, y, cout), ref) < 6e-7             # measured 1.5e-7
        assert float(from_act(g, y, 16)[:, cout:].abs().max() if cout < 8 else 0.0) == 0.0    # padded couts stay zero
        assert frame_is_zero(g, y)


@pytest.mark.parametrize("B,H,W,cin,cout,relu", [(2, 8, 12, 64, 64, True), (1, 16, 20, 32, 128, False), (5, 8, 8, 16, 64, True),
                                                 (20, 16, 16, 16, 128, True)])
@pytest.mark.parametrize("split", [False, True])
def test_winograd4_bias(B, H, W, cin, cout, relu, split):
    """dinv_conv3x3_winograd4_bias: the bias after the inverse transform; with a workspace the last round's tiles are cut along the
    input channels and the bias is added once, by the part that sums the partials (twice: the ticket words are reset)"""
    from deepinv_amd.hip import drunet as K

    x, w, b, _ = data(B, cin, cout, H, W, H * W + cout)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref = ref.relu() if relu else ref
    with emu_backend():
        g = K.geom(B, H, W)
        xa, wp, bp = to_act(K, g, x), K.pack_winograd4_weight(w), K.pack_bias(b, cout)
        ws = torch.zeros(K._l().dinv_conv3x3_winograd4_workspace_bytes(), dtype=torch.uint8) if split else None
        outs = []
        for _ in range(2):
            y = K.alloc(g, cout, "cpu")
            K.conv3x3_winograd4_bias(g, xa, wp, bp, cin, cout, y, relu=relu, workspace=ws)
            outs.append(y)
        f, nt = K.winograd4_last_split()
        if split:
            assert (f > 1) == (nt > 0)
        else:
            assert (f, nt) == (1, 0)
        assert torch.equal(outs[0], outs[1])
        assert rel(from_act(g, outs[0], cout), ref) < 6e-6      # measured 1.4e-6
        assert frame_is_zero(g, outs[0])


@pytest.mark.parametrize("cout,res", [(1, True), (3, True), (4, False)])
@pytest.mark.parametrize("B,H,W", [(2, 9, 13), (1, 70, 5)])
def test_tail_bias(cout, res, B, H, W):
    """dinv_conv3x3_tail_bias: y[:cout] = conv + b + res[:cout] (DnCNN's out_conv(x1) + x) on the vector-ALU tail"""
    from deepinv_amd.hip import drunet as K

    cin = 16
    x, w, b, r = data(B, cin, cout, H, W, cout + H)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1) + (r.double() if res else 0)
    with emu_backend():
        g = K.geom(B, H, W)
        y = K.alloc(g, 8, "cpu")
        K.conv3x3_tail_bias(g, to_act(K, g, x), K.pack_tail_weight(w), K.pack_bias(b, cout), cin, cout, y,
                            res=to_act(K, g, r) if res else None)
        assert rel(from_act(g, y, cout), ref) < 4e-7             # measured 8.5e-8
        assert frame_is_zero(g, y)


@pytest.mark.parametrize("B,H,W,c", [(2, 9, 13, 5), (3, 40, 37, 64), (1, 1, 1, 8)])
def test_bias_grad(B, H, W, c):
    """dinv_bias_grad: sum over the interior pixels (garbage on the frame is ignored), fixed order: bit-identical repeats,
    accumulate adds"""
    from deepinv_amd.hip import drunet as K

    gy = torch.randn(B, c, H, W, generator=torch.Generator().manual_seed(c + H))
    ref = gy.double().sum((0, 2, 3))
    with emu_backend():
        g = K.geom(B, H, W)
        a = to_act(K, g, gy)
        av = a[:, g.sl:g.sl + g.np].view(-1, B, g.hp, g.wp, 8)
        av[:, :, 0] = 1e6                                   # the frame is not part of the sum
        db = K.bias_grad(g, a, c)
        assert torch.equal(db, K.bias_grad(g, a, c))
        assert rel(db, ref) < 4e-7
        acc = torch.ones(c)
        K.bias_grad(g, a, c, db=acc, accumulate=True)
        assert torch.equal(acc, db + 1)


def _ref_net(C, nf, depth, bias, seed):
    from oracle.ref_shim import import_reference

    import_reference()
    from deepinv.models.dncnn import DnCNN

    torch.manual_seed(seed)
    den = DnCNN(C, C, depth=depth, nf=nf, bias=bias, pretrained=None, device="cpu")
    for p in den.parameters():
        if p.ndim == 1:
            torch.nn.init.uniform_(p, -0.5, 0.5)
    return den


@needs_reference[0]
@needs_reference[1]
@pytest.mark.parametrize("C,nf,H,W,bias", [(3, 64, 8, 12, True), (2, 16, 5, 7, True), (6, 8, 6, 5, True), (1, 64, 8, 8, False)])
def test_model_forward_vs_reference(C, nf, H, W, bias):
    """the whole model (head, body - Winograd where nf % 64 == 0 and H, W % 4 == 0 -, VALU or thin tail) against the reference"""
    import deepinv_amd as dinv

    ref = _ref_net(C, nf, 3, bias, C + nf)
    den = dinv.models.DnCNN(C, C, depth=3, nf=nf, bias=bias)
    den.load_state_dict(ref.state_dict(), strict=True)
    x = torch.rand(2, C, H, W, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = ref.double()(x.double())
        with emu_backend():
            got = den(x)
    assert rel(got, want) < 1.6e-6         # measured 3.9e-7


@needs_reference[0]
@needs_reference[1]
@pytest.mark.parametrize("C,nf,bias", [(2, 16, True), (3, 8, False)])
def test_model_backward_vs_reference(C, nf, bias):
    """DnCNNFunction: gradients of the input and of every weight and bias against the reference's autograd in fp64"""
    import deepinv_amd as dinv

    ref = _ref_net(C, nf, 3, bias, 7 + C).double()
    den = dinv.models.DnCNN(C, C, depth=3, nf=nf, bias=bias)
    den.load_state_dict(ref.state_dict(), strict=True)
    x = torch.rand(2, C, 6, 9, generator=torch.Generator().manual_seed(2))
    gy = torch.randn(2, C, 6, 9, generator=torch.Generator().manual_seed(3))
    xr = x.double().requires_grad_()
    ref(xr).backward(gy.double())
    xd = x.clone().requires_grad_()
    with emu_backend():
        den(xd).backward(gy)
    assert rel(xd.grad, xr.grad) < 1.3e-6          # measured (worst of all gradients) 3.1e-7
    for (n, p), (m, q) in zip(den.named_parameters(), ref.named_parameters()):
        assert n == m and rel(p.grad, q.grad) < 1.3e-6, n
