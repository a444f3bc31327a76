"""Every spatial convolution path of csrc/blur.hip on the MI355X against fp64 on the CPU: the whole case table of
tests/conv_cases.py through the C entry points on guarded buffers - including what the host emulation cannot run: 256^2, 512^2
and 1024 x 96 multi-tile images and more than 65535 planes in a 3-D call - then what only hardware shows: the tiled kernel's
hand-written v_pk_fma_f32 forms (the emulation replaces them with C), an output 4 bytes off 16-byte alignment, and the same bits
while bf16 matrix-core launches run on another stream (the packed-fp32 hazard of DESIGN.md 3.6).  Then the Python layer
(deepinv_amd.physics.functional conv2d / conv_transpose2d / conv3d, Blur, Downsampling) on views, with B = 0, with deepinv-sized
filters, and under double backward."""
import math

import pytest
import torch

import conv_cases as K
from fft_cases import POISON, Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def runner():
    from deepinv_amd import hip
    from deepinv_amd.hip import conv

    return K.Runner(conv._l(), DEV, lambda: hip.stream_ptr(DEV))


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.id)
def test_conv_path(runner, case):
    errs = K.run_case(runner, case)
    print(f"{case.id}: " + ", ".join(f"{op} {e:.3g}" for op, e in errs.items()))


# ------------------------------------------------------------------ an output 4 bytes off 16-byte alignment
@pytest.mark.parametrize("d", [K.Conv2(1, 2, 68, 128, 1, 1, 5, 5, "circular"), K.Conv2(2, 1, 256, 256, 1, 1, 9, 9, "valid"),
                               K.Conv2(1, 1, 64, 64, 1, 1, 16, 16, "circular", 4)], ids=["tiled-68x128", "tiled-256-valid",
                                                                                          "strided-s4"])
def test_misaligned_output_takes_the_scalar_store(runner, d):
    """Wo % 4 == 0, so an aligned output gets 16-byte stores; at a 4-byte offset the tiled kernel must fall back to scalar stores
    (its `vec` test) and write the same bits - forward and transpose - without touching the word before or the guards after"""
    gen = torch.Generator().manual_seed(d.H + d.fh)
    Ho, Wo = K.out_size(d.H, d.fh, d.mode, d.stride), K.out_size(d.W, d.fw, d.mode, d.stride)
    assert Wo % 4 == 0
    x = runner.dev(torch.randn(d.B, d.C, d.H, d.W, generator=gen))
    k = runner.dev(torch.randn(d.fb, d.fc, d.fh, d.fw, generator=gen))
    v = runner.dev(torch.randn(d.B, d.C, Ho, Wo, generator=gen))
    for name, a, n in (("dinv_conv2d", x, d.B * d.C * Ho * Wo), ("dinv_conv2d_transpose", v, d.B * d.C * d.H * d.W)):
        aligned = Guarded(n, DEV)
        runner.run(name, d, a, k, aligned.t, None)
        off = Guarded(n + 1, DEV)
        runner.run(name, d, a, k, off.t.data_ptr() + 4, None)
        torch.cuda.synchronize()
        assert off.guards_intact(), name
        bits = off.bits()
        assert int(bits[0]) == POISON, f"{name}: wrote the word before a misaligned output"
        assert torch.equal(bits[1:], aligned.bits()), f"{name}: misaligned output differs from the aligned one"


# ------------------------------------------------------------------ the same bits beside bf16 matrix-core launches
def test_spatial_kernels_reproducible_beside_a_bf16_split_launch():
    """The tiled kernel (filter widths 5 and 7: 1 and 3 mod 4, with the odd-half v_pk_fma_f32 form) and the strided kernels on one
    stream, bf16-split convolutions (csrc/drunet_wsplit.hip) on a second: every round returns the bits of the run alone.  The
    packed-fp32 form hipcc picks for the odd half returns wrong low results in lanes 48..63 beside bf16 MFMAs;
    pk_fma_tap is written out in the clean one.  A results check: two streams, a few rounds."""
    from deepinv_amd.hip import conv as hc
    from deepinv_amd.hip import drunet as D

    gen = torch.Generator().manual_seed(7)
    x = torch.randn(8, 3, 256, 256, generator=gen).to(DEV)
    k5, k7 = torch.randn(1, 1, 5, 5, generator=gen).to(DEV), torch.randn(1, 3, 7, 7, generator=gen).to(DEV)
    k16 = torch.randn(1, 1, 16, 16, generator=gen).to(DEV)
    y4 = torch.randn(8, 3, 64, 64, generator=gen).to(DEV)
    ops = [lambda: hc.conv2d_strided(x, k5, "circular", 1), lambda: hc.conv2d_strided(x, k7, "reflect", 1),
           lambda: hc.conv2d_strided_transpose(x[..., :250, :250], k7, "valid", 1, 256, 256),
           lambda: hc.conv2d_strided_transpose(x, k5, "circular", 1, 256, 256),
           lambda: hc.conv2d_strided(x, k16, "circular", 4), lambda: hc.conv2d_strided(x, k7, "constant", 2),
           lambda: hc.conv2d_strided_transpose(y4, k16, "circular", 4, 256, 256)]
    B, side, c = 8, 128, 64
    geo = D.geom(B, side, side)

    def act(fill=True):
        a = D.alloc(geo, c, DEV)
        if fill:
            t = torch.randn(B, c, side, side, generator=gen).to(DEV)
            a[:, geo.sl:geo.sl + geo.np].view(-1, B, geo.hp, geo.wp, 8)[:, :, 1:side + 1, 1:side + 1] = \
                t.view(B, -1, 8, side, side).permute(1, 0, 3, 4, 2)
        return a

    xb, rb, yb = act(), act(), act(False)
    wws = D.pack_wsplit_weight((torch.randn(c, c, 3, 3, generator=gen) / 24).to(DEV))
    sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        alone = [op() for op in ops]
    torch.cuda.synchronize()
    alone = [a.clone() for a in alone]
    for _ in range(4):
        with torch.cuda.stream(sb):
            for _ in range(2):
                D.conv3x3_wsplit(geo, xb, wws, c, c, yb, res1=rb)
        with torch.cuda.stream(sa):
            outs = [op() for op in ops]
        with torch.cuda.stream(sb):
            for _ in range(2):
                D.conv3x3_wsplit(geo, xb, wws, c, c, yb, res1=rb)
        torch.cuda.synchronize()
        for i, (o, a) in enumerate(zip(outs, alone)):
            assert torch.equal(o, a), f"operation {i}: {int((o != a).sum())} elements differ from the run alone"


# ------------------------------------------------------------------ the Python layer
def _ratio_fwd(y, x, k, mode, s=1):
    return K.worst_ratio(y, K._ref_conv(x.cpu().double(), k.cpu().double(), mode, s),
                         K._ref_conv(x.cpu().double().abs(), k.cpu().double().abs(), mode, s))


def _ratio_adj(xt, v, k, mode, s, H, W):
    B, C = v.shape[:2]
    z = torch.zeros(B, C, H, W, dtype=torch.float64)
    ref = K._grad(lambda t: K._ref_conv(t, k.cpu().double(), mode, s) * v.cpu().double(), z)
    bnd = K._grad(lambda t: K._ref_conv(t, k.cpu().double().abs(), mode, s) * v.cpu().double().abs(), z)
    return K.worst_ratio(xt, ref, bnd)


def _offset_view(shape, seed, offset=1):
    """a contiguous view at a storage offset of `offset` floats (4 bytes off 16-byte alignment), and its CPU copy"""
    g = torch.Generator().manual_seed(seed)
    n = math.prod(shape)
    base = torch.randn(n + offset, generator=g)
    v = base.to(DEV)[offset:].view(*shape)
    assert v.is_contiguous() and v.storage_offset() == offset
    return v, base[offset:].view(*shape)


@pytest.mark.parametrize("mode", list(K.MODES))
def test_functional_conv2d_on_views(mode):
    """dF.conv2d / conv_transpose2d on a view at a 4-byte storage offset and on a transposed (non-contiguous) input: the bits of
    their contiguous copies, within the forward bound against fp64"""
    import deepinv_amd.physics.functional as dF

    x, xc = _offset_view((2, 3, 70, 66), 1)
    k = torch.randn(1, 3, 7, 6, generator=torch.Generator().manual_seed(2)).to(DEV)
    y = dF.conv2d(x, k, padding=mode)
    assert torch.equal(y, dF.conv2d(x.clone(), k, padding=mode))
    assert _ratio_fwd(y, xc, k, mode) <= K.BOUNDS["conv2d_tiled_kernel"]
    xt = x.transpose(-1, -2)
    assert not xt.is_contiguous()
    assert torch.equal(dF.conv2d(xt, k, padding=mode), dF.conv2d(xt.contiguous(), k, padding=mode))
    v, vc = _offset_view(tuple(y.shape), 3, offset=3)
    a = dF.conv_transpose2d(v, k, padding=mode)
    assert torch.equal(a, dF.conv_transpose2d(v.clone(), k, padding=mode))
    kern = K.expected_kernel(K.Conv2(2, 3, 70, 66, 1, 3, 7, 6, mode), True)
    assert _ratio_adj(a, vc, k, mode, 1, 70, 66) <= K.BOUNDS[kern]
    vt = v.transpose(-1, -2)
    assert torch.equal(dF.conv_transpose2d(vt, k, padding=mode), dF.conv_transpose2d(vt.contiguous(), k, padding=mode))


def test_conv3d_blur_downsampling_on_views():
    """conv3d / conv_transpose3d, Blur and Downsampling (bicubic x4, circular: config 5's operator) on offset and non-contiguous
    inputs give the bits of their contiguous copies"""
    import deepinv_amd as dinv
    import deepinv_amd.physics.functional as dF

    v, vc = _offset_view((1, 2, 5, 9, 70), 4)
    k3 = torch.randn(1, 2, 3, 2, 5, generator=torch.Generator().manual_seed(5)).to(DEV)
    for mode in ("circular", "valid", "reflect"):
        y = dF.conv3d(v, k3, padding=mode)
        assert torch.equal(y, dF.conv3d(v.clone(), k3, padding=mode))
        ref = K._ref_conv3(vc.double(), k3.cpu().double(), mode)
        assert K.worst_ratio(y, ref, K._ref_conv3(vc.double().abs(), k3.cpu().double().abs(), mode)) <= K.BOUNDS["conv3d_pad_kernel"]
        w, _ = _offset_view(tuple(y.shape), 6, offset=2)
        assert torch.equal(dF.conv_transpose3d(w, k3, padding=mode), dF.conv_transpose3d(w.clone(), k3, padding=mode))
        vt = v.transpose(-1, -3)
        assert torch.equal(dF.conv3d(vt, k3, padding=mode), dF.conv3d(vt.contiguous(), k3, padding=mode))
    x, xc = _offset_view((2, 3, 64, 72), 7)
    k = torch.rand(1, 1, 9, 9, generator=torch.Generator().manual_seed(8)).to(DEV)
    blur = dinv.physics.Blur(filter=k / k.sum(), padding="reflect", device=DEV)
    assert torch.equal(blur.A(x), blur.A(x.clone()))
    assert torch.equal(blur.A(x.transpose(-1, -2)), blur.A(x.transpose(-1, -2).contiguous()))
    yb, _ = _offset_view((2, 3, 64, 72), 9, offset=3)
    assert torch.equal(blur.A_adjoint(yb), blur.A_adjoint(yb.clone()))
    down = dinv.physics.Downsampling(img_size=(3, 64, 72), filter="bicubic", factor=4, padding="circular", device=DEV)
    yd = down.A(x)
    assert torch.equal(yd, down.A(x.clone()))
    assert _ratio_fwd(yd, xc, down.filter, "circular", 4) <= K.BOUNDS["conv2d_strided_kernel<true>"]
    ys, ysc = _offset_view(tuple(yd.shape), 10, offset=1)
    xa = down.A_adjoint(ys)
    assert torch.equal(xa, down.A_adjoint(ys.clone()))
    assert _ratio_adj(xa, ysc, down.filter, "circular", 4, 64, 72) <= K.BOUNDS["conv2d_strided_transpose_kernel<true>"]
    ysn = yd.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not ysn.is_contiguous()
    assert torch.equal(down.A_adjoint(ysn), down.A_adjoint(yd))


def test_empty_batch():
    """B = 0 through every operator: empty outputs of the right shape, no launch error"""
    import deepinv_amd as dinv
    import deepinv_amd.physics.functional as dF

    k = torch.rand(1, 1, 5, 5, device=DEV)
    for mode in K.MODES:
        x = torch.zeros(0, 3, 20, 24, device=DEV)
        y = dF.conv2d(x, k, padding=mode)
        assert y.shape == (0, 3, K.out_size(20, 5, mode), K.out_size(24, 5, mode))
        assert dF.conv_transpose2d(y, k, padding=mode).shape == x.shape
        v = torch.zeros(0, 2, 6, 20, 24, device=DEV)
        k3 = torch.rand(1, 1, 3, 3, 3, device=DEV)
        y3 = dF.conv3d(v, k3, padding=mode)
        assert y3.shape == (0, 2, K.out_size(6, 3, mode), K.out_size(20, 3, mode), K.out_size(24, 3, mode))
        assert dF.conv_transpose3d(y3, k3, padding=mode).shape == v.shape
    blur = dinv.physics.Blur(filter=k, padding="circular", device=DEV)
    assert blur.A(torch.zeros(0, 3, 20, 24, device=DEV)).shape == (0, 3, 20, 24)
    down = dinv.physics.Downsampling(img_size=(3, 32, 32), filter="bicubic", factor=4, padding="circular", device=DEV)
    assert down.A(torch.zeros(0, 3, 32, 32, device=DEV)).shape == (0, 3, 8, 8)
    assert down.A_adjoint(torch.zeros(0, 3, 8, 8, device=DEV)).shape == (0, 3, 32, 32)


def _motion_blur_31(seed):
    """a deepinv-sized motion-blur kernel: a smoothed random trajectory rasterised on a 31 x 31 grid, normalised"""
    g = torch.Generator().manual_seed(seed)
    steps = torch.randn(400, 2, generator=g).cumsum(0)
    steps = torch.nn.functional.avg_pool1d(steps.t()[None], 25, 1)[0].t()
    steps = steps - steps.mean(0)
    steps = steps / steps.abs().max() * 14
    k = torch.zeros(31, 31)
    idx = (steps.round().long() + 15).clamp(0, 30)
    k.index_put_((idx[:, 0], idx[:, 1]), torch.ones(len(idx)), accumulate=True)
    return (k / k.sum())[None, None]


# An image and a blur filter are both positive: the forward is then a sum of n positive terms, whose rounding errors do not cancel
# the way the signed data of the case table's do - they grow like 2^-24 sqrt(n) of the sum, not like 2^-24.  Measured on the device:
# 2.2e-6 for the 25 x 25 Gaussian (625 taps); the bound is about 4x that.  The adjoint's measurement is signed, but the replicate
# transpose folds (h / 2 + 1) (w / 2 + 1) copies of the border terms into a corner pixel, which a positive filter adds up coherently:
# 1.8e-6 for the Gaussian on the device, under the same bound.
POSITIVE_BOUND = 9e-6


@pytest.mark.parametrize("name", ["motion31", "gaussian25"])
@pytest.mark.parametrize("mode", list(K.MODES))
def test_blur_with_deepinv_sized_filters_256(name, mode):
    """Blur.A / A_adjoint at 256^2 with a 31 x 31 motion-blur and a 25 x 25 Gaussian filter, per element against fp64"""
    import deepinv_amd as dinv
    import deepinv_amd.physics.functional as dF

    k = _motion_blur_31(3) if name == "motion31" else dF.gaussian_blur(psf_size=(25, 25), sigma=(4.0, 3.0), angle=30.0)
    assert tuple(k.shape[-2:]) in ((31, 31), (25, 25))
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 3, 256, 256, generator=g)
    blur = dinv.physics.Blur(filter=k.to(DEV), padding=mode, device=DEV)
    y = blur.A(x.to(DEV))
    d = K.Conv2(2, 3, 256, 256, 1, 1, k.shape[-2], k.shape[-1], mode)
    assert K.expected_kernel(d, False) == "conv2d_tiled_kernel"
    assert _ratio_fwd(y, x, k, mode) <= POSITIVE_BOUND
    v = torch.randn(tuple(y.shape), generator=g)
    xa = blur.A_adjoint(v.to(DEV))
    assert _ratio_adj(xa, v, k, mode, 1, 256, 256) <= max(K.BOUNDS[K.expected_kernel(d, True)],
                                                          POSITIVE_BOUND if mode == "replicate" else 0)


@pytest.mark.parametrize("mode,stride", [(m, 1) for m in K.MODES] + [("circular", 4), ("reflect", 2), ("valid", 3)])
def test_double_backward_matches_fp64_autograd(mode, stride):
    """second-order autograd through _Conv / _ConvT / _FilterGrad: the gradients of a loss of conv(x, k) taken with
    create_graph=True, differentiated again with respect to x and k, against the same done in fp64 torch on the CPU"""
    from deepinv_amd.hip import conv as hc

    g = torch.Generator().manual_seed(stride * 10 + len(mode))
    x = torch.randn(2, 3, 40, 50, generator=g)
    k = torch.randn(1, 3, 7, 6, generator=g)
    w = torch.randn(*K._ref_conv(x, k, mode, stride).shape, generator=g)
    a, b = torch.randn(*x.shape, generator=g), torch.randn(*k.shape, generator=g)

    def second(conv, xx, kk, ww, aa, bb):
        y = conv(xx, kk)
        loss = (y * y * ww).sum()
        gx, gk = torch.autograd.grad(loss, (xx, kk), create_graph=True)
        return torch.autograd.grad((gx * aa).sum() + (gk * bb).sum(), (xx, kk))

    xd, kd = x.to(DEV).requires_grad_(True), k.to(DEV).requires_grad_(True)
    hx, hk = second(lambda u, q: hc.conv2d_strided(u, q, mode, stride), xd, kd, w.to(DEV), a.to(DEV), b.to(DEV))
    xr, kr = x.double().requires_grad_(True), k.double().requires_grad_(True)
    rx, rk = second(lambda u, q: K._ref_conv(u, q, mode, stride), xr, kr, w.double(), a.double(), b.double())
    for got, ref, what in ((hx, rx, "d2/dx"), (hk, rk, "d2/dk")):
        err = float((got.cpu().double() - ref).norm() / ref.norm())
        assert err < 1e-5, f"{what}: relative error {err:.3g}"
