"""Every DRUNet / DnCNN inference kernel path on the MI355X against fp64 on the CPU: the whole case table of
tests/drunet_fwd_cases.py - pack / unpack, the direct fp32 convolution (both cout tiles, the thin form, the bias epilogues), Winograd
F(2x2) and F(4x4) (fp32 and bf16x3, every tail-split regime of the 32-compute-unit XCD), the bf16-split 2-D tiles (128- and
256-pixel workgroups, forced and automatic) and F(2,3), the stride-2 layers in fp32 / two-part / three-part form, the tail in its
lane-shift and flat kernels - through the C entry points on guarded buffers with NaN in every slack: bit for bit on the exact data
classes (`int`, `wide`), inside the derived per-element ceilings on N(0, 1) data.  Then what only hardware shows, for one case per
kernel family: the same bits on a side stream, and - the fp32 families - the same bits while bf16-split convolutions run on a second
stream (the hazard of DESIGN.md 3.6).  `-s` prints every run's worst fraction of its ceiling."""
import pytest
import torch

import drunet_fwd_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def be():
    return C.Backend(DEV)


@pytest.mark.parametrize("case,cls", C.items(emu=False), ids=C.item_id)
def test_drunet_fwd_case(be, case, cls):
    C.run_case(be, case, cls)


# one case per kernel family; FP32: the families that run on the fp32 pipes (vector ALU / fp32 MFMA)
FAMILIES = [C.BY_ID[i] for i in (
    "direct-1x46x42-c8o128-t64-res+res2", "direct-1x46x42-c8o16-t16-relu", "wino2-1x37x51-c32o64-res", "wino4-5x8x8-c64o64-relu-ws",
    "wino4x3-1x20x36-c16o64-relu", "split-1x17x33-c32o128-res-f32-n1", "wsplit-3x9x32-c16o128-res", "down-1x46x42-c24o64-plain",
    "down_bf16s-1x46x42-c16o128-plain", "down_bf16x3-2x5x6-c32o128-plain", "up-1x46x42-c24o64-x2", "up_bf16s-1x6x14-c64o128-x2",
    "tail-2x9x21-c64o3-x2")]
FP32 = [c for c in FAMILIES if c.kind in ("direct", "wino2", "wino4", "down", "up", "tail")]


@pytest.mark.parametrize("case", FAMILIES, ids=C.item_id)
def test_same_bits_on_a_side_stream(be, case):
    """every launch of a call (the tail-split launch of F(4x4) and its workspace included) follows the stream it is given"""
    _, alone = C.run_conv(be, case, "randn")
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _, got = C.run_conv(be, case, "randn")
    torch.cuda.synchronize()
    assert torch.equal(got, alone)


@pytest.mark.parametrize("case", FP32, ids=C.item_id)
def test_reproducible_beside_a_bf16_split_launch(be, case):
    """an fp32 kernel on one stream, bf16-split convolutions (csrc/drunet_split2d.hip) on a second: every round returns the bits of
    the run alone (fp32 work beside bf16 MFMA waves of another kernel).  A results check: two streams, three rounds."""
    K = be.K
    _, alone = C.run_conv(be, case, "randn")
    B, side, c = 4, 128, 64
    geo = K.geom(B, side, side)
    gen = torch.Generator().manual_seed(5)
    xb = be.dev(C.to_buf(geo, torch.randn(B, c, side, side, generator=gen)))
    yb = K.alloc(geo, c, DEV)
    wsp = be.dev(K.pack_split2d_weight(torch.randn(c, c, 3, 3, generator=gen) / 24))
    sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)

    def beside():
        with torch.cuda.stream(sb):
            for _ in range(3):
                K.conv3x3_split(geo, xb, wsp, c, c, yb)

    torch.cuda.synchronize()
    for _ in range(3):
        with torch.cuda.stream(sa):
            _, got = C.run_conv(be, case, "randn", beside=beside)
        torch.cuda.synchronize()
        assert torch.equal(got, alone)
