"""Every training kernel path on the MI355X against fp64 on the CPU: the whole case table of tests/bwd_cases.py -
the weight gradients, the bias gradient and the ReLU backward of csrc/drunet_bwd.hip through the C entry points on guarded buffers,
the data gradients through the calls training makes - bit for bit on the exact data classes (`int`, `wide`) and inside the derived
ceilings on N(0, 1) data.  This is where the real v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32 write-back, the hand-written
s_waitcnt of wgrad_kernel and the 16-byte LDS staging of wgrad_lds_kernel are checked (the host emulation builds its MFMA from the
documented fragment layout).  Then what only hardware shows: the same bits on a side stream, and the same bits while bf16-split
convolutions run on a second stream (the hazard of DESIGN.md 3.6).  `-s` prints every randn run's worst fraction of its ceiling."""
import pytest
import torch

import bwd_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def be():
    return C.Backend(DEV)


@pytest.mark.parametrize("case,cls", C.items(emu=False), ids=C.item_id)
def test_bwd_case(be, case, cls):
    C.run_case(be, case, cls)


# one weight-gradient case per kernel form: wgrad_lds_kernel<16> / <32>, wgrad_kernel<4, true, 16> / <4, true, 32>, the 3x3x3 one-call
# form (grid.y = depth tap) and the 2x2x2 depth pairing
_BY_ID = {c.id: c for c in C.CASES}
FORMS = [_BY_ID[i] for i in ("w3-1x94x90-m16n16", "w3-2x30x29-m24n40", "w2-down-2x30x30-m16n16", "w2-up-2x30x29-m24n40",
                             "w333-1x3x14x12-m16n16", "w222-down-1x4x30x30-m16n16")]


@pytest.mark.parametrize("case", FORMS, ids=C.item_id)
def test_wgrad_same_bits_on_a_side_stream(be, case):
    """the launch and its reduction follow the stream they are given: bits equal to the default-stream run"""
    _, alone = C.run_wgrad(be, case, "randn")
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _, got = C.run_wgrad(be, case, "randn")
    torch.cuda.synchronize()
    assert torch.equal(got, alone)


@pytest.mark.parametrize("case", FORMS, ids=C.item_id)
def test_wgrad_reproducible_beside_a_bf16_split_launch(be, case):
    """the weight gradient on one stream, bf16-split convolutions (csrc/drunet_split2d.hip) on a second: every round returns the bits
    of the run alone (fp32 work beside bf16 MFMA waves of another kernel).  A results check: two streams, a few rounds."""
    K = be.K
    _, alone = C.run_wgrad(be, case, "randn")
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
            _, got = C.run_wgrad(be, case, "randn", beside=beside)
        torch.cuda.synchronize()
        assert torch.equal(got, alone)
