"""Every 3-D DRUNet kernel path on the MI355X against fp64 on the CPU: the whole case table of
tests/drunet3d_cases.py - dinv_conv3x3x3 (the wide fp32 kernel on both cout tiles, the thin kernel with its gate epilogue),
dinv_conv3x3x3_split (128- and 256-pixel workgroups, forced and automatic, the pre-split ResBlock pair), dinv_conv_down2x2_bf16s_3d
and dinv_conv_up2x2_bf16s_3d (each depth tap alone and both) - through the C entry points on guarded buffers with NaN in every
slack and guard plane: bit for bit on the exact data classes (`int`, `wide`), inside the derived per-element ceilings on N(0, 1) data.
Then every layer shape of the 16 / 32 / 64 / 128 network through Ops3d.conv3 / down / up in three settings (the bits of the table's
call), and what only hardware shows, for one case per kernel family: the same bits on a side stream.  `-s` prints every run's worst
fraction of its ceiling."""
import pytest
import torch

import drunet3d_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def be():
    return C.Backend(DEV)


@pytest.mark.parametrize("case,cls", C.items(emu=False), ids=C.item_id)
def test_drunet3d_case(be, case, cls):
    C.run_case(be, case, cls)


@pytest.mark.parametrize("layer,setting", C.production_items(emu=False), ids=lambda v: v if isinstance(v, str) else v[0])
def test_ops3d_launches_what_the_table_tests(be, layer, setting):
    C.run_production(be, *layer, setting)


# one case per kernel family: wide fp32, thin, the 2-D tiles, down, up
FAMILIES = [C.BY_ID[i] for i in (
    "direct-1x5x14x18-c8o128-res", "direct-1x3x14x18-c16o16-relu+res", "split-1x2x3x12-c32o128-plain-f32-n1",
    "down-2x2x7x9-c16o128-plain", "up-2x2x7x5-c64o128-x2")]


@pytest.mark.parametrize("case", FAMILIES, ids=C.item_id)
def test_same_bits_on_a_side_stream(be, case):
    """every launch of a call follows the stream it is given"""
    _, alone = C.run(be, case, "randn")
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _, got = C.run(be, case, "randn")
    torch.cuda.synchronize()
    assert torch.equal(got, alone)
