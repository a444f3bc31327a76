"""Launch traces of the DRUNet / DnCNN host layer, without a GPU: the library entry points the Python layer calls, in order, with
their scalar arguments and their buffer wiring, against tests/golden/unet_launch_traces.json (recorded once by
tests/golden/make_unet_launch_traces.py, before the U-Net walk, the conv packs and the profiling bracket were single-sourced).

The library handle of hip/drunet.py and hip/elementwise.py is replaced by a recorder: geometry and ``*_bytes`` queries go to the
built library (it loads on a GPU-less host, tests/test_abi.py), every other entry point is noted and returns success.  Tensors
handed to ``ptr`` are kept alive and numbered by first appearance of their address, so the numbering is canonical and a buffer
number that comes back means the SAME memory was handed out again (the recycled ``Vol`` buffers of models/drunet3d.py: a reference
held one layer longer shows up as another number).

Also here: SHA-256 of the bytes of every bf16-split weight pack of one fixed weight."""
import functools
import hashlib
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_launch_traces.json")


class _Recorder:
    def __init__(self, real, launches):
        self._real, self._launches = real, launches

    def __getattr__(self, name):
        if name == "dinv_act_geom_init" or name.endswith("_bytes"):
            return getattr(self._real, name)

        def launch(*args):
            self._launches.append([name, [_plain(a) for a in args]])
            return 0

        return launch


def _plain(a):
    """argument of a launch as JSON: buffers are ["buf", n] (set by the `ptr` stand-in), a geometry its fields"""
    if a is None or isinstance(a, (bool, int, float, str, list)):
        return a
    if hasattr(a, "_obj"):                  # ctypes.byref(ActGeom)
        g = a._obj
        return ["geom", g.batch, g.height, g.width, int(g.cs)]
    raise TypeError(f"unexpected launch argument {a!r}")


def record(run):
    """the launches of run() as [[symbol, [arguments]], ...]"""
    from deepinv_amd.hip import drunet as K
    from deepinv_amd.hip import elementwise as ew
    from deepinv_amd.models import drunet3d

    real = (K._l(), ew._l())[0]             # declares the argument types of the queries that stay real
    launches, alive, numbers = [], [], {}

    def ptr(t):
        if t is None:
            return None
        alive.append(t)
        return ["buf", numbers.setdefault(t.data_ptr(), len(numbers))]

    saved = [(m, n, getattr(m, n)) for m in (K, ew) for n in ("_l", "ptr", "stream_ptr")]
    workspaces = dict(K._W4_WS)             # (another test may have left the workspace of another library build there)
    K._W4_WS.clear()
    K.clear_pack_cache()
    drunet3d.release_buffers()
    try:
        for m in (K, ew):
            m._l = lambda: _Recorder(real, launches)
            m.ptr = ptr
            m.stream_ptr = lambda device: None
        run()
    finally:
        for m, n, v in saved:
            setattr(m, n, v)
        K._W4_WS.clear()
        K._W4_WS.update(workspaces)
        K.clear_pack_cache()
        drunet3d.release_buffers()
    return launches


def _xin(*shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(1)).requires_grad_(True)


def _train2d():
    import deepinv_amd as dinv
    from deepinv_amd.models import drunet_train

    model = dinv.models.DRUNet(2, 2, nc=(24, 48, 96, 160), nb=2, pretrained=None)
    return lambda: drunet_train.forward_train(model, _xin(1, 3, 32, 40)).sum().backward()


def _model3d():
    import deepinv_amd as dinv

    return dinv.models.DRUNet(2, 2, nc=(16, 32, 64, 128), nb=1, dim=3, pretrained=None)


def _train3d():
    from deepinv_amd.models import drunet3d

    model = _model3d()
    return lambda: drunet3d.forward3d(model, _xin(1, 3, 8, 16, 16)).sum().backward()


def _infer3d():
    from deepinv_amd.models import drunet3d

    model = _model3d()

    def run():
        with torch.no_grad():
            drunet3d.forward3d(model, _xin(1, 3, 8, 16, 16).detach())
    return run


def _infer3d_presplit():
    """frozen weights (nothing asks for a gradient, so the node saves nothing), bf16-split kernels, two blocks per stage: the ReLU
    temporary of every ResBlock from 32 channels up travels pre-split, and each stage recycles the buffers of its first block"""
    import deepinv_amd as dinv
    from deepinv_amd.models import drunet3d

    model = dinv.models.DRUNet(2, 2, nc=(16, 32, 64, 128), nb=2, dim=3, pretrained=None).requires_grad_(False)
    model.conv_precision = "bf16split"

    def run():
        with torch.no_grad():
            drunet3d.forward3d(model, _xin(1, 3, 8, 16, 16).detach())
    return run


def _infer2d(precision, shape=(1, 2, 32, 40), **lane):
    """`lane`: the keywords a batch lane passes to `_hip_forward_lane` (lane, out, tail_split)"""
    import deepinv_amd as dinv

    model = dinv.models.DRUNet(2, 2, pretrained=None)
    model.conv_precision = precision

    def run():
        with torch.no_grad():
            model._hip_forward_lane(_xin(*shape).detach(), 0.1, **lane)
    return run


# 8 x 128 x 128: 256 x 1, 64 x 2, 16 x 4 and 4 x 8 workgroup tiles (32 tile positions x 64 couts) at the four levels - every ResBlock
# convolution reaches the F(4x4) kernel (WINOGRAD4_MIN_TILES = 32), and level 0 alone has as many tiles as the 256 compute units
# that `_compute_units` answers for a CPU device
WINO4_SHAPE = (8, 2, 128, 128)


def _dncnn(train, shape=(1, 2, 16, 16), **arch):
    import deepinv_amd as dinv
    from deepinv_amd.models import dncnn

    model = dinv.models.DnCNN(shape[1], shape[1], pretrained=None, **{"depth": 5, "nf": 64, **arch})
    if train:
        return lambda: dncnn.DnCNNFunction.apply(model, _xin(*shape), *model.parameters()).sum().backward()

    def run():
        with torch.no_grad():
            model._hip_forward(_xin(*shape).detach())
    return run


CASES = {
    "train2d": _train2d,
    "train3d": _train3d,
    "infer3d": _infer3d,
    "infer3d_presplit": _infer3d_presplit,
    "infer2d": lambda: _infer2d("fp32"),
    "infer2d_split": lambda: _infer2d("bf16split"),
    "dncnn_infer": lambda: _dncnn(False),
    "dncnn_train": lambda: _dncnn(True),
    "infer2d_wino4": lambda: _infer2d("fp32", WINO4_SHAPE),
    "infer2d_wino4_lane": lambda: _infer2d("fp32", WINO4_SHAPE, tail_split=False),
    "infer2d_lane1": lambda: _infer2d("fp32", lane=1, out=torch.empty(1, 2, 32, 40)),
    "dncnn_infer_nobias": lambda: _dncnn(False, bias=False),
    "dncnn_infer_thin": lambda: _dncnn(False, (1, 5, 16, 20), depth=4, nf=32),
}


@functools.lru_cache(maxsize=None)
def trace(case):
    torch.manual_seed(0)
    return record(CASES[case]())


@pytest.mark.parametrize("case", list(CASES))
def test_launch_trace_matches_golden(case):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got = json.loads(json.dumps(trace(case)))
    assert len(got) > 0, "no launch recorded"
    assert [l[0] for l in got] == [l[0] for l in want], "another sequence of entry points"
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"launch {i}: {a} != {b}"


def _wino4_workspaces(case):
    """{image height: [workspace argument, ...]} of the F(4x4) launches of a case"""
    by_level = {}
    for name, args in trace(case):
        if name == "dinv_conv3x3_winograd4":
            assert (args[8] is None) == (args[9] == 0)
            by_level.setdefault(args[0][2], []).append(args[8])
    return by_level


def test_wino4_cases_reach_the_kernel_and_the_tail_split_rule():
    """what the two 8 x 128 x 128 cases are there to pin: all 56 ResBlock convolutions run on the F(4x4) kernel; with the tail split
    every launch has the workspace, without it (a batch lane) only the launches of fewer tiles than compute units: level 0 has 256
    tiles on 256 units and gets none, levels 1 to 3 have 128, 64 and 32 and keep it"""
    whole, lane = _wino4_workspaces("infer2d_wino4"), _wino4_workspaces("infer2d_wino4_lane")
    for by_level in (whole, lane):
        assert {h: len(v) for h, v in by_level.items()} == {128: 16, 64: 16, 32: 16, 16: 8}
    assert all(w is not None for v in whole.values() for w in v)
    assert all(w is None for w in lane[128])
    assert all(w is not None for h in (64, 32, 16) for w in lane[h])


def test_forward_writes_no_model_state():
    """the launch policy of a call travels as an argument: a forward call leaves no attribute on the model but the engine cache"""
    import deepinv_amd as dinv

    assert not hasattr(dinv.models.DRUNet, "_tail_split")
    drunet = dinv.models.DRUNet(2, 2, nc=(16, 32, 64, 64), nb=1, pretrained=None)
    dncnn = dinv.models.DnCNN(2, 2, depth=3, nf=64, pretrained=None)
    x = _xin(1, 2, 32, 32).detach()
    for model, run in ((drunet, lambda: drunet._hip_forward_lane(x, 0.1, lane=1, tail_split=False)), (dncnn, lambda: dncnn._hip_forward(x))):
        before = set(vars(model))
        with torch.no_grad():
            assert len(record(run)) > 0
        assert set(vars(model)) - before <= {"_engine"} and before <= set(vars(model))
        assert not hasattr(model, "_tail_split")


# ---- packs: bytes of every bf16-split pack of one fixed weight
def _weight(*shape):
    """fixed fp32 values in (-0.5, 0.5) from integer arithmetic (no random generator involved)"""
    n = 1
    for s in shape:
        n *= s
    v = (torch.arange(n, dtype=torch.int64) * 2654435761 + 12345) % (1 << 32)
    return (v.double() / float(1 << 32) - 0.5).float().reshape(shape)


PACKS = {
    "pack_split2d_weight": ((64, 32, 3, 3), "a2a45bf9c0e628ec7d7a5756f60c3f9f040bd9fc1b6d9915944871f24bf6700f"),
    "pack_wsplit_weight": ((64, 32, 3, 3), "ffc888c724b4542ea3c04411e4b02e5377d7696274e94904c291f6e2e6368c8c"),
    "pack_split3d_weight": ((64, 32, 3, 3, 3), "89e7ee0fcbb1f3ec88abdb092a53076f78dc67edcf10635663cf64afba9384d6"),
    "pack_winograd4_bf16x3_weight": ((64, 32, 3, 3), "3a9de9cbffab9547999583cc3a677df236ad4f560419ee3c4d2d0c0133e9a8fc"),
    "pack_down_bf16s_weight": ((64, 32, 2, 2), "df35e37707f0ddbe65838b9c906c096bdaeaa9c6a7aa4b673f8346bb35dc1bfb"),
    "pack_down_bf16x3_weight": ((64, 32, 2, 2), "8631d73667acd54410f2c79866a7cc59cdbd9a31f34f616942aed0c96f61fb25"),
    "pack_up_bf16s_weight": ((32, 64, 2, 2), "3ef938d31fcb7b1cc9c88fee71b9f352f5162c80f01ba6e3047fe6bc08fda536"),
}


def pack_hash(name):
    from deepinv_amd.hip import drunet as K

    packed = getattr(K, name)(_weight(*PACKS[name][0]))
    assert packed.dtype == torch.bfloat16 and packed.is_contiguous()
    return hashlib.sha256(packed.view(torch.uint8).numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("name", list(PACKS))
def test_pack_bytes(name):
    assert pack_hash(name) == PACKS[name][1]
