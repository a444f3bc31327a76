"""DnCNN (deepinv_amd.models.DnCNN) without a device: the architectures the HIP kernels do not cover raise at construction,
`pretrained` handling, the reference's parameter names and initialisation, and the CPU-tensor error."""
import pytest
import torch

import deepinv_amd as dinv
from deepinv_amd.hip import HipExtensionError


@pytest.mark.parametrize("kw, what", [({"dim": 3}, "dim=3"), ({"in_channels": 2, "out_channels": 1}, "in_channels must equal"),
                                      ({"in_channels": 8, "out_channels": 8}, "1..7"), ({"depth": 1}, "depth >= 2")])
def test_unsupported_architectures_raise(kw, what):
    with pytest.raises(NotImplementedError, match=what.replace(".", r"\.").replace("(", r"\(")):
        dinv.models.DnCNN(**kw)


def test_download_raises():
    for name in ("download", "download_lipschitz"):
        with pytest.raises(RuntimeError, match="no network access"):
            dinv.models.DnCNN(pretrained=name)


def test_pretrained_path_loads_strictly(tmp_path):
    a = dinv.models.DnCNN(1, 1, depth=4, nf=16)
    path = tmp_path / "w.pth"
    torch.save(a.state_dict(), path)
    b = dinv.models.DnCNN(1, 1, depth=4, nf=16, pretrained=str(path))
    assert not b.training
    for (n, p), (m, q) in zip(a.state_dict().items(), b.state_dict().items()):
        assert n == m and torch.equal(p, q)
    with pytest.raises(RuntimeError):
        dinv.models.DnCNN(1, 1, depth=5, nf=16, pretrained=str(path))        # strict: a missing layer is an error


def test_parameter_names_and_init():
    torch.manual_seed(0)
    m = dinv.models.DnCNN(2, 2, depth=7)
    keys = list(m.state_dict())
    assert keys[:2] == ["in_conv.weight", "in_conv.bias"] and keys[-2:] == ["out_conv.weight", "out_conv.bias"]
    assert [k for k in keys if k.startswith("conv_list")] == [f"conv_list.{i}.{t}" for i in range(5) for t in ("weight", "bias")]
    w = m.conv_list[0].weight
    assert abs(float(w.detach().std()) - (2.0 / (64 * 9)) ** 0.5) < 0.1 * (2.0 / (64 * 9)) ** 0.5    # Kaiming normal, fan_in
    assert set(dinv.models.DnCNN(bias=False).state_dict()) == {"in_conv.weight", "out_conv.weight"} | {
        f"conv_list.{i}.weight" for i in range(18)}


def test_cpu_tensor_raises():
    m = dinv.models.DnCNN(1, 1, depth=3, nf=8)
    with pytest.raises(HipExtensionError):
        m(torch.rand(1, 1, 8, 8))
