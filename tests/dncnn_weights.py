"""TEST INFRASTRUCTURE: the DnCNN weights of tests/golden/dncnn.npz, rebuilt from a seed instead of stored (make_golden_dncnn.py and
tests/test_dncnn_gpu.py both call these).  `c20_state()`: a depth-20, nf-64 colour DnCNN drawn on the CPU from a fixed torch
generator: Kaiming-normal weights (fan_in, as deepinv's weights_init_kaiming) and biases uniform in +-1/sqrt(fan_in) (PyTorch's
default); `derive()` cuts every smaller net of the golden cases out of it."""
import torch

SEED = 1


def c20_state(C=3, depth=20, nf=64, seed=SEED):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    names = ["in_conv"] + [f"conv_list.{i}" for i in range(depth - 2)] + ["out_conv"]
    for i, name in enumerate(names):
        cin = C if i == 0 else nf
        cout = C if i == len(names) - 1 else nf
        fan_in = 9 * cin
        sd[f"{name}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / fan_in) ** 0.5
        sd[f"{name}.bias"] = (torch.rand(cout, generator=g) * 2 - 1) / fan_in ** 0.5
    return sd


def derive(sd, C, depth, nf, bias=True):
    """state dict of DnCNN(C, C, depth, bias, nf) cut out of the depth-20 colour weights: in_conv [:nf, :C], conv_list.i
    [:nf, :nf], out_conv [:C, :nf] (biases likewise)"""
    out = {"in_conv.weight": sd["in_conv.weight"][:nf, :C]}
    for i in range(depth - 2):
        out[f"conv_list.{i}.weight"] = sd[f"conv_list.{i}.weight"][:nf, :nf]
    out["out_conv.weight"] = sd["out_conv.weight"][:C, :nf]
    if bias:
        out["in_conv.bias"] = sd["in_conv.bias"][:nf]
        for i in range(depth - 2):
            out[f"conv_list.{i}.bias"] = sd[f"conv_list.{i}.bias"][:nf]
        out["out_conv.bias"] = sd["out_conv.bias"][:C]
    return {k: v.clone() for k, v in out.items()}


# gradients with more elements than this are stored as every GRAD_STRIDE-th element plus the norm of the whole tensor
GRAD_FULL_MAX = 4096
GRAD_STRIDE = 7


def grad_sample(t):
    flat = t.detach().reshape(-1)
    return flat if flat.numel() <= GRAD_FULL_MAX else flat[::GRAD_STRIDE]
