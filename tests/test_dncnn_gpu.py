"""DnCNN (deepinv_amd.models.DnCNN, csrc/drunet*.hip bias epilogues) on the GPU: the reference golden vectors
(tests/golden/dncnn.npz from make_golden_dncnn.py; the weights are rebuilt from their seed by tests/dncnn_weights.py), the
full-size colour net against an fp64 CPU restatement, bit-identical repeat calls, state_dict compatibility, a graph-captured PnP
loop, and training through unfolded_builder."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dncnn_weights import c20_state, derive, grad_sample

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(G, "dncnn.npz"))
    return {k: torch.from_numpy(d[k]) for k in d.files}


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def net(gold, dev, C=3, depth=20, nf=64, bias=True):
    import deepinv_amd as dinv

    den = dinv.models.DnCNN(C, C, depth=depth, bias=bias, nf=nf)
    den.load_state_dict(derive(c20_state(), C, depth, nf, bias), strict=True)
    return den.to(dev).eval()


def ref64(sd, x, depth):
    """fp64 restatement of deepinv/models/dncnn.py forward"""
    p = {k: v.double() for k, v in sd.items()}
    x1 = F.relu(F.conv2d(x, p["in_conv.weight"], p.get("in_conv.bias"), padding=1))
    for i in range(depth - 2):
        x1 = F.relu(F.conv2d(x1, p[f"conv_list.{i}.weight"], p.get(f"conv_list.{i}.bias"), padding=1))
    return F.conv2d(x1, p["out_conv.weight"], p.get("out_conv.bias"), padding=1) + x


CASES = {"c20_even": (3, 20, 64, True), "c20_odd": (3, 20, 64, True), "gray": (1, 5, 64, True), "nobias": (3, 5, 64, False),
         "nf48": (3, 5, 48, True), "nf8": (3, 3, 8, True), "ch2": (2, 7, 64, True)}


@pytest.mark.parametrize("tag", sorted(CASES))
def test_golden(gold, dev, tag):
    C, depth, nf, bias = CASES[tag]
    den = net(gold, dev, C, depth, nf, bias)
    with torch.no_grad():
        y = den(gold[f"{tag}_x"].to(dev))
    exact = ref64(derive(c20_state(), C, depth, nf, bias), gold[f"{tag}_x"].double(), depth)
    e_ref = rel_err(gold[f"{tag}_y"], exact)
    assert rel_err(y, exact) < TOL
    assert rel_err(y, gold[f"{tag}_y"]) < max(TOL, 2.0 * e_ref)


def test_full_size_fp64(gold, dev):
    """[4,3,128,128], depth 20: every body layer on the Winograd kernel with bias, tail split included"""
    den = net(gold, dev)
    x = torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        y = den(x.to(dev))
    e = rel_err(y, ref64(c20_state(), x.double(), 20))
    print("DnCNN [4,3,128,128] vs fp64:", f"{e:.2e}")
    assert e < 2e-5


@pytest.mark.parametrize("shape", [(2, 3, 37, 53), (1, 3, 30, 34), (3, 3, 17, 9)])
def test_direct_fallback_shapes(gold, dev, shape):
    """H or W not a multiple of 4: the body runs on the direct kernel with bias"""
    den = net(gold, dev, depth=6)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        y = den(x.to(dev))
    assert rel_err(y, ref64(derive(c20_state(), 3, 6, 64), x.double(), 6)) < TOL


@pytest.mark.parametrize("C", [4, 5, 7])
def test_tail_channels(dev, C):
    """4 channels on the VALU tail, 5 and 7 on the thin MFMA tail; nf = 40 (direct body), with and without bias"""
    import deepinv_amd as dinv

    for bias in (True, False):
        torch.manual_seed(C)
        den = dinv.models.DnCNN(C, C, depth=4, nf=40, bias=bias).to(dev).eval()
        for p in den.parameters():
            if p.ndim == 1:
                torch.nn.init.uniform_(p, -0.3, 0.3)
        x = torch.rand(2, C, 24, 28, generator=torch.Generator().manual_seed(5))
        with torch.no_grad():
            y = den(x.to(dev))
        sd = {k: v.cpu() for k, v in den.state_dict().items()}
        assert rel_err(y, ref64(sd, x.double(), 4)) < TOL


def test_repeat_bit_identical(gold, dev):
    den = net(gold, dev)
    x = torch.rand(3, 3, 96, 100, device=dev)
    with torch.no_grad():
        a, b = den(x), den(x)
    assert torch.equal(a, b)


def test_state_dict_round_trip(gold, dev, tmp_path):
    """reference keys load strictly; a saved state dict loads back (pretrained=<path>) and gives the same output"""
    import deepinv_amd as dinv

    den = net(gold, dev)
    assert set(den.state_dict()) == set(c20_state())
    path = tmp_path / "dncnn.pth"
    torch.save(den.state_dict(), path)
    den2 = dinv.models.DnCNN(pretrained=str(path)).to(dev)
    x = torch.rand(1, 3, 64, 64, device=dev)
    with torch.no_grad():
        assert torch.equal(den(x), den2(x))


def _pgd(gold, dev, use_graph):
    import deepinv_amd as dinv

    den = net(gold, dev, depth=6)
    p = dinv.physics.BlurFFT(img_size=(3, 48, 48), filter=gold["pgd_filter"].to(dev), device=dev)
    model = dinv.optim.PGD(prior=dinv.optim.PnP(den), data_fidelity=dinv.optim.L2(), stepsize=1.0, g_param=0.05, max_iter=5,
                           early_stop=False)
    model.fixed_point.use_graph = use_graph
    with torch.no_grad():
        return model(gold["pgd_y"].to(dev), p)


def test_pgd_golden_and_graph(gold, dev):
    eager = _pgd(gold, dev, False)
    assert rel_err(eager, gold["pgd_rec"]) < TOL
    graph = _pgd(gold, dev, True)
    assert torch.equal(graph, eager)


def test_unfolded_training_step(gold, dev):
    """unfolded_builder("PGD") on MultiCoilMRI with PnP(DnCNN(2, 2, depth=7)): loss and gradients of every parameter and of
    the measurements against the reference"""
    import deepinv_amd as dinv

    den = net(gold, dev, C=2, depth=7).train()
    maps = torch.view_as_complex(gold["unf_maps"].contiguous()).to(dev)
    pm = dinv.physics.MultiCoilMRI(mask=gold["unf_mask"].to(dev), coil_maps=maps, img_size=(2, 32, 32), device=dev)
    model = dinv.unfolded.unfolded_builder("PGD", data_fidelity=dinv.optim.L2(), prior=dinv.optim.PnP(den),
                                           params_algo={"stepsize": 0.8, "g_param": 0.05, "lambda": 1.0}, max_iter=3,
                                           trainable_params=["stepsize", "g_param"], device=dev).to(dev)
    y = gold["unf_y"].to(dev).requires_grad_()
    rec = model(y, pm)
    loss = (rec - gold["unf_x"].to(dev)).pow(2).mean()
    loss.backward()
    assert rel_err(rec, gold["unf_rec"]) < TOL
    assert abs(float(loss) - float(gold["unf_loss"])) / float(gold["unf_loss"]) < TOL
    assert rel_err(y.grad, gold["unf_grad_y"]) < TOL
    worst = (0.0, "")
    for n, p in model.named_parameters():
        key = n.replace(".", "_")
        if "unf_grad_" + key not in gold:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n      # g_param: DnCNN ignores the noise level
            continue
        # (large gradients are stored as a stride sample, plus the norm of the whole tensor)
        worst = max(worst, (rel_err(grad_sample(p.grad), gold["unf_grad_" + key]), n),
                    (abs(float(p.grad.double().norm()) / float(gold["unf_gnorm_" + key]) - 1.0), n + " (norm)"))
    print("unfolded DnCNN: worst gradient error vs the reference:", f"{worst[0]:.2e}", worst[1])
    assert worst[0] < 1e-3, worst


def test_backward_fp64_and_reproducible(gold, dev):
    """one autograd node: gradients of x and every weight / bias against fp64 autograd, bit-identical on repeat"""
    den = net(gold, dev, depth=5, nf=64)
    x = torch.rand(2, 3, 40, 36, generator=torch.Generator().manual_seed(6))
    gy = torch.randn(2, 3, 40, 36, generator=torch.Generator().manual_seed(7))
    grads = []
    for _ in range(2):
        den.zero_grad(set_to_none=True)
        xd = x.to(dev).requires_grad_()
        den(xd).backward(gy.to(dev))
        grads.append([xd.grad.clone()] + [p.grad.clone() for p in den.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    sd = {k: v.detach().double().requires_grad_() for k, v in derive(c20_state(), 3, 5, 64).items()}
    xr = x.double().requires_grad_()
    ref64(sd, xr, 5).backward(gy.double())
    assert rel_err(grads[0][0], xr.grad) < TOL
    for (n, p), g in zip(den.named_parameters(), grads[0][1:]):
        assert rel_err(g, sd[n].grad) < 1e-4, n
    with pytest.raises(RuntimeError):
        xd = x.to(dev).requires_grad_()
        (gx,) = torch.autograd.grad(den(xd).sum(), xd, create_graph=True)
        gx.sum().backward()
