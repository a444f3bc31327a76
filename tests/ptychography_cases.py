"""Shared cases of the ptychography tests: deepinv_amd.physics.Ptychography on a device `dev`, checked against
tests/golden/ptychography.npz (the real reference in complex64, with its own error against complex128 next to every output) and
against complex128 restatements written here.  tests/test_emu_ptychography.py runs them on the host emulation of the kernels,
tests/test_ptychography_gpu.py on the GPU.

Bounds: those of tests/phase_retrieval_cases.py.  Where a golden output K exists, the error against complex128 is at most
2 K__err and against the stored complex64 output at most 3 K__err.  The docstring case keeps only some planes / images of each
output in the file (K__sel_*): the stored comparison is over those, the complex128 comparison and K__err over the whole output."""
import os

import numpy as np
import torch

import phase_retrieval_cases as PC
from phase_retrieval_cases import C128, U, Restated, cdot, crel, up  # noqa: F401

import deepinv_amd as dinv
from deepinv_amd.hip import cdense as hcd
from deepinv_amd.hip import ptycho as hpt
from deepinv_amd.physics.phase_retrieval import build_probe, generate_shifts

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ptychography.npz"))
TAGS = [str(t) for t in GOLD["tags"]]
# (img_size, n_img, disk radius) of the generator's cases; c16 takes its probe and shifts from the file
DISKS = {"p16": ((1, 16, 16), 4, 5), "p12x20": ((1, 12, 20), 9, 4), "p33x22": ((1, 33, 22), 4, 6)}
STATE_KEYS = ["B.shifts", "B.init_probe", "B.probe"]


def gold(key, dev=None):
    t = torch.from_numpy(np.asarray(GOLD[key]))
    return t if dev is None else t.to(dev)


def inputs(key, dev):
    """x, yc (complex, measurement-shaped), v (real) and ymeas (non-negative, with zeros) of a case; the docstring case stores
    the last three as factors a[b, l] u[h, w], one multiplication per element"""
    def get(name):
        if f"{key}_{name}" in GOLD:
            return gold(f"{key}_{name}", dev)
        return (gold(f"{key}_{name}__a") * gold(f"{key}_{name}__u")).to(dev)
    return gold(f"{key}_x", dev), get("yc"), get("v"), get("ymeas")


def check(got, key, want, scale=1.0):
    """the two bounds of a golden output; `want` is the complex128 restatement, which must itself be the reference's operator"""
    e = float(GOLD[key + "__err"]) * scale
    ref = gold(key)
    sel = lambda t: t
    if key + "__sel_images" in GOLD:
        images, planes = [int(i) for i in GOLD[key + "__sel_images"]], [int(i) for i in GOLD[key + "__sel_planes"]]
        sel = lambda t: t[images][:, planes]
    got, want = got.detach().cpu(), want.cpu()
    assert tuple(sel(got).shape) == tuple(ref.shape), (key, got.shape, ref.shape)
    assert crel(ref, sel(want)) <= 2 * e, f"{key}: the restatement is not the reference's operator ({crel(ref, sel(want)):.3e})"
    e128, e64 = crel(got, want), crel(sel(got), ref)
    print(f"{key}: kernel vs complex128 {e128:.3e}, vs stored complex64 {e64:.3e}, reference {e:.3e}")
    assert e128 <= 2 * e and e64 <= 3 * e, (key, e128, e64, e)


def restate(probe):
    """complex128 B and B^H (with the conjugate) from the probe stack [1, L, H, W]"""
    P = up(probe)
    return Restated(lambda x: torch.fft.fft2(P * x, norm="ortho"),
                    lambda y: (P.conj() * torch.fft.ifft2(y.to(C128), norm="ortho")).sum(dim=1, keepdim=True))


def physics(tag, dev):
    """the public class built as the generator built the reference's, with its state checked against the reference's"""
    if tag == "doc":
        p = dinv.physics.Ptychography(img_size=(1, 64, 64), device=dev)
    elif tag in DISKS:
        img, n_img, radius = DISKS[tag]
        p = dinv.physics.Ptychography(img_size=img, probe=build_probe(img, type="disk", probe_radius=radius),
                                      shifts=generate_shifts(img, n_img=n_img), device=dev)
    else:
        p = dinv.physics.Ptychography(img_size=tuple(int(v) for v in GOLD[f"{tag}_img"]), probe=gold(f"{tag}_sd__B.init_probe"),
                                      shifts=gold(f"{tag}_sd__B.shifts"), device=dev)
    assert list(p.state_dict().keys()) == [str(k) for k in GOLD[f"{tag}_keys"]] == STATE_KEYS
    for k, v in p.state_dict().items():
        ref = gold(f"{tag}_sd__{k}")
        assert v.dtype == ref.dtype and v.shape == ref.shape and torch.equal(v.cpu(), ref), (tag, k)
    assert p.B.probe.device.type == torch.device(dev).type and p.probe is p.B.probe and p.shifts is p.B.shifts
    return p, restate(gold(f"{tag}_sd__B.probe"))


def run_operators(key, p, r, dev):
    """A, B, B_adjoint, A_vjp, AmplitudeLoss.fn and .grad of one golden case"""
    x, yc, v, ym = inputs(key, dev)
    X, YC, V, YM = up(x), up(yc), up(v), up(ym)
    check(p.A(x), f"{key}_A", r.A(X))
    check(p.B(x), f"{key}_B", r.B(X))
    check(p.B_adjoint(yc), f"{key}_Bt", r.Bt(YC))
    check(p.A_vjp(x, v), f"{key}_vjp", r.vjp(X, V))
    al = dinv.optim.AmplitudeLoss()
    check(al.fn(x, ym, p), f"{key}_alfn", r.alfn(X, YM))
    check(al.grad(x, ym, p), f"{key}_algrad", r.algrad(X, YM))
    assert p(x).dtype == torch.float32 and torch.equal(p(x), p.A(x))
    return x, yc, v, ym


def run_normal(key, p, r, dev, group=0):
    """normal_epilogue under the bounds of the vjp and algrad goldens, and bit for bit the adjoint operation applied to the
    forward operation's stored result at the same group size: both sum the same fp32 values in the same order"""
    x, _, v, ym = inputs(key, dev)
    B = p.B
    nw, na = B.normal_epilogue(x, hcd.WEIGHT, v, group=group), B.normal_epilogue(x, hcd.AMPLITUDE, ym, 1e-12, group=group)
    check(2 * nw, f"{key}_vjp", r.vjp(up(x), up(v)))
    check(2 * na, f"{key}_algrad", r.algrad(up(x), up(ym)))
    assert torch.equal(nw, B.A_adjoint(B.apply_epilogue(x, hcd.WEIGHT, v), group=group))
    assert torch.equal(na, B.A_adjoint(B.apply_epilogue(x, hcd.AMPLITUDE, ym, 1e-12), group=group))
    assert torch.equal(nw, B.normal_epilogue(x, hcd.WEIGHT, v, group=group))
    assert torch.equal(na, B.normal_epilogue(x, hcd.AMPLITUDE, ym, 1e-12, group=group))
    return nw, na


def run_adjoint(key, p, r, dev, group):
    _, yc, _, _ = inputs(key, dev)
    got = p.B.A_adjoint(yc, group=group)
    check(got, f"{key}_Bt", r.Bt(up(yc)))
    assert torch.equal(got, p.B.A_adjoint(yc, group=group))


def run_autograd(key, p, r, dev, zero_planes):
    """gradients of A(x).sum() and of AmplitudeLoss.fn through the fused path against torch.autograd on the complex128
    expression, under the bounds of the vjp and algrad goldens (the same computations with v = 1 and eps = 0).

    With a probe plane that is all zero, u = |Bx|^2 is exactly zero on that plane and the derivative of sqrt(u) there is
    infinite: the gradient of AmplitudeLoss.fn does not exist, in the reference and in complex128 alike (0 times inf).  For those
    cases the second check is that both sides say so."""
    x, _, _, ym = inputs(key, dev)
    al = dinv.optim.AmplitudeLoss()
    for name, f, f128 in (("vjp", lambda t: p.A(t).sum(), lambda t: r.A(t).sum()),
                          ("algrad", lambda t: al.fn(t, ym, p).sum(), lambda t: r.alfn(t, up(ym)).sum())):
        a = x.clone().requires_grad_(True)
        f(a).backward()
        b = up(x).requires_grad_(True)
        f128(b).backward()
        if name == "algrad" and len(zero_planes):
            assert not torch.isfinite(b.grad.real).all() and not torch.isfinite(a.grad.real).all()
            continue
        e = crel(a.grad, b.grad)
        print(f"{key} autograd {name}: {e:.3e} (reference {float(GOLD[f'{key}_{name}__err']):.3e})")
        assert e <= 2 * float(GOLD[f"{key}_{name}__err"])


def run_zero_planes(key, p, dev):
    """on a plane whose probe is zero, with measurements that hold zeros and non-zeros: the AMPLITUDE result is finite and
    exactly zero"""
    zero = [int(l) for l in GOLD[f"{key}_zero_planes"]]
    x, _, _, ym = inputs(key, dev)
    assert zero and bool((ym[:, zero] == 0).any()) and bool((ym[:, zero] > 0).any())
    got = p.B.apply_epilogue(x, hcd.AMPLITUDE, ym, 1e-12)
    assert torch.isfinite(got.real).all() and torch.isfinite(got.imag).all() and bool((got[:, zero] == 0).all())
    assert torch.isfinite(dinv.optim.AmplitudeLoss().grad(x, ym, p).real).all()


def run_spectral(tag, p, r, dev):
    y, x0 = gold(f"{tag}_spec_y", dev), gold(f"{tag}_spec_x0", dev)
    n = int(GOLD["spec_iters"])
    got = dinv.optim.spectral_methods(y, p, x=x0, n_iter=n, early_stop=False)
    check(got, f"{tag}_spec_x", r.spectral(up(y), up(x0), n))


def run_boundary(dev):
    """the largest fused square and the next size up (composed path), n_img = 4, against complex128 torch.fft within the derived
    bound of one transform and one diagonal plus n_img units in the last place for the sum"""
    n = PC.largest_fused_square()
    for side in (n, n + 1):
        img = (1, side, side)
        p = dinv.physics.Ptychography(img_size=img, probe=torch.randn(img, dtype=torch.complex64, generator=torch.Generator().manual_seed(side)),
                                      shifts=generate_shifts(img, n_img=4), device=dev)
        assert hpt.fits(side, side) == (side == n)
        r = restate(p.B.probe)
        g = torch.Generator().manual_seed(side + 1)
        x = torch.randn((1, *img), dtype=torch.complex64, generator=g).to(dev)
        yc = torch.randn((1, 4, side, side), dtype=torch.complex64, generator=g).to(dev)
        w = torch.randn((1, 4, side, side), generator=g).to(dev)
        bound = PC.derived_fft_bound(side, side, 1, 1, dev)
        e, et = crel(p.B(x), r.B(up(x))), crel(p.B_adjoint(yc), r.Bt(up(yc)))
        en = crel(p.B.normal_epilogue(x, hcd.WEIGHT, w), r.Bt(r.B(up(x)) * up(w)))
        print(f"{side} x {side}: B {e:.3e} B^H {et:.3e} normal {en:.3e} bound {bound:.3e}")
        assert e <= bound and et <= bound + 4 * U
        assert en <= PC.derived_fft_bound(side, side, 2, 2, dev) + 5 * U       # two transforms and probes, the weight, the sum


def probe_groups(p, B, op, group=0):
    _, L, H, W = p.B.probe.shape
    return hpt.groups(B, L, H, W, op, group)
