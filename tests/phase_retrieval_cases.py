"""Shared cases of the phase-retrieval tests: the public classes of deepinv_amd on a device `dev`, checked against
tests/golden/phase_retrieval.npz (the real reference in complex64, with its own error against complex128 next to every output)
and against complex128 restatements written here.  tests/test_emu_phase_retrieval.py runs them on the host emulation of the
kernels, tests/test_phase_retrieval_gpu.py on the GPU.

Bounds.  Where a golden output K exists: the error against complex128 is at most 2 K__err, against the stored complex64 output
at most 3 K__err (the project's rule).  conftest.rel_err and conftest.dot_test drop imaginary parts, so this module has its own
complex relative l2 error and conjugate-inner-product dot test."""
import math
import os

import numpy as np
import torch

import deepinv_amd as dinv
from deepinv_amd.hip import cdense as hcd
from deepinv_amd.hip import cstructured as hcs

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phase_retrieval.npz"))
C128 = torch.complex128
U = 2.0 ** -24
RP_TAGS = [str(t) for t in GOLD["rp_tags"]]
SP_TAGS = [str(t) for t in GOLD["sp_tags"]]


def up(t):
    t = t.detach().cpu()
    return t.to(C128) if t.is_complex() else t.double()


def crel(a, b) -> float:
    """||a - b||_2 / ||b||_2 over complex128 (or float64) on the CPU"""
    a, b = up(a), up(b)
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b).clamp_min(1e-300))


def cdot(B, x, y) -> float:
    """|<Bx, y> - <x, B^H y>| / (||Bx|| ||y||) with <a, b> = sum conj(a) b"""
    Bx, Bty = up(B.A(x)), up(B.A_adjoint(y))
    s1, s2 = (Bx.conj() * up(y)).sum(), (up(x).conj() * Bty).sum()
    return float((s1 - s2).abs() / (torch.linalg.vector_norm(Bx) * torch.linalg.vector_norm(up(y))))


def gold(key, dev=None):
    t = torch.from_numpy(np.asarray(GOLD[key]))
    return t if dev is None else t.to(dev)


def check(got, key, want, scale=1.0):
    """the two bounds of a golden output; `want` is the complex128 restatement, which must itself be the reference's operator"""
    e = float(GOLD[key + "__err"]) * scale
    ref = gold(key)
    assert tuple(got.shape) == tuple(ref.shape), (key, got.shape, ref.shape)
    assert crel(ref, want) <= 2 * e, f"{key}: the restatement is not the reference's operator ({crel(ref, want):.3e})"
    e128, e64 = crel(got, want), crel(got, ref)
    print(f"{key}: kernel vs complex128 {e128:.3e}, vs stored complex64 {e64:.3e}, reference {e:.3e}")
    assert e128 <= 2 * e and e64 <= 3 * e, (key, e128, e64, e)


# ---------------------------------------------------------------- complex128 restatements
class Restated:
    """phase retrieval in complex128 from the two linear maps B and B^H"""

    def __init__(self, B, Bt, Bd=None):
        self.B, self.Bt, self.Bd = B, Bt, Bd

    def A(self, x):
        return self.B(x).abs().square()

    def vjp(self, x, v):
        return 2 * self.Bt(self.B(x) * v)

    def alfn(self, x, y):
        d = torch.sqrt(self.A(x)) - torch.sqrt(y)
        return torch.linalg.vector_norm(d, dim=tuple(range(1, d.dim()))) ** 2

    def algrad(self, x, y, eps=1e-12):
        return self.vjp(x, 1 - torch.sqrt(y / (self.A(x) + eps)))

    def spectral(self, y, x, n_iter, lamb=10.0, rtol=None):
        norm_x = torch.sqrt(y.sum())
        y = y / y.mean()
        T = torch.max(1 - 1 / y, torch.tensor(-5.0, dtype=y.dtype))
        for _ in range(n_iter):
            x_new = self.Bt(T * self.B(x)) + lamb * x
            x_new = x_new / torch.linalg.norm(x_new)
            if rtol is not None and torch.linalg.norm(x_new - x) / torch.linalg.norm(x) < rtol:
                break
            x = x_new
        return x * norm_x


def restate_random(A, Ad, img, cw):
    A, Ad = up(A), up(Ad)
    C, H, W = img

    def B(x):
        N = x.shape[0]
        y = torch.einsum("in,mn->im", x.reshape(N * C, -1) if cw else x.reshape(N, -1), A)
        return y.view(N, C, -1) if cw else y

    def back(M):
        def f(y):
            N = y.shape[0]
            return torch.einsum("im,nm->in", y.to(C128).reshape(N * C, -1) if cw else y.to(C128), M).reshape(N, C, H, W)
        return f

    return Restated(B, back(A.conj().T), back(Ad))


def _pad(t, small, big):
    top, left = math.ceil((big[0] - small[0]) / 2), math.ceil((big[1] - small[1]) / 2)
    return torch.nn.functional.pad(t, (left, big[1] - small[1] - left, top, big[0] - small[0] - top))


def _trim(t, big, small):
    top, left = math.ceil((big[0] - small[0]) / 2), math.ceil((big[1] - small[1]) / 2)
    return t[..., top:top + small[0], left:left + small[1]]


def restate_structured(diag, img, osz, nl):
    diag = up(diag)
    L, half = math.floor(nl), nl - math.floor(nl) == 0.5
    i, o = tuple(img[1:]), tuple(osz[1:])
    work = (max(i[0], o[0]), max(i[1], o[1]))
    F = lambda t: torch.fft.fft2(t, norm="ortho")
    Fi = lambda t: torch.fft.ifft2(t, norm="ortho")

    def B(x):
        x = _pad(x, i, work)
        if half:
            x = F(x)
        for l in range(L):
            x = F(diag[l] * x)
        return _trim(x, work, o)

    def Bt(y):
        y = _pad(y.to(C128), o, work)
        for l in range(L):
            y = diag[L - 1 - l].conj() * Fi(y)
        if half:
            y = Fi(y)
        return _trim(y, work, i)

    return Restated(B, Bt, Bt)


# ---------------------------------------------------------------- the public classes from the golden file
def random_physics(tag, dev):
    m, img, cw = int(GOLD[f"{tag}_m"]), tuple(int(v) for v in GOLD[f"{tag}_img"]), bool(GOLD[f"{tag}_cw"])
    p = dinv.physics.RandomPhaseRetrieval(m=m, img_size=img, channelwise=cw, device=dev)
    keys = [str(k) for k in GOLD[f"{tag}_keys"]]
    assert sorted(p.state_dict().keys()) == keys == sorted(["B._A", "B._A_adjoint", "B._A_dagger", "B.initial_random_state",
                                                           "initial_random_state"])
    sd = {k: gold(f"{tag}_sd__{k}") for k in keys}
    p.load_state_dict(sd)
    assert torch.equal(p.B._A.cpu(), sd["B._A"]) and torch.equal(p.B._A_adjoint.cpu(), sd["B._A"].conj().T)
    # one copy of the matrix: the adjoint buffer is a view of _A
    assert p.B._A_adjoint.is_conj() and p.B._A_adjoint.data_ptr() == p.B._A.data_ptr()
    return p, restate_random(sd["B._A"], sd["B._A_dagger"], img, cw)


def structured_physics(tag, dev):
    key = f"sp_{tag}"
    img, osz = tuple(int(v) for v in GOLD[f"{key}_img"]), tuple(int(v) for v in GOLD[f"{key}_out"])
    nl, shared = float(GOLD[f"{key}_layers"]), bool(GOLD[f"{key}_shared"])
    nl = int(nl) if nl == int(nl) else nl
    p = dinv.physics.StructuredRandomPhaseRetrieval(img, osz, nl, shared_weights=shared, device=dev)
    assert list(p.state_dict().keys()) == ["B.diagonals"]
    diag = gold(f"{key}_diag")
    p.load_state_dict({"B.diagonals": diag})
    assert len(p.diagonals) == math.floor(nl) and all(torch.equal(d.cpu(), diag[i]) for i, d in enumerate(p.diagonals))
    return p, restate_structured(diag, img, osz, nl)


def run_operators(key, p, r, dev):
    """A, B, B_adjoint, B_dagger, A_vjp, AmplitudeLoss.fn and .grad of one golden case"""
    x, yc, v, ym = gold(f"{key}_x", dev), gold(f"{key}_yc", dev), gold(f"{key}_v", dev), gold(f"{key}_ymeas", dev)
    X, YC, V, YM = up(x), up(yc), up(v), up(ym)
    check(p.A(x), f"{key}_A", r.A(X))
    check(p.B(x), f"{key}_B", r.B(X))
    check(p.B_adjoint(yc), f"{key}_Bt", r.Bt(YC))
    check(p.B_dagger(yc), f"{key}_Bd", r.Bd(YC))
    check(p.A_vjp(x, v), f"{key}_vjp", r.vjp(X, V))
    al = dinv.optim.AmplitudeLoss()
    check(al.fn(x, ym, p), f"{key}_alfn", r.alfn(X, YM))
    check(al.grad(x, ym, p), f"{key}_algrad", r.algrad(X, YM))
    assert p(x).dtype == torch.float32 and torch.equal(p(x), p.A(x))      # forward: no noise by default, run to run identical
    return x, X, ym, YM


def run_autograd(key, p, r, dev):
    """gradients of A(x).sum() and of AmplitudeLoss.fn through the fused path against torch.autograd on the complex128
    expression.  Both are the computations of A_vjp and AmplitudeLoss.grad (with v = 1, and eps = 0), so they take the bound of
    those golden outputs: twice the reference's own error."""
    x, ym = gold(f"{key}_x", dev), gold(f"{key}_ymeas", dev)
    al = dinv.optim.AmplitudeLoss()
    for name, f, f128 in (("vjp", lambda t: p.A(t).sum(), lambda t: r.A(t).sum()),
                          ("algrad", lambda t: al.fn(t, ym, p).sum(), lambda t: r.alfn(t, up(ym)).sum())):
        a = x.clone().requires_grad_(True)
        f(a).backward()
        b = up(x).requires_grad_(True)
        f128(b).backward()
        e = crel(a.grad, b.grad)
        print(f"{key} autograd {name}: {e:.3e} (reference {float(GOLD[f'{key}_{name}__err']):.3e})")
        assert e <= 2 * float(GOLD[f"{key}_{name}__err"])


def run_epilogues(p, r, x, eB, dev):
    """ABS2, WEIGHT and AMPLITUDE of the operator B of p against the composed complex128 expression, with measurements that hold
    zeros.  With z exact and z + dz computed, |dz| <= e |z| (e = 2 eB, the bound of the golden B):  |z|^2 is within 2 e + u,
    z w within e + u, and the amplitude factor f = 1 - s, s = sqrt(y / (|z|^2 + eps)), moves by |df| <= s (e + 2 u) (half the
    relative error of |z|^2 and the roundings of the division and the root), so z f is within e |z f| + (e + 2 u) |z s| + u |z f|;
    summed in l2."""
    e = 2 * eB
    Z = r.B(up(x))
    y = p.A(x) * torch.rand(Z.shape, generator=torch.Generator().manual_seed(3)).to(dev) * 2
    y.view(-1)[::5] = 0.0                                           # y = 0: the factor is exactly 1
    w = torch.randn(Z.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    Y, W = up(y), up(w)
    B = p.B
    assert crel(B.apply_epilogue(x, hcd.ABS2), Z.abs().square()) <= 2 * e + U
    assert crel(B.apply_epilogue(x, hcd.WEIGHT, w), Z * W) <= e + U
    s = torch.sqrt(Y / (Z.abs().square() + 1e-12))
    want = Z * (1 - s)
    got = up(B.apply_epilogue(x, hcd.AMPLITUDE, y, 1e-12))
    bound = (e + U) * float(torch.linalg.vector_norm(want)) + (e + 2 * U) * float(torch.linalg.vector_norm(Z * s))
    err = float(torch.linalg.vector_norm(got - want))
    print(f"amplitude epilogue: error {err:.3e} bound {bound:.3e}")
    assert torch.isfinite(got.real).all() and err <= bound
    zero_y = Y == 0
    assert zero_y.any() and crel(got[zero_y], Z[zero_y]) <= e + U
    return got, Z, y


def run_spectral(tag, p, r, dev, loop=True):
    y, x0 = gold(f"{tag}_y", dev), gold(f"{tag}_x0", dev)
    n = int(GOLD["spec_iters"])
    got = dinv.optim.spectral_methods(y, p, x=x0, n_iter=n, early_stop=False)
    check(got, f"{tag}_x", r.spectral(up(y), up(x0), n))
    if not loop:
        return
    # spectral initialisation, then explicit gradient steps on the amplitude loss
    al, step = dinv.optim.AmplitudeLoss(), float(GOLD["loop_stepsize"])
    x, X = got, r.spectral(up(y), up(x0), n)
    for _ in range(int(GOLD["loop_steps"])):
        x = x - step * al.grad(x, y, p)
        X = X - step * r.algrad(X, up(y))
    check(x, f"{tag}_loop", X)


def derived_fft_bound(H, W, transforms, diagonals, dev):
    """the bound tests/test_emu_dst.py derives: a radix-r stage adds at most (r + 3) u to the relative l2 error (radix 4 and 8
    are two and three radix-2 levels), the scale and a diagonal one u each; summed over both axes and all transforms"""
    from deepinv_amd.hip import fft_plan
    cost = {4: 10, 8: 15}
    per = 1
    for n in (H, W):
        plan, _ = fft_plan(n, dev)
        per += sum(cost.get(r, r + 3) for r in plan.radix[:plan.nstages])
    return (transforms * per + diagonals) * U


def largest_fused_square():
    n = 1
    while hcs.fits(n + 1, n + 1):
        n += 1
    return n
