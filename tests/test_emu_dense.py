"""Dense fp32 MFMA product (deepinv_amd/csrc/dense.hip) on the host emulation against ``torch.matmul`` in float64.

Bound against fp64: twice the reference's own fp32 error (``K__err`` of tests/golden/compressed_sensing.npz) for the
CompressedSensing golden cases.  For the shape sweep, which has no golden case, the worst-case rounding of the arithmetic,
elementwise: an output is a sum of K products accumulated by fused multiply-adds in S slices and S - 1 additions of the slices,
so |got - exact| <= gamma_{K+S} sum_k |in[i, k]| |M[r, k]| with gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import emu_lib as E
from emu_backend import emu_backend
from emu_lib import lib

from deepinv_amd.hip import dense as hdense

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compressed_sensing.npz"))
U = 2.0 ** -24


def dense(x, M, transposed=False):
    """out[i, r] = sum_k x[i, k] M[r, k]; `transposed`: M is handed over as the contiguous [K, R] matrix"""
    l = lib()
    I, K = x.shape
    R = M.shape[0]
    store = M.t().contiguous() if transposed else M.contiguous()
    out = torch.full((I, R), float("nan"))
    nbytes = l.dinv_dense_workspace_bytes(I, K, R)
    ws = torch.full((nbytes // 4,), float("nan"))
    rc = l.dinv_dense_apply(E.p(x), E.p(store), E.p(out), I, K, R, store.shape[1], int(transposed), E.p(ws) if nbytes else None,
                            nbytes, None)
    assert rc == 0, l.dinv_last_error()
    return out, nbytes


def slices(I, K, R):
    return max(lib().dinv_dense_workspace_bytes(I, K, R) // (4 * I * R), 1)


def rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-300))


def within_gamma(got, x, M, K, S):
    """the elementwise bound of the docstring: |got - exact| <= gamma_{K+S} |x| |M|^T"""
    n = K + S
    gamma = n * U / (1 - n * U)
    x, M = x.double(), M.double()
    return bool(((got.double() - x @ M.t()).abs() <= gamma * (x.abs() @ M.abs().t())).all())


@pytest.mark.parametrize("transposed", [False, True], ids=["rows", "transposed"])
@pytest.mark.parametrize("R", [10, 48, 500])
@pytest.mark.parametrize("K", [9, 192, 1000, 1024])
@pytest.mark.parametrize("I", [1, 3, 33])
def test_shape_sweep(I, K, R, transposed):
    g = torch.Generator().manual_seed(I * 7 + K * 3 + R)
    x, M = torch.randn(I, K, generator=g), torch.randn(R, K, generator=g)
    got, _ = dense(x, M, transposed)
    assert not torch.isnan(got).any()
    want = x.double() @ M.double().t()
    n = K + slices(I, K, R)
    gamma = n * U / (1 - n * U)
    assert bool(((got.double() - want).abs() <= gamma * (x.double().abs() @ M.double().abs().t())).all())
    again, _ = dense(x, M, transposed)
    assert torch.equal(got, again)


def test_split_k_boundaries():
    """K = 1000 over several slices ends its last slice short, K = 1024 fills them, K = 9 is a single slice that writes `out` itself"""
    assert slices(3, 1000, 48) > 1 and slices(3, 1024, 48) > 1 and slices(3, 9, 48) == 1
    assert lib().dinv_dense_workspace_bytes(3, 9, 48) == 0
    # an uneven crossing: ones make every partial sum exact, so a k counted twice or dropped shows as an integer error
    for K in (1000, 97, 65):
        x, M = torch.ones(2, K), torch.ones(40, K)
        for t in (False, True):
            assert torch.equal(dense(x, M, t)[0], torch.full((2, 40), float(K))), (K, t)


def test_more_rows_than_accumulators():
    """I = 130 takes two chunks of 128 rows"""
    g = torch.Generator().manual_seed(5)
    x, M = torch.randn(130, 70, generator=g), torch.randn(33, 70, generator=g)
    for t in (False, True):
        got, _ = dense(x, M, t)
        assert within_gamma(got, x, M, 70, slices(130, 70, 33))
        with emu_backend():                                      # the product's wrapper makes the same call: M, or the view of M^T
            assert torch.equal(hdense.apply(x, M.t().contiguous().t() if t else M), got)


def test_row_stride_and_unaligned():
    """a matrix inside a wider one (ldm > K, not a multiple of 4) and operands off 16-byte alignment take the scalar loads"""
    g = torch.Generator().manual_seed(6)
    big = torch.randn(20, 75, generator=g)
    xbuf = torch.randn(3 * 64 + 1, generator=g)
    x = xbuf[1:].view(3, 64)
    out = torch.full((3, 20), float("nan"))
    l = lib()
    nbytes = l.dinv_dense_workspace_bytes(3, 64, 20)
    ws = torch.empty(max(nbytes // 4, 1))
    assert l.dinv_dense_apply(ctypes.c_void_p(x.data_ptr()), E.p(big), E.p(out), 3, 64, 20, 75, 0, E.p(ws), nbytes, None) == 0
    assert within_gamma(out, x, big[:, :64], 64, slices(3, 64, 20))


TAGS = [str(t) for t in GOLD["cs_tags"]] + ["doc"]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("tag", TAGS)
def test_compressed_sensing_golden(tag, B):
    A = torch.from_numpy(GOLD[f"{tag}_sd___A"])
    Ad = torch.from_numpy(GOLD[f"{tag}_sd___A_dagger"])
    x, y = torch.from_numpy(GOLD[f"{tag}_b{B}_x"]), torch.from_numpy(GOLD[f"{tag}_b{B}_y"])
    cw = bool(GOLD[f"{tag}_cw"])
    xf = x.reshape(B * x.shape[1], -1) if cw else x.reshape(B, -1)
    yf = y.reshape(-1, y.shape[-1])
    for key, inp, M, tr in ((f"{tag}_b{B}_A", xf, A, False), (f"{tag}_b{B}_At", yf, A.t(), True), (f"{tag}_b{B}_Ad", yf, Ad, False)):
        want = inp.double() @ M.double().t()
        ref = torch.from_numpy(GOLD[key]).reshape(want.shape)
        bound = 2 * float(GOLD[key + "__err"])
        assert rel(ref, want) <= bound
        got, _ = dense(inp, M, tr)
        err = rel(got, want)
        print(f"{key} kernel {err:.3e} reference {bound / 2:.3e}")
        assert err <= bound


def test_argument_checks():
    l = lib()
    x, M, out = torch.zeros(2, 8), torch.zeros(4, 8), torch.zeros(2, 4)
    assert l.dinv_dense_apply(E.p(x), E.p(M), E.p(out), 2, 8, 4, 7, 0, None, 0, None) != 0 and b"row stride" in l.dinv_last_error()
    assert l.dinv_dense_apply(E.p(x), None, E.p(out), 2, 8, 4, 8, 0, None, 0, None) != 0
    assert l.dinv_dense_apply(E.p(x), E.p(M), E.p(out), 2, 0, 4, 8, 0, None, 0, None) != 0 and b"bad shape" in l.dinv_last_error()
    xx, MM, oo = torch.zeros(2, 1000), torch.zeros(48, 1000), torch.full((2, 48), float("nan"))
    assert l.dinv_dense_apply(E.p(xx), E.p(MM), E.p(oo), 2, 1000, 48, 1000, 0, None, 0, None) != 0
    assert b"workspace" in l.dinv_last_error() and torch.isnan(oo).all()
