"""Phase retrieval without a GPU and without a kernel: constructor errors, state-dict keys, ``get_structure``, the view and
conjugate handling of the matrix wrapper, and the unchanged refusals of the real operators."""
import numpy as np
import pytest
import torch

import deepinv_amd as dinv
from deepinv_amd.hip import HipExtensionError
from deepinv_amd.hip import cdense as hcd
from deepinv_amd.physics import phase_retrieval as PR


def test_exports():
    for name in ("PhaseRetrieval", "RandomPhaseRetrieval", "StructuredRandomPhaseRetrieval"):
        assert hasattr(dinv.physics, name)
    for name in ("AmplitudeLoss", "AmplitudeLossDistance", "default_preprocessing", "correct_global_phase", "cosine_similarity",
                 "spectral_methods", "spectral_methods_wrapper"):
        assert hasattr(dinv.optim, name)


def test_random_constructor_and_state_dict():
    p = dinv.physics.RandomPhaseRetrieval(m=10, img_size=(2, 3, 3), rng=torch.Generator().manual_seed(1))
    assert sorted(p.state_dict()) == ["B._A", "B._A_adjoint", "B._A_dagger", "B.initial_random_state", "initial_random_state"]
    assert p.B._A.shape == (10, 18) and p.B._A.dtype == torch.cfloat and p.name == "Random Phase Retrieval"
    assert p.B._A_adjoint.is_conj() and p.B._A_adjoint.data_ptr() == p.B._A.data_ptr()
    # the reference's own draw expression
    want = torch.randn((10, 18), dtype=torch.cfloat, generator=torch.Generator().manual_seed(1)) / np.sqrt(10)
    assert torch.equal(p.B._A, want)
    # the pseudo-inverse, from complex128 on the host
    assert torch.allclose(p.B._A_dagger, torch.linalg.pinv(want.to(torch.complex128)).to(torch.cfloat))
    assert abs(float(p.get_A_squared_mean().abs()) - 0.1) < 0.05      # E|B_ij|^2 = 1 / m
    cw = dinv.physics.RandomPhaseRetrieval(m=10, img_size=(2, 3, 3), channelwise=True)
    assert cw.B._A.shape == (10, 9)
    with pytest.raises(NotImplementedError, match="cfloat"):
        dinv.physics.RandomPhaseRetrieval(m=10, img_size=(2, 3, 3), dtype=torch.float)
    q = dinv.physics.RandomPhaseRetrieval(m=10, img_size=(2, 3, 3))
    q.load_state_dict(p.state_dict())
    assert torch.equal(q.B._A, p.B._A) and torch.equal(q.B._A_adjoint, p.B._A.conj().T)
    assert q.B._A_adjoint.data_ptr() == q.B._A.data_ptr()


def test_structured_constructor_and_state_dict():
    S = dinv.physics.StructuredRandomPhaseRetrieval
    p = S((2, 8, 12), (2, 8, 12), 2.5)
    assert list(p.state_dict()) == ["B.diagonals"] and p.B.diagonals.shape == (2, 2, 8, 12) and p.B.diagonals.dtype == torch.cfloat
    assert torch.allclose(p.B.diagonals.abs(), torch.ones(2, 2, 8, 12))
    assert p.structure == "FDFDF" and p.mode == "equisampling" and len(p.diagonals) == 2 and p.name == "Structured Random Phase Retrieval"
    assert not torch.equal(p.diagonals[0], p.diagonals[1]) and not torch.equal(p.diagonals[0][0], p.diagonals[0][1])
    assert S.get_structure(0.5) == "F" and S.get_structure(1) == "FD" and S.get_structure(3.5) == "FDFDFDF"
    sh = S((1, 8, 12), (1, 8, 12), 3, shared_weights=True)
    assert torch.equal(sh.diagonals[0], sh.diagonals[2])
    assert S((1, 8, 12), (1, 11, 15), 1).B.diagonals.shape == (1, 1, 11, 15)          # oversampling: the output size
    assert S((1, 8, 12), (1, 5, 7), 1).B.diagonals.shape == (1, 1, 8, 12)             # undersampling: the image size
    half = S((1, 8, 12), (1, 8, 12), 0.5)
    assert half.B.diagonals.shape == (0, 1, 8, 12) and half.get_A_squared_mean() is None
    assert abs(float(p.get_A_squared_mean().abs()) - 1) < 0.2
    assert float(S((1, 8, 12), (1, 16, 24), 1).oversampling_ratio) == 4.0
    with pytest.raises(ValueError, match="integer or an integer plus 0.5"):
        S((1, 8, 12), (1, 8, 12), 1.25)
    with pytest.raises(ValueError, match="Unimplemented transform"):
        S((1, 8, 12), (1, 8, 12), 1, transform="dst")
    with pytest.raises(ValueError, match="Unsupported mode"):
        S((1, 8, 12), (1, 8, 12), 1, diagonal_mode="rademacher")
    with pytest.raises(ValueError, match="different sampling schemes"):
        S((1, 8, 12), (1, 9, 11), 1)
    with pytest.raises(NotImplementedError, match="cfloat"):
        S((1, 8, 12), (1, 8, 12), 1, dtype=torch.complex128)
    with pytest.raises(ValueError, match="working size"):
        PR._StructuredLinear((1, 8, 12), (1, 11, 15), 1, diagonals=[torch.ones(1, 8, 12, dtype=torch.cfloat)])
    with pytest.raises(TypeError, match=r"\.to\(torch\.cfloat\)"):
        PR._StructuredLinear((1, 8, 12), (1, 8, 12), 1, diagonals=[torch.ones(1, 8, 12)])


def test_matrix_views_and_conjugates():
    """a row-major matrix, its transposed view and the lazily conjugated views of both are read where they lie"""
    A = torch.randn(6, 10, dtype=torch.cfloat)
    for M, want in ((A, (10, 0, 0)), (A.t(), (10, 1, 0)), (A.conj(), (10, 0, 1)), (A.conj().T, (10, 1, 1)), (A.mH, (10, 1, 1)),
                    (A[:, :4], (10, 0, 0)), (A[:3].mH, (10, 1, 1))):
        store, ldm, tr, cj = hcd._matrix(M)
        assert store.data_ptr() == A.data_ptr() and not store.is_conj() and (ldm, tr, cj) == want
    store, ldm, tr, cj = hcd._matrix(A[:, ::2].conj())
    assert store.data_ptr() != A.data_ptr() and (ldm, tr, cj) == (5, 0, 0) and torch.equal(store, A[:, ::2].conj().resolve_conj())
    with pytest.raises(TypeError, match=r"\.to\(torch\.cfloat\)"):
        hcd._matrix(A.real.contiguous())
    with pytest.raises(ValueError, match="matrix"):
        hcd._matrix(A[0])


def test_no_cpu_fallback():
    p = dinv.physics.RandomPhaseRetrieval(m=6, img_size=(1, 3, 3))
    with pytest.raises(HipExtensionError):
        p.A(torch.randn(1, 1, 3, 3, dtype=torch.cfloat))
    s = dinv.physics.StructuredRandomPhaseRetrieval((1, 8, 12), (1, 8, 12), 1)
    with pytest.raises(HipExtensionError):
        s.B_adjoint(torch.randn(1, 1, 8, 12, dtype=torch.cfloat))


def test_helpers():
    a = torch.randn(2, 1, 4, 4, dtype=torch.cfloat)
    b = a * torch.exp(torch.tensor(0.7j))
    assert torch.allclose(dinv.optim.cosine_similarity(a, b), torch.tensor(1.0), atol=1e-6)
    assert torch.allclose(dinv.optim.correct_global_phase(b, a), a, atol=1e-5)
    assert torch.allclose(dinv.optim.correct_global_phase(3 * b, a, correct_magnitude=True), a, atol=1e-5)
    y = torch.tensor([0.1, 1.0, 4.0])
    assert torch.equal(dinv.optim.default_preprocessing(y, None), torch.tensor([-5.0, 0.0, 0.75]))
    d = dinv.optim.AmplitudeLossDistance()
    u = torch.tensor([[4.0, 9.0]])
    assert torch.allclose(d.fn(u, torch.tensor([[1.0, 4.0]])), torch.tensor([2.0]))
    assert torch.allclose(d.grad(u, torch.tensor([[1.0, 0.0]])), torch.tensor([[0.5, 1.0]]))
    with pytest.raises(ValueError, match="same"):
        dinv.optim.correct_global_phase(a, a[:1])


def test_real_operators_still_refuse_complex():
    with pytest.raises(NotImplementedError, match="phase retrieval"):
        dinv.physics.CompressedSensing(m=4, img_size=(1, 3, 3), dtype=torch.cfloat)
    with pytest.raises(NotImplementedError, match="phase retrieval"):
        dinv.physics.structured_random.generate_diagonal((1, 4, 4), mode="uniform_phase")
    with pytest.raises(NotImplementedError, match="phase retrieval"):
        dinv.physics.StructuredRandom((1, 4, 4), (1, 4, 4), diagonals=[torch.ones(1, 4, 4, dtype=torch.cfloat)])


def test_random_linear_checks_the_generator_device_like_compressed_sensing():
    kw = dict(m=10, img_size=(1, 3, 3), device="meta", rng=torch.Generator("cpu"))
    with pytest.raises(ValueError, match="random generator") as cs:
        dinv.physics.CompressedSensing(**kw)
    with pytest.raises(ValueError, match="random generator") as rl:
        PR._RandomLinear(**kw)
    assert str(rl.value) == str(cs.value)
