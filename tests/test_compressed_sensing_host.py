"""Host logic of StructuredRandom and CompressedSensing (no GPU): shape helpers against the golden shapes, constructor errors,
state-dict keys, the no-CPU-fallback rule and the order in which user-supplied transforms are called."""
import os

import numpy as np
import pytest
import torch

import deepinv_amd as dinv
from deepinv_amd.physics import structured_random as SR

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compressed_sensing.npz"))


def test_compare_padding_trimming_against_golden_shapes():
    assert SR.compare((2, 8, 12), (2, 8, 12)) == "equisampling"
    assert SR.compare((2, 8, 12), (2, 11, 15)) == "oversampling"
    assert SR.compare((2, 8, 12), (2, 5, 7)) == "undersampling"
    with pytest.raises(ValueError):
        SR.compare((2, 8, 12), (2, 9, 7))
    x = torch.arange(2 * 8 * 12, dtype=torch.float32).view(1, 2, 8, 12) + 1
    p = SR.padding(x, (2, 8, 12), (2, 11, 15))
    assert tuple(p.shape[1:]) == tuple(GOLD["sr_over1_A"].shape[1:]) == (2, 11, 15)
    # ceil of the difference on the top / left, floor on the bottom / right
    assert torch.equal(p[..., 2:10, 2:14], x) and p[..., :2, :].abs().sum() == 0 and p[..., 10:, :].abs().sum() == 0
    assert p[..., :2].abs().sum() == 0 and p[..., 14:].abs().sum() == 0
    t = SR.trimming(x, (2, 8, 12), (2, 5, 7))
    assert tuple(t.shape[1:]) == tuple(GOLD["sr_under2.5_A"].shape[1:]) == (2, 5, 7)
    assert torch.equal(t, x[..., 2:7, 3:10])
    assert torch.equal(SR.trimming(p, (2, 8, 12), (2, 11, 15)), x)


def test_constructor_errors():
    SRand, CS = dinv.physics.StructuredRandom, dinv.physics.CompressedSensing
    with pytest.raises(ValueError, match="different sampling"):
        SRand((2, 8, 12), (2, 9, 7))
    with pytest.raises(ValueError, match="working size"):
        SRand((2, 8, 12), (2, 11, 15), diagonals=[torch.ones(2, 8, 12)])
    with pytest.raises(ValueError, match="output size"):
        SRand((2, 8, 12), (2, 11, 15))
    with pytest.raises(NotImplementedError):
        SRand((2, 8, 12), (2, 8, 12), diagonals=[torch.ones(2, 8, 12, dtype=torch.cfloat)])
    with pytest.raises(NotImplementedError):
        SR.generate_diagonal((2, 8, 12), mode="uniform_phase")
    with pytest.raises(ValueError):
        SR.generate_diagonal((2, 8, 12), mode="gaussian")
    with pytest.raises(NotImplementedError):
        CS(m=10, img_size=(1, 3, 3), dtype=torch.cfloat)
    with pytest.raises(ValueError, match="random generator"):
        CS(m=10, img_size=(1, 3, 3), device="meta", rng=torch.Generator("cpu"))


def test_defaults_and_state_dict_keys():
    p = dinv.physics.StructuredRandom((2, 8, 12), (2, 5, 7), n_layers=2.5, rng=torch.Generator().manual_seed(1))
    assert p.mode == "undersampling" and tuple(p.diagonals.shape) == (2, 2, 8, 12)
    assert set(p.diagonals.unique().tolist()) == {-1.0, 1.0}
    assert list(p.state_dict().keys()) == ["diagonals"]
    q = dinv.physics.StructuredRandom((2, 8, 12), (2, 5, 7), n_layers=2.5, rng=torch.Generator().manual_seed(1))
    assert torch.equal(p.diagonals, q.diagonals)
    assert dinv.physics.StructuredRandom((12,), (12,), n_layers=2).mode is None
    for tag in [str(t) for t in GOLD["cs_tags"]] + ["doc"]:
        m, img, cw = int(GOLD[f"{tag}_m"]), tuple(int(v) for v in GOLD[f"{tag}_img"]), bool(GOLD[f"{tag}_cw"])
        c = dinv.physics.CompressedSensing(m=m, img_size=img, channelwise=cw)
        assert sorted(c.state_dict().keys()) == [str(k) for k in GOLD[f"{tag}_keys"]]
        sd = {k: torch.from_numpy(GOLD[f"{tag}_sd__{k}"]) for k in c.state_dict()}
        c.load_state_dict(sd)
        assert torch.equal(c._A, sd["_A"]) and torch.equal(c._A_adjoint, sd["_A"].t()) and torch.equal(c._A_dagger, sd["_A_dagger"])
        assert c._A_adjoint.data_ptr() == c._A.data_ptr() and not c._A_adjoint.is_contiguous()     # a view, as in the reference
    # the host pseudo-inverse, and the reference's own matrix for the same seed
    c = dinv.physics.CompressedSensing(m=80, img_size=(1, 6, 6), rng=torch.Generator().manual_seed(80))
    assert torch.equal(c._A, torch.from_numpy(GOLD["cs80_sd___A"]))
    assert torch.allclose(c._A_dagger @ c._A, torch.eye(36), atol=1e-5)


def test_cpu_tensors_raise():
    from deepinv_amd.hip import HipExtensionError

    with pytest.raises(HipExtensionError):
        dinv.physics.functional.dst1(torch.randn(3, 12))
    p = dinv.physics.StructuredRandom((2, 8, 12), (2, 5, 7), n_layers=1.5)
    with pytest.raises(HipExtensionError):
        p.A(torch.randn(1, 2, 8, 12))
    with pytest.raises(HipExtensionError):
        p.A_adjoint(torch.randn(1, 2, 5, 7))
    c = dinv.physics.CompressedSensing(m=10, img_size=(1, 3, 3))
    for call, shape in ((c.A, (1, 1, 3, 3)), (c.A_adjoint, (1, 10)), (c.A_dagger, (1, 10))):
        with pytest.raises(HipExtensionError):
            call(torch.randn(shape))


def test_custom_transforms_are_called_in_the_reference_order():
    log = []

    def f(x):
        log.append(("F", float(x.flatten()[0])))
        return x + 1

    def finv(x):
        log.append(("Finv", float(x.flatten()[0])))
        return x + 10

    d = [torch.full((1, 4, 6), 2.0), torch.full((1, 4, 6), 3.0)]
    p = dinv.physics.StructuredRandom((1, 4, 6), (1, 2, 4), n_layers=2.5, transform_func=f, transform_func_inv=finv, diagonals=d)
    y = p.A(torch.zeros(1, 1, 4, 6))
    # F(0) = 1; D0: 2, F: 3; D1: 9, F: 10; trim
    assert log == [("F", 0.0), ("F", 2.0), ("F", 9.0)] and tuple(y.shape) == (1, 1, 2, 4) and float(y[0, 0, 0, 0]) == 10.0
    log.clear()
    x = p.A_adjoint(torch.ones(1, 1, 2, 4))
    # centre: Finv(1) = 11, D1: 33; Finv: 43, D0: 86; the half layer Finv: 96.  padded border: Finv(0) = 10, 30; 40, 80; 90
    assert [k for k, _ in log] == ["Finv"] * 3 and tuple(x.shape) == (1, 1, 4, 6)
    assert float(x[0, 0, 1, 1]) == 96.0 and float(x[0, 0, 0, 0]) == 90.0


def test_adjoint_stays_a_view_after_load_state_dict():
    from deepinv_amd.physics.phase_retrieval import _RandomLinear

    for cls, conj in ((dinv.physics.CompressedSensing, False), (_RandomLinear, True)):
        # a copying load writes into the view; an assigning load hands every buffer a storage of its own, and only the re-tie
        # after the load makes _A_adjoint a view of the new _A again
        for assign in (False, True):
            src = cls(m=10, img_size=(2, 3, 3), rng=torch.Generator().manual_seed(3))
            dst = cls(m=10, img_size=(2, 3, 3))
            # as a checkpoint read from disk arrives: every tensor with a storage of its own
            dst.load_state_dict({k: v.clone() for k, v in src.state_dict().items()}, assign=assign)
            assert torch.equal(dst._A, src._A) and torch.equal(dst._A_adjoint, src._A.conj().T)
            assert dst._A_adjoint.data_ptr() == dst._A.data_ptr() and dst._A_adjoint.is_conj() == conj, (cls.__name__, assign)
            assert list(dst.state_dict()) == list(src.state_dict())
