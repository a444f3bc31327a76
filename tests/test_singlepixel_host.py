"""Host side of SinglePixelCamera (deepinv_amd/physics/singlepixel.py): the mask builders against the reference's masks in
tests/golden/singlepixel.npz (tests/golden/make_golden_singlepixel.py) element for element, the reference's error and warning
texts, the guards, the state dict, and - where the reference is present - a sweep of every m at two small sizes."""
import os
import warnings

import numpy as np
import pytest
import torch

from deepinv_amd.hip import HipExtensionError
from oracle.ref_shim import reference_available
from deepinv_amd.physics import SinglePixelCamera
from deepinv_amd.physics import singlepixel as sp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "singlepixel.npz")
ORDERINGS = ("sequency", "cake_cutting", "zig_zag", "xy")
SIZES = ((1, 32, 32), (3, 64, 128), (1, 16, 16))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def build(img, m, ordering):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return SinglePixelCamera(m=m, img_size=img, ordering=ordering).mask


@pytest.mark.parametrize("ordering", ORDERINGS)
@pytest.mark.parametrize("img", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_masks_equal_reference(gold, img, ordering):
    n = img[1] * img[2]
    mask = build(img, n // 5, ordering)
    want = gold[f"mask_{'x'.join(map(str, img))}_{ordering}"]
    assert mask.dtype == torch.float32 and tuple(mask.shape) == (1, *img)
    assert np.array_equal(mask.numpy(), want.astype(np.float32))


@pytest.mark.parametrize("img", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_sequency_mask_ends(gold, img):
    """m = 1 keeps the constant pattern alone, m = H W keeps everything"""
    n = img[1] * img[2]
    for m in (1, 16, n):
        want = gold[f"mask_{'x'.join(map(str, img))}_sequency_m{m}"]
        assert np.array_equal(build(img, m, "sequency").numpy(), want.astype(np.float32)), m
        assert int(want.sum()) == m * img[0]


def test_sequency_order_definition():
    """row r of the natural-order matrix has sequency_order^-1(r) sign changes"""
    for n in (2, 8, 64):
        h = torch.ones(1, 1)
        while h.shape[0] < n:
            h = torch.cat((torch.cat((h, h), 1), torch.cat((h, -h), 1)), 0)
        changes = (h[:, 1:] != h[:, :-1]).sum(1)
        order = sp.sequency_order(n)
        assert order.dtype == np.int32 and changes[torch.as_tensor(order.astype(np.int64))].tolist() == list(range(n))
    assert sp.get_permutation_list(8).tolist() == [sp.reverse(sp.gray_decode(k), 3) for k in range(8)]
    assert [sp.gray_decode(k ^ (k >> 1)) for k in range(16)] == list(range(16))
    assert sp.gray_code(4).tolist() == [[0, 0], [0, 1], [1, 1], [1, 0]]


def test_messages():
    with pytest.raises(ValueError, match="Unknown ordering spiral. Available options are: `sequency`, `cake_cutting`, `zig_zag`, `xy`."):
        SinglePixelCamera(m=4, img_size=(1, 8, 8), ordering="spiral")
    with pytest.raises(ValueError, match="image height must be a power of 2"):
        SinglePixelCamera(m=4, img_size=(1, 12, 8))
    with pytest.raises(ValueError, match="image width must be a power of 2"):
        SinglePixelCamera(m=4, img_size=(1, 8, 24))
    with pytest.warns(UserWarning, match="Image height and width must be equal for cake cutting mask."):
        SinglePixelCamera(m=4, img_size=(1, 8, 16), ordering="cake_cutting")


def test_fast_false_raises():
    with pytest.raises(NotImplementedError, match="fast=False"):
        SinglePixelCamera(m=4, img_size=(1, 8, 8), fast=False)


def test_cpu_tensor_raises():
    p = SinglePixelCamera(m=4, img_size=(1, 8, 8))
    x = torch.zeros(1, 1, 8, 8)
    for call in (p.A, p.A_adjoint, p.A_adjoint_A, p.A_A_adjoint, p.A_dagger, p.V, p.V_adjoint, sp.hadamard_1d, sp.hadamard_2d):
        with pytest.raises(HipExtensionError):
            call(x)
    with pytest.raises(HipExtensionError):
        p.prox_l2(x, x, 1.0)
    assert p.U(x) is x and p.U_adjoint(x) is x


def test_attributes_and_state_dict(gold):
    p = SinglePixelCamera(m=100, img_size=(2, 16, 32), ordering="zig_zag")
    assert p.name == "spcamera_m100" and p.img_size == (2, 16, 32) and p.fast is True
    assert sorted(p.state_dict().keys()) == gold["sd_keys"].tolist() == ["initial_random_state", "mask"]
    assert p.initial_random_state.dtype == torch.uint8
    # a state dict written by the reference loads
    q = SinglePixelCamera(m=3, img_size=(2, 16, 32))
    q.load_state_dict({k: torch.from_numpy(gold[f"sd__{k}"]) for k in gold["sd_keys"].tolist()})
    assert torch.equal(q.mask, p.mask)
    # update_parameters replaces the mask
    new = torch.rand(1, 2, 16, 32)
    q.update_parameters(mask=new)
    assert torch.equal(q.mask, new)
    assert SinglePixelCamera(m=3, img_size=(1, 8, 8), dtype=torch.float64).mask.dtype == torch.float64


@pytest.mark.reference
@pytest.mark.skipif(not reference_available(), reason="reference checkout not present")
@pytest.mark.parametrize("img", [(1, 8, 8), (2, 16, 32)], ids=["8x8", "16x32"])
def test_mask_sweep_against_reference(img):
    """all four orderings, every m from 1 to H W"""
    from oracle.ref_shim import import_reference

    import_reference()
    from deepinv.physics import singlepixel as ref

    n = img[1] * img[2]
    assert np.array_equal(sp.sequency_order(n), ref.sequency_order(n))
    assert np.array_equal(sp.cake_cutting_order(n), ref.cake_cutting_order(n))
    assert torch.equal(sp.diagonal_index_matrix(*img[1:]), ref.diagonal_index_matrix(*img[1:]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name in ("sequency_mask", "cake_cutting_mask", "zig_zag_mask", "xy_mask"):
            ours, theirs = getattr(sp, name), getattr(ref, name)
            for m in range(1, n + 1):
                assert torch.equal(ours(img, m), theirs(img, m)), (name, m)
