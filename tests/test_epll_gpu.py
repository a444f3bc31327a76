"""GaussianMixtureModel, EPLL and EPLLDenoiser on the MI355X against the goldens of the real reference (tests/golden/epll.npz):
the checks of tests/epll_cases.py - parity within 1e-4 relative, bitwise equality of two runs and of a batched call with the
per-image calls, batch_size without effect, the conjugate-gradient path with a BlurFFT physics and PnP-PGD on the denoiser."""
import pytest
import torch

import epll_cases as EC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def test_mixture_on_rows_against_reference():
    EC.check_rows(DEV)


@pytest.mark.parametrize("tag", ["den_a", "den_b"])
def test_denoiser_against_reference(tag):
    EC.check_denoiser(tag, DEV)


def test_epll_blur_against_reference():
    EC.check_blur(DEV)


def test_pnp_pgd_runs():
    EC.check_pnp(DEV)


def test_no_autograd_and_no_cpu_path():
    from deepinv_amd.hip import HipExtensionError

    m = EC.gmm("a", DEV)
    with pytest.raises(NotImplementedError, match="no backward"):
        m(EC.t("rows_x", DEV).requires_grad_())
    with pytest.raises(HipExtensionError):
        EC.gmm("a", "cpu")(EC.t("rows_x", "cpu"))
