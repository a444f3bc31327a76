"""GaussianMixtureModel, EPLL and EPLLDenoiser through the product's Python layers on the host emulation of the kernel sources
(tests/emu, emu_backend), against the goldens of the real reference (tests/golden/epll.npz): the checks of tests/epll_cases.py,
and - through the emulation's launch log - that a denoising step is exactly three launches.  tests/test_epll_gpu.py runs the same
checks on the device."""
import pytest
import torch

import epll_cases as EC
from emu_backend import emu_backend

CPU = torch.device("cpu")


def test_mixture_on_rows_against_reference():
    with emu_backend():
        EC.check_rows(CPU)


@pytest.mark.parametrize("tag", ["den_a", "den_b"])
def test_denoiser_against_reference(tag):
    with emu_backend():
        EC.check_denoiser(tag, CPU)


def test_epll_blur_against_reference():
    with emu_backend():
        EC.check_blur(CPU)


def test_pnp_pgd_runs():
    with emu_backend():
        EC.check_pnp(CPU)


def test_denoising_step_is_three_launches():
    with emu_backend() as emu:
        l = emu._cdll
        den = EC.denoiser("a", CPU)
        y, sigma = EC.t("den_a_y", CPU), EC.t("den_a_sigma", CPU)
        l.dinv_emu_launch_log_reset()
        den(y, sigma, betas=[40.0])
        got = [l.dinv_emu_launch_log_name(i).decode() for i in range(l.dinv_emu_launch_log_count())]
        assert got == ["(gmm_score_kernel<true, 1>)", "gmm_estimate_kernel", "gmm_aggregate_kernel"], got
        l.dinv_emu_launch_log_reset()
        den(y, sigma)
        assert l.dinv_emu_launch_log_count() == 15
