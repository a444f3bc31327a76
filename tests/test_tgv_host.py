"""Total generalized variation without a GPU: TGVDenoiser exists where deepinv has it, with the reference's defaults and
attributes, and refuses what the package does not support (CPU tensors, non-fp32 or complex input, autograd recording, wrong
ranks) with a clear error."""
import inspect

import pytest
import torch


def test_export_and_signature():
    """deepinv/models/tgv.py:45-71"""
    import deepinv_amd as dinv

    cls = dinv.models.TGVDenoiser
    assert issubclass(cls, dinv.models.Denoiser)
    params = list(inspect.signature(cls.__init__).parameters)
    assert params == ["self", "verbose", "n_it_max", "crit", "x2", "u2", "r2", "ths"]


def test_defaults_match_the_reference():
    import deepinv_amd as dinv

    d = dinv.models.TGVDenoiser()
    assert (d.verbose, d.n_it_max, d.crit, d.restart, d.ths, d.tau, d.rho) == (False, 1000, 1e-5, True, None, 0.01, 1.99)
    assert (d.x2, d.u2, d.r2, d.has_converged) == (None, None, None, False)
    d = dinv.models.TGVDenoiser(verbose=True, n_it_max=7, crit=1e-3, ths=0.2)
    assert (d.verbose, d.n_it_max, d.crit, d.ths) == (True, 7, 1e-3, 0.2)


BAD = [(torch.randn(1, 1, 8, 8, dtype=torch.float64), TypeError),
       (torch.randn(1, 1, 8, 8, dtype=torch.complex64), TypeError),
       (torch.randn(1, 1, 8, 8, dtype=torch.float16), TypeError),
       (torch.randn(1, 1, 8, 8, requires_grad=True), NotImplementedError),
       (torch.randn(1, 1, 8, 8), RuntimeError)]


@pytest.mark.parametrize("x,err", BAD)
def test_denoiser_refuses(x, err):
    import deepinv_amd as dinv

    with pytest.raises(err):
        dinv.models.TGVDenoiser()(x, 0.1)


@pytest.mark.parametrize("x,err", BAD)
def test_epsilon_pair_refuses(x, err):
    import deepinv_amd as dinv

    D = dinv.models.TGVDenoiser
    v = torch.stack([x, x], -1)
    if x.requires_grad:
        v = v.detach().requires_grad_()
    with pytest.raises(err):
        D.epsilon(v)
    with pytest.raises(err):
        D.epsilon_adjoint(torch.cat([v, v], -1))


def test_cpu_error_is_runtime_error_without_fallback():
    """a CPU tensor never computes quietly: RuntimeError, and the instance state stays untouched"""
    import deepinv_amd as dinv

    d = dinv.models.TGVDenoiser(ths=0.1)
    with pytest.raises(RuntimeError, match="HIP device"):
        d(torch.rand(1, 3, 16, 16))
    assert d.x2 is None and d.u2 is None and d.r2 is None and d.restart and not d.has_converged


def test_missing_ths_and_bad_shapes():
    import deepinv_amd as dinv

    D = dinv.models.TGVDenoiser
    with pytest.raises(RuntimeError, match="ths"):
        D()(torch.rand(1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="ths"):
        D(ths=None)(torch.rand(1, 1, 8, 8), ths=None)
    for shape in [(8, 8), (1, 8, 8), (1, 1, 1, 2, 8, 8)]:
        with pytest.raises(ValueError):
            D(ths=0.1)(torch.rand(shape))
    for shape in [(1, 8, 8, 2), (1, 1, 8, 8), (1, 1, 1, 1, 8, 8, 3)]:
        with pytest.raises(ValueError, match="5D or 6D"):
            D.epsilon(torch.rand(shape))
        with pytest.raises(ValueError, match="5D or 6D"):
            D.epsilon_adjoint(torch.rand(shape))
    with pytest.raises(ValueError):
        D.nabla(torch.rand(8, 8))
    with pytest.raises(ValueError):
        D.nabla_adjoint(torch.rand(1, 8, 8, 2))
