"""Total variation without a GPU: the public names exist where deepinv has them, and the TV entry points refuse what the
package does not support (CPU tensors, non-fp32 or complex input, autograd recording) with a clear error."""
import pytest
import torch


def test_exports():
    import deepinv_amd as dinv

    assert dinv.models.TVDenoiser and dinv.models.TVL1Denoiser
    assert dinv.optim.TVPrior is dinv.optim.prior.TVPrior and dinv.optim.TVL1Prior is dinv.optim.prior.TVL1Prior
    assert issubclass(dinv.models.TVL1Denoiser, dinv.models.TVDenoiser)
    assert issubclass(dinv.optim.TVPrior, dinv.optim.Prior) and issubclass(dinv.optim.TVL1Prior, dinv.optim.TVPrior)


def test_defaults_match_the_reference():
    """deepinv/models/tv.py:45-71, deepinv/optim/prior.py:485-496"""
    import deepinv_amd as dinv

    d = dinv.models.TVDenoiser()
    assert (d.tau, d.rho, d.n_it_max, d.crit, d.x2, d.u2, d.ths, d.restart) == (0.01, 1.99, 1000, 1e-5, None, None, None, True)
    p = dinv.optim.TVPrior()
    assert p.explicit_prior and isinstance(p.TVModel, dinv.models.TVDenoiser)
    assert (p.TVModel.crit, p.TVModel.n_it_max) == (1e-8, 1000)
    p1 = dinv.optim.TVL1Prior(def_crit=1e-6, n_it_max=50)
    assert isinstance(p1.TVModel, dinv.models.TVL1Denoiser) and (p1.TVModel.crit, p1.TVModel.n_it_max) == (1e-6, 50)
    assert p1.explicit_prior


BAD = [(torch.randn(1, 1, 8, 8, dtype=torch.float64), TypeError),
       (torch.randn(1, 1, 8, 8, dtype=torch.complex64), TypeError),
       (torch.randn(1, 1, 8, 8, dtype=torch.float16), TypeError),
       (torch.randn(1, 1, 8, 8, requires_grad=True), NotImplementedError),
       (torch.randn(1, 1, 8, 8), RuntimeError)]


@pytest.mark.parametrize("x,err", BAD)
def test_denoisers_refuse(x, err):
    import deepinv_amd as dinv

    for cls in (dinv.models.TVDenoiser, dinv.models.TVL1Denoiser):
        with pytest.raises(err):
            cls()(x, 0.1)


@pytest.mark.parametrize("x,err", BAD)
def test_prior_entry_points_refuse(x, err):
    import deepinv_amd as dinv

    p = dinv.optim.TVPrior()
    for f in (p.fn, p.grad, p.nabla, lambda v: p.prox(v, gamma=0.1), dinv.optim.TVL1Prior().fn):
        with pytest.raises(err):
            f(x)
    with pytest.raises(err):
        p.nabla_adjoint(torch.stack([x, x], -1))


def test_cpu_error_is_runtime_error_without_fallback():
    """a CPU tensor never computes quietly: RuntimeError, and the instance state stays untouched"""
    import deepinv_amd as dinv

    d = dinv.models.TVDenoiser(ths=0.1)
    with pytest.raises(RuntimeError, match="HIP device"):
        d(torch.rand(1, 3, 16, 16))
    assert d.x2 is None and d.u2 is None and d.restart


def test_missing_ths_and_bad_shapes():
    import deepinv_amd as dinv

    with pytest.raises(RuntimeError, match="ths"):
        dinv.models.TVDenoiser()(torch.rand(1, 1, 8, 8))
    with pytest.raises(ValueError):
        dinv.models.TVDenoiser.nabla(torch.rand(8, 8))
    with pytest.raises(ValueError):
        dinv.models.TVDenoiser.nabla_adjoint(torch.rand(1, 8, 8, 2))
