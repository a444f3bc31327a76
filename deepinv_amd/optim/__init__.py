from .potential import Potential
from .distance import Distance, L2Distance, PoissonLikelihoodDistance, L1Distance, LogPoissonLikelihoodDistance, AmplitudeLossDistance
from .data_fidelity import DataFidelity, L2, ZeroFidelity, PoissonLikelihood, L1, LogPoissonLikelihood, AmplitudeLoss
from .prior import Prior, PnP, ZeroPrior, TVPrior, TVL1Prior
from .optim_iterators import (OptimIterator, fStep, gStep, PGDIteration, HQSIteration)
from .fixed_point import FixedPoint
from .optimizers import BaseOptim, PGD, HQS, optim_builder, create_iterator, BacktrackingConfig
from .linear import conjugate_gradient, least_squares, least_squares_implicit_backward, dot
from .linear_solvers import lsqr, bicgstab, minres
from .dpir import DPIR, get_DPIR_params
from .phase_retrieval import (default_preprocessing, correct_global_phase, cosine_similarity, spectral_methods,
                              spectral_methods_wrapper)
from . import linear
from . import phase_retrieval
from .epll import EPLL, GaussianMixtureModel
