"""Operator API mirror of ``deepinv.physics`` for the accelerated hot path."""
from .forward import (Physics, LinearPhysics, DecomposablePhysics, Denoising, adjoint_function, power_method)
from .noise import NoiseModel, ZeroNoise, GaussianNoise, PoissonNoise, PoissonGaussianNoise, LogPoissonNoise
from .mri import MRI, MultiCoilMRI, MRIMixin
from .tomography import Tomography, RampFilter
from .blur import Blur, BlurFFT, Downsampling, SpaceVaryingBlur
from .singlepixel import SinglePixelCamera
from .compressed_sensing import CompressedSensing
from .structured_random import StructuredRandom
from .phase_retrieval import (PhaseRetrieval, Ptychography, PtychographyLinearOperator, RandomPhaseRetrieval,
                              StructuredRandomPhaseRetrieval)
from . import functional
from . import singlepixel
from . import generator
