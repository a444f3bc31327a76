from .base import Denoiser, Reconstructor
from .drunet import DRUNet
from .tv import TVDenoiser, TVL1Denoiser
from .dncnn import DnCNN
from .tgv import TGVDenoiser
from .anscombe import AnscombeDenoiser, generalized_anscombe_transform, inverse_generalized_anscombe_transform
from .epll import EPLLDenoiser
