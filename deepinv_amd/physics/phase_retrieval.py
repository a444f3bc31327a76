"""Phase retrieval ``y = |Bx|^2`` (reference deepinv/physics/phase_retrieval.py:17-539).  ``B`` is a complex64 linear operator:
a dense iid Gaussian matrix on csrc/cdense.hip (hip/cdense.py), a product of 2-D DFTs and unit-modulus diagonals on
csrc/cstructured.hip (hip/cstructured.py), or the shifted probes and 2-D DFTs of ptychography on the same file's ptychography
kernels (hip/ptycho.py).  With any of them the modulus, the weights of ``A_vjp`` and of the spectral initialiser and the residual
of the amplitude loss are epilogues of the forward launch, so ``A`` is one launch and ``A_vjp``, ``AmplitudeLoss.grad`` and one
power iteration are two; the ptychography operator has ``normal_epilogue``, which runs forward, pointwise stage and adjoint per
position inside one workgroup.  With any other ``LinearPhysics`` the methods are the reference's expressions."""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import Tensor

from ..hip import cdense as hcd
from ..hip import cstructured as hcs
from ..hip import epilogue as hep
from ..hip import ptycho as hpt
from .compressed_sensing import _GaussianMatrix
from .forward import LinearPhysics, Physics
from .structured_random import _changes, compare


def _real_like(t, shape) -> bool:
    return isinstance(t, Tensor) and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape)


class _RandomLinear(_GaussianMatrix):
    """the linear operator of :class:`RandomPhaseRetrieval`: the reference's ``CompressedSensing(dtype=torch.cfloat)`` with its
    buffers ``_A``, ``_A_dagger``, ``_A_adjoint`` and ``initial_random_state``.  ``_A_adjoint`` is the view ``_A.conj().T`` and
    the kernel reads it in place: the device holds one copy of the matrix.  The pseudo-inverse is computed in complex128."""

    _dtype, _pinv_dtype = torch.cfloat, torch.complex128
    _refusal = "RandomPhaseRetrieval runs in torch.cfloat on the complex dense kernel, got dtype {dtype}"
    _product = staticmethod(hcd.apply)

    def __init__(self, m: int, img_size, channelwise: bool = False, dtype: torch.dtype = torch.cfloat, device="cpu",
                 rng: torch.Generator = None, **kwargs):
        super().__init__(m, img_size, channelwise, dtype, device, rng, **kwargs)

    def measurement_shape(self, x):
        N, C = x.shape[:2]
        return (N, C, self._A.shape[0]) if self.channelwise else (N, self._A.shape[0])

    def apply_epilogue(self, x: Tensor, epilogue: int, aux=None, eps: float = 1e-12) -> Tensor:
        """``B x`` through an epilogue of hip/epilogue.py, in the shape of the measurements"""
        x, shaped = self._rows(x)
        if aux is not None:
            aux = aux.reshape(x.shape[0], -1)
        return shaped(hcd.apply(x, self._A, epilogue, aux, eps))


def generate_diagonal(shape: tuple, mode: str = "uniform_phase", dtype=torch.cfloat, device="cpu"):
    """a random unit-modulus diagonal, the reference's own draw (structured_random.py:95-98): ``exp(2 pi i u)`` with ``u``
    uniform, drawn from torch's default generator on the host"""
    if mode != "uniform_phase":
        raise ValueError(f"Unsupported mode: {mode}")
    diag = torch.rand(shape)
    diag = 2 * np.pi * diag
    diag = torch.exp(1j * diag)
    return diag.to(dtype).to(device)


class _StructuredLinear(LinearPhysics):
    """the linear operator of :class:`StructuredRandomPhaseRetrieval`: the reference's ``StructuredRandom`` with the orthonormal
    ``fft2`` / ``ifft2`` as transforms and complex64 diagonals in the buffer ``diagonals`` ``[L, C, H, W]`` of the working size
    (the larger of ``img_size`` and ``output_size``).  ``A`` and ``A_adjoint`` are one launch each for any number of layers
    while the working plane fits the LDS of a workgroup (:func:`deepinv_amd.hip.cstructured.fits`); larger planes take the
    composed device path, which computes the same."""

    def __init__(self, img_size, output_size, n_layers=1, diagonals=None, device="cpu", **kwargs):
        super().__init__(device=device, **kwargs)
        if len(img_size) != 3 or len(output_size) != 3:
            raise ValueError(f"img_size and output_size must be (C, H, W), got {tuple(img_size)} and {tuple(output_size)}")
        self.mode = compare(img_size, output_size)
        self.img_size = img_size
        self.output_size = output_size
        self.n_layers = n_layers
        L = math.floor(n_layers)
        work = (int(img_size[0]), max(int(img_size[1]), int(output_size[1])), max(int(img_size[2]), int(output_size[2])))
        if diagonals is None:
            raise ValueError("the diagonals are required: a tensor [layers, C, H, W] of the working size, or a list of its layers")
        if isinstance(diagonals, (list, tuple)):
            diagonals = torch.stack(list(diagonals), dim=0) if len(diagonals) else torch.zeros((0, *work), dtype=torch.cfloat, device=device)
        if diagonals.dtype != torch.cfloat:
            raise TypeError(f"the diagonals must be complex64, got {diagonals.dtype}; convert them with .to(torch.cfloat)")
        if diagonals.shape[0] < L or tuple(diagonals.shape[1:]) != work:
            raise ValueError(f"the diagonals must have shape [{L}, {', '.join(map(str, work))}] (the working size: the larger of "
                             f"img_size and output_size), got {tuple(diagonals.shape)}")
        self.register_buffer("diagonals", diagonals)
        self.to(device)

    def _geometry(self, adjoint):
        C, H, W = (int(s) for s in self.img_size)
        _, Ho, Wo = (int(s) for s in self.output_size)
        top, _, left, _ = _changes(self.img_size, self.output_size)
        work = (max(H, Ho), max(W, Wo))
        a, b = ((Ho, Wo), (H, W)) if adjoint else ((H, W), (Ho, Wo))
        return a, b, work, top, left, C

    def measurement_shape(self, x):
        return (*x.shape[:-2], int(self.output_size[1]), int(self.output_size[2]))

    def _run(self, x, adjoint, epilogue=hep.NONE, aux=None, eps=1e-12):
        L = math.floor(self.n_layers)
        half = self.n_layers - L == 0.5
        geom = self._geometry(adjoint)
        (h_in, w_in), (h_out, w_out) = geom[0], geom[1]
        if x.dim() < 3 or tuple(x.shape[-2:]) != (h_in, w_in) or x.shape[-3] != self.img_size[0]:
            raise ValueError(f"expected an input [..., {self.img_size[0]}, {h_in}, {w_in}], got shape {tuple(x.shape)}")
        lead = x.shape[:-2]
        if aux is not None:
            aux = aux.reshape(-1, h_out, w_out)
        out = hcs.apply(x.reshape(-1, h_in, w_in), self.diagonals[:L], geom, L, half, adjoint, epilogue, aux, eps)
        return out.reshape(*lead, h_out, w_out)

    def apply_epilogue(self, x: Tensor, epilogue: int, aux=None, eps: float = 1e-12) -> Tensor:
        """``B x`` through an epilogue of hip/cstructured.py, in the shape of the measurements"""
        return self._run(x, False, epilogue, aux, eps)

    def A(self, x: Tensor, *args, **kwargs) -> Tensor:
        return self._run(x, False)

    def A_adjoint(self, y: Tensor, *args, **kwargs) -> Tensor:
        return self._run(y.type(torch.cfloat), True)


class PtychographyLinearOperator(LinearPhysics):
    r"""
    The linear operator of ptychography (phase_retrieval.py:317-430): :math:`B = [B_1; \dots; B_{n_{img}}]`,
    :math:`B_l = F \text{diag}(p_l)` with :math:`F` the orthonormal 2-D DFT and :math:`p_l` the probe shifted to position
    :math:`l`, zero where the shift left the plane.  Same signature, buffers (``shifts``, ``init_probe``, ``probe`` of shape
    ``[1, n_img, H, W]``) and state-dict keys as the reference; the probe stack is built once, on the host, with the reference's
    own torch expressions, so the buffer is bit-identical to the reference's.  The kernels read ``probe`` where it lies at every
    call, float32 or complex64: writing to the buffer changes the operator, as in the reference.

    ``A`` fans an image out to its ``n_img`` diffraction planes in one launch; ``A_adjoint`` and :meth:`normal_epilogue` sum over
    the positions inside the kernel (:mod:`deepinv_amd.hip.ptycho`), while the plane fits the LDS of a workgroup
    (:func:`deepinv_amd.hip.cstructured.fits`, squares up to 99 x 99); larger planes take the composed device path.

    Deviation from the reference: ``A_adjoint`` multiplies by the **conjugate** of the probe.  The reference multiplies by the probe
    itself (phase_retrieval.py:395), which is the adjoint for real probes only.  The two coincide for every probe ``build_probe``
    makes; for a complex probe this class computes the true adjoint, which ``A_vjp``, the amplitude-loss gradient and the spectral
    method need.

    Like the reference, the operator works for ``img_size[0] == 1`` only (the reference's broadcast of the probe stack against a
    multi-channel image fails); another channel count raises ``ValueError``.

    :param tuple img_size: shape (1, H, W) of inputs.
    :param None, torch.Tensor probe: probe of shape ``img_size``, float32 or complex64; ``None`` is the disk of radius 10 of
        :func:`build_probe`.
    :param None, torch.Tensor shifts: integer shifts ``[n_img, 2]``; ``None`` is :func:`generate_shifts` with ``n_img = 25``.
    :param str device: device of the buffers.
    """

    def __init__(self, img_size, probe=None, shifts=None, device="cpu", **kwargs):
        super().__init__(**kwargs)
        if len(img_size) != 3 or int(img_size[0]) != 1:
            raise ValueError(f"ptychography works for img_size = (1, H, W) only, as the reference's operator does (its probe stack "
                             f"[1, n_img, H, W] does not broadcast against more channels); got {tuple(img_size)}")
        self.img_size = img_size
        if shifts is None:
            self.n_img = 25
            shifts = generate_shifts(img_size=img_size, n_img=self.n_img)
        else:
            self.n_img = len(shifts)
        # the stack is built on the host with the reference's expressions and moved once
        self.register_buffer("shifts", torch.as_tensor(shifts).cpu())
        if probe is None:
            probe = build_probe(img_size=img_size, type="disk", probe_radius=10, device="cpu")
        probe = probe.detach().cpu()
        if probe.dtype not in (torch.float32, torch.cfloat):
            raise TypeError(f"the probe must be float32 or complex64, got {probe.dtype}")
        if tuple(probe.shape) != tuple(int(s) for s in img_size):
            raise ValueError(f"the probe must have the shape of the image {tuple(img_size)}, got {tuple(probe.shape)}")
        self.register_buffer("init_probe", probe.clone())
        probe = probe / self.get_overlap_img(self.shifts).mean().sqrt()
        probe = torch.cat([self.shift(probe, x_shift, y_shift) for x_shift, y_shift in self.shifts], dim=0).unsqueeze(0)
        self.register_buffer("probe", probe)
        self.to(device)

    def measurement_shape(self, x):
        return (x.shape[0], self.n_img, int(self.img_size[1]), int(self.img_size[2]))

    def _image(self, x):
        H, W = int(self.img_size[1]), int(self.img_size[2])
        if x.dim() != 4 or tuple(x.shape[1:]) != (1, H, W):
            raise ValueError(f"expected an input [batch, 1, {H}, {W}], got shape {tuple(x.shape)}")
        return x.reshape(-1, H, W)

    def apply_epilogue(self, x: Tensor, epilogue: int, aux=None, eps: float = 1e-12, group: int = 0) -> Tensor:
        """``B x`` through an epilogue of hip/ptycho.py, in the shape of the measurements"""
        return hpt.apply(self._image(x), self.probe, hpt.FORWARD, epilogue, aux, eps, group)

    def normal_epilogue(self, x: Tensor, epilogue: int, aux, eps: float = 1e-12, group: int = 0) -> Tensor:
        """``B^H f(B x, aux)`` with ``f`` the ``WEIGHT`` or ``AMPLITUDE`` epilogue, without the ``n_img``-fold intermediate: what
        ``A_adjoint(apply_epilogue(x, epilogue, aux, eps))`` computes, position by position inside the workgroup"""
        return hpt.apply(self._image(x), self.probe, hpt.NORMAL, epilogue, aux, eps, group).unsqueeze(1)

    def A(self, x: Tensor, **kwargs) -> Tensor:
        return self.apply_epilogue(x, hep.NONE)

    def A_adjoint(self, y: Tensor, group: int = 0, **kwargs) -> Tensor:
        return hpt.apply(y.type(torch.cfloat), self.probe, hpt.ADJOINT, hep.NONE, None, 0.0, group).unsqueeze(1)

    def shift(self, x, x_shift, y_shift, pad_zeros=True):
        """``x`` rolled by (``x_shift``, ``y_shift``) along the last two axes, with zeros where it wrapped (phase_retrieval.py:397-418)"""
        x_shift, y_shift = int(x_shift), int(y_shift)
        x = torch.roll(x, (x_shift, y_shift), dims=(-2, -1))
        if pad_zeros:
            if x_shift < 0:
                x[..., x_shift:, :] = 0
            elif x_shift > 0:
                x[..., 0:x_shift, :] = 0
            if y_shift < 0:
                x[..., :, y_shift:] = 0
            elif y_shift > 0:
                x[..., :, 0:y_shift] = 0
        return x

    def get_overlap_img(self, shifts):
        """the summed intensity of the shifted initial probes, whose mean normalises the probe (phase_retrieval.py:420-430)"""
        overlap_img = torch.zeros_like(self.init_probe, dtype=torch.float32)
        for x_shift, y_shift in shifts:
            overlap_img += torch.abs(self.shift(self.init_probe, x_shift, y_shift)) ** 2
        return overlap_img


def fused_operator(physics):
    """the linear operator of a phase-retrieval physics when its epilogues are kernels, else None"""
    B = getattr(physics, "B", None)
    return B if isinstance(B, (_RandomLinear, _StructuredLinear, PtychographyLinearOperator)) else None


class PhaseRetrieval(Physics):
    r"""
    :math:`A(x) = |Bx|^2` with :math:`B` a :class:`deepinv_amd.physics.LinearPhysics` (phase_retrieval.py:17-104).

    :param deepinv_amd.physics.LinearPhysics B: the linear forward operator.
    """

    def __init__(self, B: LinearPhysics, **kwargs):
        super().__init__(**kwargs)
        self.name = "Phase Retrieval"
        self.B = B

    def A(self, x: Tensor, **kwargs) -> Tensor:
        B = fused_operator(self)
        if B is not None:
            return B.apply_epilogue(x, hep.ABS2)
        return self.B(x, **kwargs).abs().square()

    def A_dagger(self, y: Tensor, **kwargs) -> Tensor:
        """an initial reconstruction by the spectral method (:func:`deepinv_amd.optim.phase_retrieval.spectral_methods`)"""
        from ..optim.phase_retrieval import spectral_methods

        return spectral_methods(y, self, **kwargs)

    def A_adjoint(self, y: Tensor, **kwargs) -> Tensor:
        return self.B_adjoint(y, **kwargs)

    def B_adjoint(self, y: Tensor, **kwargs) -> Tensor:
        return self.B.A_adjoint(y, **kwargs)

    def B_dagger(self, y):
        """the linear pseudo-inverse of :math:`B`"""
        return self.B.A_dagger(y)

    def forward(self, x, **kwargs):
        return self.sensor(self.noise(self.A(x, **kwargs)))

    def A_vjp(self, x, v):
        r""":math:`2 \overline{B}^{\top} \text{diag}(Bx) v`"""
        B = fused_operator(self)
        if B is not None and _real_like(v, B.measurement_shape(x)):
            if hasattr(B, "normal_epilogue"):
                return 2 * B.normal_epilogue(x, hep.WEIGHT, v)
            return 2 * self.B_adjoint(B.apply_epilogue(x, hep.WEIGHT, v))
        return 2 * self.B_adjoint(self.B(x) * v)

    def release_memory(self):
        del self.B
        torch.cuda.empty_cache()
        return


class RandomPhaseRetrieval(PhaseRetrieval):
    r"""
    Random phase retrieval with :math:`B_{i,j} \sim \mathcal{N}(0, \frac{1}{2m}) + \mathrm{i} \mathcal{N}(0, \frac{1}{2m})`
    (phase_retrieval.py:107-180).  Same signature, buffers and state-dict keys (``B._A``, ``B._A_adjoint``, ``B._A_dagger``,
    ``B.initial_random_state``, ``initial_random_state``) as the reference, so ``load_state_dict`` of a reference state dict
    works.  The matrix is the reference's own draw; the pseudo-inverse is computed once at construction, on the host in
    complex128, and rounded to complex64.  ``dtype`` other than ``torch.cfloat`` raises ``NotImplementedError``.

    :param int m: number of measurements.
    :param tuple img_size: shape (C, H, W) of inputs.
    :param bool channelwise: channels are processed independently with the same matrix.
    :param torch.dtype dtype: ``torch.cfloat``.
    :param str device: device of the matrix.
    :param torch.Generator rng: generator of the matrix, on ``device``.
    """

    def __init__(self, m, img_size, channelwise=False, dtype=torch.cfloat, device="cpu", rng: torch.Generator = None, **kwargs):
        self.m = m
        self.img_size = img_size
        self.channelwise = channelwise
        self.dtype = dtype
        if rng is None:
            self.rng = torch.Generator(device=device)
        else:
            if torch.device(rng.device).type != torch.device(device).type or (
                    torch.device(device).index is not None and rng.device.index is not None
                    and rng.device.index != torch.device(device).index):
                raise ValueError("The random generator is not on the same device as the Physics Generator. Got random generator on "
                                 f"{rng.device} and the Physics Generator on {device}.")
            self.rng = rng
        B = _RandomLinear(m=m, img_size=img_size, channelwise=channelwise, dtype=dtype, device=device, rng=self.rng)
        super().__init__(B, **kwargs)
        self.register_buffer("initial_random_state", self.rng.get_state())
        self.name = "Random Phase Retrieval"
        self.to(device)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        key = prefix + "initial_random_state"
        if key in state_dict and state_dict[key].shape != self.initial_random_state.shape:
            self.initial_random_state = state_dict[key].clone().to(self.initial_random_state.device)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def get_A_squared_mean(self):
        return self.B._A.var() + self.B._A.mean() ** 2


class StructuredRandomPhaseRetrieval(PhaseRetrieval):
    r"""
    :math:`A(x) = |\prod_{i=1}^N (F D_i) x|^2` with :math:`F` the orthonormal 2-D DFT and :math:`D_i` diagonals of unit modulus
    and uniform random phase; ``n_layers = N + 0.5`` applies one more :math:`F` first (phase_retrieval.py:183-314).  Oversampling
    zero-pads the input to the output shape, undersampling trims the output, both centred.  Same signature as the reference;
    the state-dict key is ``B.diagonals``.  One launch per ``A`` / ``B`` / ``B_adjoint`` for any ``n_layers`` while the working
    plane fits the LDS of a workgroup (:func:`deepinv_amd.hip.cstructured.fits`), the composed device path above that.

    :param tuple img_size: shape (C, H, W) of inputs.
    :param tuple output_size: shape (C, H, W) of outputs.
    :param float n_layers: number of layers :math:`N`, or :math:`N + 0.5`.
    :param str transform: ``"fft"``.
    :param str diagonal_mode: ``"uniform_phase"``.
    :param bool shared_weights: the same diagonal in every layer.
    :param torch.dtype dtype: ``torch.cfloat``.
    :param str device: device of the physics.
    """

    def __init__(self, img_size: tuple, output_size: tuple, n_layers: int, transform="fft", diagonal_mode="uniform_phase",
                 shared_weights=False, dtype=torch.cfloat, device="cpu", **kwargs):
        if dtype != torch.cfloat:
            raise NotImplementedError(f"StructuredRandomPhaseRetrieval runs in torch.cfloat on the fused FFT-layer kernel, got dtype {dtype}")
        if transform != "fft":
            raise ValueError(f"Unimplemented transform: {transform}")
        if not (n_layers % 1 == 0.5 or n_layers % 1 == 0):
            raise ValueError("n_layers must be an integer or an integer plus 0.5")
        if n_layers < 0.5:
            raise ValueError("n_layers must be at least 0.5: the operator needs one transform")
        if output_size is None:
            output_size = img_size
        self.img_size = img_size
        self.output_size = output_size
        self.n = torch.prod(torch.tensor(self.img_size))
        self.m = torch.prod(torch.tensor(self.output_size))
        self.oversampling_ratio = self.m / self.n
        self.n_layers = n_layers
        self.structure = self.get_structure(self.n_layers)
        self.shared_weights = shared_weights
        self.dtype = dtype
        self.mode = compare(img_size, output_size)
        shape = tuple(self.output_size) if self.mode == "oversampling" else tuple(self.img_size)
        L = math.floor(self.n_layers)
        if not shared_weights:
            diagonals = [generate_diagonal(shape, diagonal_mode, self.dtype, device) for _ in range(L)]
        else:
            diagonals = [generate_diagonal(shape, diagonal_mode, self.dtype, device)] * L
        B = _StructuredLinear(img_size=self.img_size, output_size=self.output_size, n_layers=self.n_layers, diagonals=diagonals,
                              device=device)
        super().__init__(B, **kwargs)
        self.name = "Structured Random Phase Retrieval"
        self.to(device)

    @property
    def diagonals(self):
        """the list of diagonals, one per layer: views of the buffer ``B.diagonals``"""
        return [self.B.diagonals[i] for i in range(math.floor(self.n_layers))]

    def B_dagger(self, y):
        return self.B.A_adjoint(y)

    def get_A_squared_mean(self):
        if self.n_layers == 0.5:
            print("warning: computing the mean of the squared operator for a single Fourier transform.")
            return None
        return self.diagonals[0].var() + self.diagonals[0].mean() ** 2

    @staticmethod
    def get_structure(n_layers) -> str:
        """the structure of the operator as a string, e.g. ``"FDFD"``"""
        return "FD" * math.floor(n_layers) + "F" * (n_layers % 1 == 0.5)


class Ptychography(PhaseRetrieval):
    r"""
    :math:`A(x) = |Bx|^2` with :math:`B` a :class:`PtychographyLinearOperator` (phase_retrieval.py:433-485): the intensities of the
    diffraction patterns of the image under a probe at ``n_img`` positions.  Same signature and state-dict keys (``B.shifts``,
    ``B.init_probe``, ``B.probe``) as the reference.  ``B_adjoint`` multiplies by the conjugate of the probe, which differs from
    the reference for complex probes only (see :class:`PtychographyLinearOperator`).  ``B_dagger`` is not provided.

    :param tuple img_size: shape (1, H, W) of inputs.
    :param None, torch.Tensor probe: probe of shape ``img_size``; ``None`` is the disk of :func:`build_probe`.
    :param None, torch.Tensor shifts: shifts ``[n_img, 2]``; ``None`` is :func:`generate_shifts`.
    :param str device: device of the physics.

    >>> physics = Ptychography(img_size=(1, 64, 64), device="cuda")
    >>> x = torch.randn((1, 1, 64, 64), dtype=torch.cfloat, device="cuda")
    >>> physics(x).shape  # 25 probe positions by default
    torch.Size([1, 25, 64, 64])
    """

    def __init__(self, img_size=None, probe=None, shifts=None, device="cpu", **kwargs):
        B = PtychographyLinearOperator(img_size=img_size, probe=probe, shifts=shifts, device=device)
        self.img_size = img_size
        super().__init__(B, **kwargs)
        self.name = "Ptychography_PR"
        self.to(device)

    @property
    def probe(self):
        return self.B.probe

    @property
    def shifts(self):
        return self.B.shifts


def build_probe(img_size, type="disk", probe_radius=10, device="cpu"):
    """a probe of shape ``img_size``: for ``"disk"``, one inside the centred disk of ``probe_radius`` and zero outside
    (phase_retrieval.py:488-511)"""
    if type == "disk" or type is None:
        x = torch.arange(img_size[1], dtype=torch.float64)
        y = torch.arange(img_size[2], dtype=torch.float64)
        X, Y = torch.meshgrid(x, y, indexing="ij")
        probe = torch.zeros(tuple(img_size))
        probe[torch.sqrt((X - img_size[1] // 2) ** 2 + (Y - img_size[2] // 2) ** 2).unsqueeze(0).expand(img_size[0], -1, -1)
              < probe_radius] = 1
    else:
        raise NotImplementedError(f"Probe type {type} not implemented")
    return probe.to(device)


def generate_shifts(img_size, n_img: int = 25, fov: int = None) -> Tensor:
    """the ``n_img`` probe shifts of a square grid across the field of view, ``[n_img, 2]`` int32 (phase_retrieval.py:514-539)"""
    if fov is None:
        fov = img_size[-1]
    start_shift = -fov // 2
    end_shift = fov // 2
    if n_img != int(np.sqrt(n_img)) ** 2:
        raise ValueError("n_img needs to be a perfect square")
    side_n_img = int(np.sqrt(n_img))
    shifts = torch.linspace(start_shift, end_shift, side_n_img).to(torch.int32)
    y_shifts, x_shifts = torch.meshgrid(shifts, shifts, indexing="ij")
    return torch.concatenate([x_shifts.reshape(n_img, 1), y_shifts.reshape(n_img, 1)], dim=1)
