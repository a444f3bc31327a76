"""TEST INFRASTRUCTURE: run the PRODUCT's Python layer (deepinv_amd.physics / optim / ...) on CPU tensors by pointing its
ctypes binding at tests/emu/libdeepinv_amd_emu.so - the product's kernel SOURCES compiled for the host (tests/emu).

    with emu_backend():
        physics = deepinv_amd.physics.MultiCoilMRI(..., device="cpu")
        y = physics.A(x)            # csrc/mri.hip executed by the fiber emulation

The product itself has no CPU path (hip.require_hip raises for CPU tensors and hip.lib() loads only the gfx950 library); this
hook exists so that the GPU-less build container can drive the real deepinv optimizers over the product's operator objects
(tests/test_dropin_reference.py).  Small problems only: a kernel launch costs seconds."""
import contextlib
import ctypes

import torch

import emu_lib


@contextlib.contextmanager
def emu_backend():
    import deepinv_amd.hip as H
    import deepinv_amd.hip.elementwise as EW

    emu = emu_lib.guarded_lib()                      # builds the emulation library if needed

    def require(*tensors):
        dev = None
        for t in tensors:
            if t is None:
                continue
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise H.HipExtensionError(f"operands on different devices: {dev} vs {t.device}")
        return dev

    def eligible_on_host(*tensors):   # the fast-path predicate of the loop algebra with "on the HIP device" read as "on the host"
        for t in tensors:
            if t is None:
                continue
            if not (isinstance(t, torch.Tensor) and not t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                return False
            if (torch.is_grad_enabled() and t.requires_grad) or t.data_ptr() % 16:
                return False
        return True

    # every module of the package took `from . import require_hip, stream_ptr` by name; lib() everywhere returns hip._lib
    patches = {"require_hip": require, "stream_ptr": lambda device: ctypes.c_void_p(0)}
    swaps = [(m, name, fn) for m in emu_lib.hip_modules() for name, fn in patches.items() if hasattr(m, name)]
    swaps += [(H, "_lib", emu), (EW, "eligible", eligible_on_host), (torch.cuda, "current_device", lambda: 0)]
    saved = [(m, name, getattr(m, name)) for m, name, _ in swaps]
    plan_cache, plan_host = dict(H._plan_cache), dict(H._plan_host)
    for m, name, fn in swaps:
        setattr(m, name, fn)
    H._plan_cache.clear()
    try:
        yield emu
    finally:
        for m, name, fn in saved:
            setattr(m, name, fn)
        for cache, was in ((H._plan_cache, plan_cache), (H._plan_host, plan_host)):
            cache.clear()
            cache.update(was)
