"""TEST INFRASTRUCTURE: ctypes access to tests/emu/libdeepinv_amd_emu.so, i.e. the product's kernel SOURCES
(deepinv_amd/csrc/*.hip) compiled for the host against a fiber-based emulation of the HIP execution model
(tests/emu/include/hip/hip_runtime.h).  It lets the GPU-less CPU suite execute the real kernel code on small problems
and compare it with the oracle.  The product never loads this library."""
import ctypes
import importlib
import os
import pkgutil
import subprocess

import numpy as np
import torch

import deepinv_amd.hip as H
from deepinv_amd.hip import FftPlan  # noqa: F401  (the structures of include/deepinv_amd.h are the product's classes)
from radon_cases import RadonGeom as _RadonTables
from radon_cases import FanGeom as _FanTables

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_libs = {}


def hip_modules():
    """every module of deepinv_amd.hip, the package first"""
    return [H] + [importlib.import_module(m.name) for m in pkgutil.iter_modules(H.__path__, H.__name__ + ".")]


def _load(target):
    """(the ctypes library, the same behind the product's call wrapper) of one TARGET of tests/emu/Makefile, with every prototype
    the product declares: each hip module's _declare, so that a direct call here goes through the argtypes the product uses"""
    if target not in _libs:
        subprocess.run(["make", "-C", EMU_DIR, "-j8", f"TARGET={target}"], check=True, stdout=subprocess.DEVNULL)
        cdll = ctypes.CDLL(os.path.join(EMU_DIR, target))
        guarded = H._DeviceGuardedLib(cdll)
        for m in hip_modules():
            if hasattr(m, "_declare"):
                H.declare_once(guarded, m._declare)
        cdll.dinv_emu_launch_log_name.restype = cdll.dinv_emu_launch_log_instance.restype = ctypes.c_char_p
        cdll.dinv_emu_lds_probe.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32]
        _libs[target] = cdll, guarded
    return _libs[target]


def lib():
    """the one emulation library"""
    return _load("libdeepinv_amd_emu.so")[0]


def guarded_lib():
    """lib() as the product holds a library (hip._DeviceGuardedLib): what tests/emu_backend.py puts in hip._lib"""
    return _load("libdeepinv_amd_emu.so")[1]


def private_copy():
    """the same objects linked a second time and loaded from a path of their own: a library whose static state (the LDS caps
    raised so far, the launch log) no other test has touched"""
    return _load("libdeepinv_amd_emu_private.so")[0]


def check(rc):
    if rc != 0:
        raise RuntimeError(f"emu lib error {rc}: {lib().dinv_last_error().decode()}")


def p(a):
    """pointer to a numpy array / torch CPU tensor (None -> NULL)"""
    if a is None:
        return ctypes.c_void_p(0)
    if isinstance(a, torch.Tensor):
        assert a.is_contiguous() and a.device.type == "cpu"
        return ctypes.c_void_p(a.data_ptr())
    assert a.flags["C_CONTIGUOUS"]
    return ctypes.c_void_p(a.ctypes.data)


class RadonGeom(_RadonTables):
    """the host tables exactly as deepinv_amd.hip.radon.RadonGeometry builds them, planned by the emulated library"""

    def plan(self, n_img, kw=0):
        """kw = 1, 2, 4, 8 forces the angles per workgroup (dinv_radon_plan_init reads plan.kw on entry), 0 = automatic"""
        pl, blob = self.plan_host(lib(), n_img, kw)
        return pl, blob.numpy()


def radon_forward_tiled(x, geo, norm=None, scale=1.0, kw=0):
    l = lib()
    B, C, W, _ = x.shape
    x = x.contiguous().float()
    d = geo.desc(B * C, scale)
    pl, blob = geo.plan(B * C, kw)
    sino = torch.full((B, C, geo.G, geo.A), float("nan"))
    ws = np.zeros(l.dinv_radon_tiled_workspace_bytes(ctypes.byref(d), 0), np.uint8)
    check(l.dinv_radon_forward_tiled(ctypes.byref(d), ctypes.byref(pl), p(blob), p(x), p(geo.xn), p(geo.cs), p(norm), p(sino),
                                     p(ws), ctypes.c_size_t(ws.size), None))
    return sino, pl


def radon_adjoint_tiled(y, geo, norm=None, scale=1.0):
    l = lib()
    B, C, G, A = y.shape
    y = y.contiguous().float()
    d = geo.desc(B * C, scale)
    x = torch.full((B, C, geo.W, geo.W), float("nan"))
    ws = np.zeros(l.dinv_radon_tiled_workspace_bytes(ctypes.byref(d), 1), np.uint8)
    check(l.dinv_radon_adjoint_tiled(ctypes.byref(d), p(y), p(geo.xn), p(geo.cs), p(norm), p(x), p(ws),
                                     ctypes.c_size_t(ws.size), None))
    return x


def radon_forward_gather(x, geo, scale=1.0):
    l = lib()
    B, C, W, _ = x.shape
    x = x.contiguous().float()
    d = geo.desc(B * C, scale)
    sino = torch.full((B, C, geo.G, geo.A), float("nan"))
    ws = np.zeros(l.dinv_radon_workspace_bytes(ctypes.byref(d), 0), np.uint8)
    check(l.dinv_radon_forward(ctypes.byref(d), p(x), p(geo.xn), p(geo.cs), p(sino), p(ws), ctypes.c_size_t(ws.size), None))
    return sino


def fft_plan(n):
    l = lib()
    plan = FftPlan()
    table = np.zeros(l.dinv_fft_table_bytes(ctypes.c_int32(n)), np.uint8)
    check(l.dinv_fft_plan_init(ctypes.c_int32(n), ctypes.byref(plan), p(table)))
    return plan, table


def ramp_fft(y):
    l = lib()
    B, C, N, A = y.shape
    y = y.contiguous().float()
    P = l.dinv_radon_ramp_padded_size(ctypes.c_int32(N))
    plan, table = fft_plan(P)
    filt = np.zeros(P, np.float32)
    check(l.dinv_radon_ramp_filter_init(ctypes.c_int32(P), p(table), p(filt)))
    out = torch.full_like(y, float("nan"))
    check(l.dinv_radon_ramp_fft(B * C, N, A, P, ctypes.byref(plan), p(table), p(filt), p(y), p(out), None))
    return out


class FanGeom(_FanTables):
    """fan-beam tables from the product's own host code (deepinv_amd.hip.radon.fan_tables: pure torch)"""


def radon_fan_forward(x, geo):
    l = lib()
    B, C, W, _ = x.shape
    x = x.contiguous().float()
    d = geo.desc(B * C)
    sino = torch.full((B, C, geo.n_det, geo.A), float("nan"))
    ws = np.zeros(l.dinv_radon_fan_workspace_bytes(ctypes.byref(d), geo.n_det, 0), np.uint8)
    check(l.dinv_radon_fan_forward(ctypes.byref(d), geo.n_det, p(x), p(geo.xm), p(geo.sc), p(geo.yd), p(geo.cs), p(sino), p(ws),
                                   ctypes.c_size_t(ws.size), None))
    return sino


def radon_fan_adjoint(y, geo):
    l = lib()
    B, C, N, A = y.shape
    y = y.contiguous().float()
    d = geo.desc(B * C)
    x = torch.full((B, C, geo.W, geo.W), float("nan"))
    ws = np.zeros(l.dinv_radon_fan_workspace_bytes(ctypes.byref(d), geo.n_det, 1), np.uint8)
    check(l.dinv_radon_fan_adjoint(ctypes.byref(d), geo.n_det, p(y), p(geo.xm), p(geo.sc), p(geo.yd), p(geo.cs), p(x), p(ws),
                                   ctypes.c_size_t(ws.size), None))
    return x
