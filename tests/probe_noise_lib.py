"""Builder + ctypes loader of the task-noise probe (tests/device_probe/orr_probe_noise.hip) -- test infrastructure only.

A sibling of tests/probe_lib.py (one more ProbeBuilds: flags, hash file, file lock, atomic rename): normal_pair of
csrc/orr_device.h behind two entry points, built once with the flags of the unit that uses it (_lib.HIPCC_FLAGS, orr_kernels_noise.hip),
next to its source; no part of libopenroborl_hip.so, of _lib.DEPS or of the source hash.
"""
import ctypes as C
import functools
import os

import numpy as np

from openroborl_amd import _lib
from tests import probe_lib

SRC = os.path.join(probe_lib.PROBE_DIR, "orr_probe_noise.hip")
LIB = os.path.join(probe_lib.PROBE_DIR, "liborr_probe_noise.so")

_builds = probe_lib.ProbeBuilds(SRC, {"noise": (os.path.basename(LIB), _lib.HIPCC_FLAGS)})
# a single build: the module-level functions take no build name
probe_hash, needs_build = functools.partial(_builds.probe_hash, "noise"), functools.partial(_builds.needs_build, "noise")
compile_command, build = functools.partial(_builds.compile_command, "noise"), functools.partial(_builds.build, "noise")

_lib_handle = None


def lib():
    global _lib_handle
    if _lib_handle is None:
        import torch  # noqa: F401  (first: see _lib.load)
        L = C.CDLL(build())
        L.orrp_normal_pair_sweep.restype = C.c_int
        L.orrp_normal_pair_sweep.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orrp_normal_pair.restype = C.c_int
        L.orrp_normal_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib_handle = L
    return _lib_handle


def normal_pair(ua, ub):
    """normal_pair on the device for float32 arrays ua, ub [n] -> (z0, z1) float32 [n]."""
    import torch
    x = np.ascontiguousarray(np.stack([np.asarray(ua, dtype=np.float32), np.asarray(ub, dtype=np.float32)], axis=1))
    tin = torch.from_numpy(x).to("cuda:0")
    tout = torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda:0")
    probe_lib._launch(lib(), "normal_pair", tin, tout, len(x))
    out = tout.cpu().numpy()
    return out[:, 0], out[:, 1]


def sweep(ub, first=0, count=1 << 24):
    """For each ub[j]: (max |z - z_float64| over ua = i / 2^24, i = first .. first + count - 1; the i of the maximum), then the number of
    non-finite results and the number of ua covered.  The float64 definition is evaluated on the device."""
    import torch
    ub = np.ascontiguousarray(ub, dtype=np.float32)
    t_ub = torch.from_numpy(ub).to("cuda:0")
    out = torch.full((2 * len(ub) + 2,), float("nan"), dtype=torch.float64, device="cuda:0")
    scratch = torch.zeros(len(ub) + 2, dtype=torch.int64, device="cuda:0")
    rc = lib().orrp_normal_pair_sweep(t_ub.data_ptr(), len(ub), int(first), int(count), out.data_ptr(), scratch.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("orrp_normal_pair_sweep failed: %d" % rc)
    o = out.cpu().numpy()
    return o[0:2 * len(ub):2], o[1:2 * len(ub):2].astype(np.int64), int(o[-2]), int(o[-1])
