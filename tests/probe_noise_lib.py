"""Builder + ctypes loader of the task-noise probe (tests/device_probe/orr_probe_noise.hip) -- test infrastructure only.

A sibling of tests/probe_lib.py (whose machinery - flags, hash file, file lock, atomic rename - it reuses): normal_pair of
csrc/orr_device.h behind two entry points, built once with the flags of the unit that uses it (_lib.HIPCC_FLAGS, orr_kernels_noise.hip),
next to its source; no part of libopenroborl_hip.so, of _lib.DEPS or of the source hash.
"""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

from openroborl_amd import _lib
from tests import probe_lib

SRC = os.path.join(probe_lib.PROBE_DIR, "orr_probe_noise.hip")
LIB = os.path.join(probe_lib.PROBE_DIR, "liborr_probe_noise.so")


def probe_hash():
    h = hashlib.sha256()
    for d in [SRC] + sorted(_lib.DEPS):
        h.update(os.path.basename(d).encode())
        with open(d, "rb") as f:
            h.update(f.read())
    h.update(" ".join(_lib.HIPCC_FLAGS).encode())
    return h.hexdigest()[:32]


def needs_build():
    try:
        with open(LIB + ".hash") as f:
            return f.read().strip() != probe_hash() or not os.path.exists(LIB)
    except OSError:
        return True


def compile_command(out):
    return [_lib.HIPCC] + list(_lib.HIPCC_FLAGS) + ["-I", _lib.CSRC, "-I", os.path.join(probe_lib.ROOT, "include"), "-o", out, SRC]


def build(force=False):
    """Compile the probe for gfx950 (no GPU needed); same locking and renaming as probe_lib.build."""
    import fcntl
    with open(os.path.join(probe_lib.PROBE_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or needs_build():
                tmp = LIB + ".%d.tmp" % os.getpid()
                try:
                    subprocess.check_call(compile_command(tmp))
                    os.replace(tmp, LIB)
                finally:
                    if os.path.exists(tmp):
                        os.remove(tmp)
                with open(LIB + ".hash.tmp", "w") as f:
                    f.write(probe_hash() + "\n")
                os.replace(LIB + ".hash.tmp", LIB + ".hash")
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB


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
    rc = lib().orrp_normal_pair(tin.data_ptr(), tout.data_ptr(), len(x), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("orrp_normal_pair failed: %d" % rc)
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
