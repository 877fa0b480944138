"""Builder + ctypes loader of the device-primitive probe (tests/device_probe/orr_probe.hip) -- test infrastructure only.

The probe wraps the device helpers of the env kernels (csrc/orr_device.h, orr_physics.h, orr_task.h) in small kernels of their own,
so that tests/test_gpu_device_primitives.py can compare each helper with a float64 definition.  It is built twice, with the flags
of the two env translation units whose code generation differs (`one`: _lib.HIPCC_FLAGS; `w2`: _lib.HIPCC_FLAGS_W2, -Os and the other
scheduler), next to its source; it is no part of libopenroborl_hip.so, of _lib.DEPS or of the source hash.
"""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

from openroborl_amd import _abi, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PROBE_DIR = os.path.join(HERE, "device_probe")
SRC = os.path.join(PROBE_DIR, "orr_probe.hip")
# The probe mirrors the two units' compiler FLAGS (optimisation level, scheduler), not their macros: it defines neither ORR_TU_STEP_W2 /
# ORR_PARITY (orr_kernels_w2.hip) nor _lib.tuning_defines().  Those select between helpers and pad loops of the step kernel; the
# helpers themselves are the same text in every unit, and the probe instantiates both forms where a unit chooses (WITH_M).
BUILDS = {"one": ("liborr_probe.so", _lib.HIPCC_FLAGS), "w2": ("liborr_probe_w2.so", _lib.HIPCC_FLAGS_W2)}

# entry point -> (words per input record, words per output record, whole waves only?)
SPECS = {
    "joint_sincos": (1, 2, False), "atan2_bf": (2, 1, False), "asin_bf": (1, 1, False), "map_pi": (1, 1, False),
    "q_norm_angle": (4, 1, False), "euler_from_quat": (4, 3, False), "qheading": (4, 1, False), "qslerp": (9, 4, False),
    "q_to_mat": (4, 9, False), "qrot": (7, 3, False), "pick4": (4, 1, False),
    "row_sum16": (1, 1, True), "bcast_lane": (1, 16, True), "dpp_bcast_max0": (1, 12, True), "dpp_contact_triplet": (21, 12, True),
    "part_suffix_sum": (1, 1, True), "part_suffix_sum_inplace": (6, 6, True),
    "part_suffix_sum_first_moment_m0": (7, 4, True), "part_suffix_sum_first_moment_m1": (7, 4, True), "zero_in_lane": (1, 16, True),
    "chol6": (42, 12, False), "chol6_pk": (42, 12, False),
}
INT_ENTRIES = ("philox_block", "time_limit")


class ProbeBuilds:
    """The builds of one probe source: `builds` maps a build name to (library file name, flags).  Every library lies next to the sources
    in PROBE_DIR, with a `.hash` side file that says what it was built from."""

    def __init__(self, src, builds):
        self.src, self.builds = src, builds

    def lib_path(self, build_name):
        return os.path.join(PROBE_DIR, self.builds[build_name][0])

    def probe_hash(self, build_name):
        """What a probe library is built from: its source, everything the env kernels are built from (_lib.DEPS) and the flags."""
        h = hashlib.sha256()
        for d in [self.src] + sorted(_lib.DEPS):
            h.update(os.path.basename(d).encode())
            with open(d, "rb") as f:
                h.update(f.read())
        h.update(" ".join(self.builds[build_name][1]).encode())
        return h.hexdigest()[:32]

    def needs_build(self, build_name):
        so = self.lib_path(build_name)
        try:
            with open(so + ".hash") as f:
                return f.read().strip() != self.probe_hash(build_name) or not os.path.exists(so)
        except OSError:
            return True

    def compile_command(self, build_name, out):
        return [_lib.HIPCC] + list(self.builds[build_name][1]) + ["-I", _lib.CSRC, "-I", os.path.join(ROOT, "include"), "-o", out, self.src]

    def build(self, build_name, force=False):
        """Compile one probe library for gfx950 (no GPU needed).  File lock + atomic rename: concurrent callers never load half a file."""
        import fcntl
        so = self.lib_path(build_name)
        with open(os.path.join(PROBE_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                if force or self.needs_build(build_name):
                    tmp = so + ".%d.tmp" % os.getpid()
                    try:
                        subprocess.check_call(self.compile_command(build_name, tmp))
                        os.replace(tmp, so)
                    finally:
                        if os.path.exists(tmp):
                            os.remove(tmp)
                    with open(so + ".hash.tmp", "w") as f:
                        f.write(self.probe_hash(build_name) + "\n")
                    os.replace(so + ".hash.tmp", so + ".hash")
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
        return so

    def build_all(self, force=False):
        return [self.build(b, force=force) for b in self.builds]


_builds = ProbeBuilds(SRC, BUILDS)
lib_path, probe_hash, needs_build, compile_command = _builds.lib_path, _builds.probe_hash, _builds.needs_build, _builds.compile_command
build, build_all = _builds.build, _builds.build_all

_libs = {}


def declare(L):
    for name in list(SPECS) + list(INT_ENTRIES):
        fn = getattr(L, "orrp_" + name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.orrp_sizeof_config.restype = C.c_int
    assert L.orrp_sizeof_config() == C.sizeof(_abi.OrrConfig)
    return L


def lib(build_name):
    """The probe library of one build, with its ctypes signatures (builds it when missing or stale)."""
    if build_name not in _libs:
        import torch  # noqa: F401  (first: the probe then resolves its HIP symbols against the runtime torch has mapped, see _lib.load)
        _libs[build_name] = declare(C.CDLL(build(build_name)))
    return _libs[build_name]


def _launch(L, name, tin, tout, n):
    import torch
    rc = getattr(L, "orrp_" + name)(tin.data_ptr(), tout.data_ptr(), int(n), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("orrp_%s(n=%d) failed: %d" % (name, n, rc))


def run(build_name, name, x):
    """helper `name` on the float32 records x[n, NIN] (or x[n] for one word per record) -> float32 [n, NOUT] ([n] for one word)."""
    import torch
    nin, nout, wave = SPECS[name]
    x = np.ascontiguousarray(x, dtype=np.float32)
    x2 = x.reshape(len(x), -1)
    assert x2.shape[1] == nin, (name, x.shape)
    n = x2.shape[0]
    assert not wave or (n % 64 == 0 and n >= 128), "whole waves, at least two blocks"
    tin = torch.from_numpy(x2).to("cuda:0")
    tout = torch.full((n, nout), float("nan"), dtype=torch.float32, device="cuda:0")
    _launch(lib(build_name), name, tin, tout, n)
    out = tout.cpu().numpy()
    return out[:, 0] if nout == 1 else out


def run_philox(build_name, seed, robot, episode, block):
    """philox_block for arrays of (seed: uint64, robot, episode, block: uint32) -> float32 [n, 4]"""
    import torch
    seed = np.asarray(seed, dtype=np.uint64)
    n = len(seed)
    rec = np.zeros((n, 6), dtype=np.uint32)
    rec[:, 0] = (seed & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rec[:, 1] = (seed >> np.uint64(32)).astype(np.uint32)
    rec[:, 2] = np.asarray(robot, dtype=np.uint32)
    rec[:, 3] = np.asarray(episode, dtype=np.uint32)
    rec[:, 4] = np.asarray(block, dtype=np.uint32)
    tin = torch.from_numpy(rec.view(np.int32)).to("cuda:0")
    tout = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    _launch(lib(build_name), "philox_block", tin, tout, n)
    return tout.cpu().numpy()


def run_time_limit(build_name, cfg, totals):
    """time_limit(cfg, total) for an array of int64 totals -> int32 [n]"""
    import torch
    totals = np.ascontiguousarray(totals, dtype=np.int64)
    n = len(totals)
    off = (C.sizeof(_abi.OrrConfig) + 7) & ~7
    buf = np.zeros(off + 8 * n, dtype=np.uint8)
    buf[:C.sizeof(_abi.OrrConfig)] = np.frombuffer(bytes(cfg), dtype=np.uint8)
    buf[off:] = totals.view(np.uint8)
    tin = torch.from_numpy(buf).to("cuda:0")
    tout = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    _launch(lib(build_name), "time_limit", tin, tout, n)
    return tout.cpu().numpy()
