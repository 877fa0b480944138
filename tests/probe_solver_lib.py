"""Builder + ctypes loader of the solver-stage probe (tests/device_probe/orr_probe_solver.hip) -- test infrastructure only.

A sibling of tests/probe_lib.py (one more ProbeBuilds: flags, hash file, file lock, atomic rename): delassus_columns<HAS_B> and
pgs_sweeps<HAS_B> of csrc/orr_physics.h behind four entry points.  Built three times next to its source: `one` and `w2` with the flags
of the two env units (the hand-scheduled sweeps), `generic` with the `one` flags plus -DORR_GENERIC_PGS (the readable C++ sweeps);
no part of libopenroborl_hip.so, of _lib.DEPS or of the source hash.
"""
import ctypes as C
import os

import numpy as np

from openroborl_amd import _lib
from tests import probe_lib

SRC = os.path.join(probe_lib.PROBE_DIR, "orr_probe_solver.hip")
BUILDS = {"one": ("liborr_probe_solver.so", list(_lib.HIPCC_FLAGS)),
          "w2": ("liborr_probe_solver_w2.so", list(_lib.HIPCC_FLAGS_W2)),
          "generic": ("liborr_probe_solver_generic.so", list(_lib.HIPCC_FLAGS) + ["-DORR_GENERIC_PGS"])}
ASM_BUILDS = ("one", "w2")

# entry point -> (words per input record, words per output record); the record layouts are listed in the source's header
PGS_IN, PGS_OUT, DEL_IN, DEL_OUT = 105, 28, 75, 115
SPECS = {"pgs_a": (PGS_IN, PGS_OUT), "pgs_ab": (PGS_IN, PGS_OUT), "delassus_pgs_a": (DEL_IN, DEL_OUT), "delassus_pgs_ab": (DEL_IN, DEL_OUT)}
MAX_ITERS = 32


_builds = probe_lib.ProbeBuilds(SRC, BUILDS)
lib_path, probe_hash, needs_build, compile_command = _builds.lib_path, _builds.probe_hash, _builds.needs_build, _builds.compile_command
build, build_all = _builds.build, _builds.build_all

_libs = {}


def lib(build_name):
    if build_name not in _libs:
        import torch  # noqa: F401  (first: see _lib.load)
        L = C.CDLL(build(build_name))
        for name in SPECS:
            fn = getattr(L, "orrp_" + name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.orrp_solver_record_words.restype = C.c_int
        L.orrp_solver_record_words.argtypes = [C.c_int]
        assert [L.orrp_solver_record_words(k) for k in range(4)] == [PGS_IN, PGS_OUT, DEL_IN, DEL_OUT]
        _libs[build_name] = L
    return _libs[build_name]


def run(build_name, name, x, iters):
    """entry point `name` on the float32 records x[n, NIN] with `iters` sweeps -> float32 [n, NOUT]"""
    import torch
    nin, nout = SPECS[name]
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = len(x)
    assert x.shape == (n, nin), (name, x.shape)
    assert n % 64 == 0 and n >= 128, "whole waves, at least two blocks"
    assert 0 <= iters <= MAX_ITERS
    tin = torch.from_numpy(x).to("cuda:0")
    tout = torch.full((n, nout), float("nan"), dtype=torch.float32, device="cuda:0")
    rc = getattr(lib(build_name), "orrp_" + name)(tin.data_ptr(), tout.data_ptr(), n, int(iters), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("orrp_%s(n=%d, iters=%d) failed: %d" % (name, n, iters, rc))
    return tout.cpu().numpy()
