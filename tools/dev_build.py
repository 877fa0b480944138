"""What the tools that run a development build of the env kernels share (phase_cycles, wave_timeline, wave_phases, wave_pairing,
wave_times, diag/wave_spread, dual_contact): build + load of the library, the names of the phase timers' slots, the per-wave
timeline and the decoding of its hardware-slot word.  Only what at least two of them call; everything else stays in the tool."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openroborl_amd import _lib  # noqa: E402  (importing it loads nothing)

# the PT(k) slots 0..15 of orr_step_kernel (-DORR_PHASE_TIMERS; 3..9 are marks inside physics_substep)
PHASE_NAMES = ["load+leg consts", "set_act/filter", "substep control", "leg dynamics", "fall proxies", "row setup", "row response",
               "Delassus columns", "PGS sweeps", "du+integrate", "receive_obs (ring)", "ctrl_obs+sensors", "reward+ref update",
               "termination+obs", "episode end/reset", "store"]
DEBUG_ARGTYPES = {"orr_debug_phase_cycles": [C.POINTER(C.c_longlong), C.c_int], "orr_debug_wave_phases": [C.POINTER(C.c_longlong), C.c_int],
                  "orr_debug_wave_times": [C.POINTER(C.c_longlong), C.c_int], "orr_debug_dual_contact": [C.POINTER(C.c_ulonglong), C.c_int],
                  "orr_debug_stage_words": [], "orr_debug_stage_dump": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]}
PHASE_TIMERS = ("phase_timers", ["-DORR_PHASE_TIMERS"])      # load(*PHASE_TIMERS): the build that four of the tools and tests/test_gpu_tools.py share
STAGE_DUMP = ("stage_dump", ["-DORR_STAGE_DUMP"])            # the build with orr_debug_stage_dump (tests/test_gpu_substep_stages.py)


def build(name, flags):
    """openroborl_amd/libopenroborl_<name>.so = the library with `flags` added to the env kernels' units; compiled unless the file
    already is that build of the sources on disk"""
    lib = os.path.join(_lib.PKG_DIR, "libopenroborl_%s.so" % name)
    if _lib.library_hash(lib) != _lib.source_hash(flags):
        _lib.build(out_path=lib, extra_flags=flags)
    return lib


def load(name, flags, step_waves_per_eu=None):
    """build(), then make that library the one of this process (ORR_LIB_PATH, and ORR_STEP_WAVES_PER_EU if given: call this before
    anything creates an env), load it and declare the orr_debug_* entries it exports."""
    os.environ["ORR_LIB_PATH"] = build(name, flags)
    if step_waves_per_eu is not None:
        os.environ["ORR_STEP_WAVES_PER_EU"] = str(step_waves_per_eu)
    L = _lib.load()
    for entry, argtypes in DEBUG_ARGTYPES.items():
        if hasattr(L, entry):
            getattr(L, entry).argtypes = argtypes
    return L


def laikago_env(robots):
    """The workload of the phase timers' tools: `robots` Laikago robots, reset, and one fixed batch of small random actions."""
    import torch
    from openroborl_amd.env import VecQuadrupedEnv
    env = VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=robots, seed=0)
    env.reset()
    act = (torch.randn(robots, 12, generator=torch.Generator().manual_seed(0)) * 0.1).to(env.device)
    return env, act


def wave_rows(L, waves):
    """The per-wave timeline of the last step launch (-DORR_WAVE_TIMELINE / -DORR_PHASE_TIMERS builds), int64 [waves, 4]: realtime start,
    realtime end (100 MHz ticks), shader cycles, slot word (decode_slot).  The first call allocates the device buffer, and only the
    launches after it are recorded: call it once before the launches to be read."""
    buf = (C.c_longlong * (4 * waves))()
    _lib.check(L.orr_debug_wave_times(None, waves) or L.orr_debug_wave_times(buf, waves), L)    # (no room for `waves` yet: allocates)
    return np.frombuffer(buf, dtype=np.int64).reshape(waves, 4)


def decode_slot(rows):
    """Word 3 of the timeline's rows -> (mask of the wave's robots that finished an episode, XCC, SE, SH, CU, SIMD)"""
    w = rows[:, 3]
    hw = (w >> 8) & 0xFFFFFFFF            # HW_REG_HW_ID: wave 3:0, simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13 (gfx9 layout)
    return w & 0xFF, (w >> 40) & 0xF, (hw >> 13) & 7, (hw >> 12) & 1, (hw >> 8) & 0xF, (hw >> 4) & 3
