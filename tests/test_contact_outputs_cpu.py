"""No GPU: the host side of the foot contact outputs (orr_bind_contact_outputs) - the new translation unit compiles for gfx950 with
exactly its three step kernels, the loader's tables and exports, the entry point's host-side refusals, the env's kwarg, the reduction of
the oracle's sub-step trace that the GPU test (tests/test_gpu_contact_outputs.py) compares with, and that test's floor rule run with
the oracle alone: float64 against the float32 parity build in the device's place."""
import ctypes as C
import inspect
import os
import re
import sys
import tempfile

import numpy as np
import pytest

from openroborl_amd import _abi, _lib, env as envmod
from tests import contact_lib as cl
from tests import variant_probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_STEP, ENV_STEP_TERMS, DEBUG = ("_Z15orr_step_kernelILi8ELi1ELb0ELb1ELb1EE", "_Z15orr_step_kernelILi12ELi1ELb0ELb1ELb1EE",
                                   "_Z15orr_step_kernelILi9ELi1ELb0ELb0ELb0EE")


# ---- 1. ABI mirror, refusal texts, unit table ----------------------------------------------------------------------------------------
def test_the_contacts_unit_compiles_for_gfx950_with_its_three_kernels_no_fence_and_no_spill():
    """orr_kernels_contacts.hip with the flags of its row: the env step with the contact sums (MODE 8), the same with the reward terms
    (MODE 12), both with CLIPS and NOISE, and the debug physics (MODE 9), nothing else; no cache write-back, no spilled vector register,
    no scratch access in the sub-step loop."""
    from tests import test_step_kernel_no_fence as nf
    (name, src, flags, hashed), = _lib.CONTACT_UNITS
    assert name == "contacts" and not hashed and flags is _lib.HIPCC_FLAGS and src in _lib.DEPS and src == _lib.SRC_CONTACTS
    with tempfile.TemporaryDirectory() as d:
        asm = nf.compile_unit(src, flags, d)
    bodies = nf.kernel_bodies(asm)
    assert sorted(re.match(r"(_Z15orr_step_kernelILi\d+ELi\dELb\dELb\dELb\dEE)", s).group(1) for s in bodies) == sorted([ENV_STEP, ENV_STEP_TERMS, DEBUG]), sorted(bodies)
    assert not re.search(r"^_Z16orr_reset_kernel\S*:", asm, re.M)            # the resets are the noise unit's
    nf.assert_no_cache_writeback(bodies)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats
    assert "noise" in isa_stats.STEP_KERNELS[-1][1] and len(isa_stats.TERMS_STEP_KERNELS) == 1        # the older tables stay
    assert [s + "E" for s, _ in isa_stats.CONTACT_STEP_KERNELS] == [ENV_STEP, ENV_STEP_TERMS] and all("contact" in t for _, t in isa_stats.CONTACT_STEP_KERNELS)
    for sym in (ENV_STEP, ENV_STEP_TERMS, DEBUG):
        res = isa_stats.resources(asm, sym)
        assert res is not None and int(res[5]) == 0, (sym, res)          # no spilled VGPR
        assert int(res[4]) <= 512, res                                   # one wave per SIMD
    for sym, _ in isa_stats.CONTACT_STEP_KERNELS:
        insts, labels = isa_stats.parse_kernel(asm.split("\n"), sym)[:2]
        lo, hi = isa_stats.substep_loop(insts, labels)
        assert hi - lo > 2000 and isa_stats.scratch_accesses(insts[lo:hi + 1]) == 0
        side = isa_stats.loop_side_blocks(insts, labels, lo, hi)
        assert isa_stats.scratch_accesses([insts[i] for i in side]) == 0


@pytest.mark.parametrize("defs", [["-DORR_GENERIC_PGS"], ["-DORR_PHASE_TIMERS"], ["-DORR_COUNT_DUAL_CONTACT"], ["-DORR_WAVE_TIMELINE"], ["-DORR_WAVES_PER_EU=2"]])
def test_the_kernel_tuning_knobs_compile_in_the_contacts_unit_too(defs):
    from tests import test_step_kernel_no_fence as nf
    r = nf.front_end_compiles(_lib.SRC_CONTACTS, defs)
    assert r.returncode == 0, "%s:\n%s" % (" ".join(defs), r.stderr[-1500:])


def test_unit_tables_exports_and_refusal_texts(tmp_path_factory):
    assert [u[0] for u in _lib.CONTACT_UNITS] == ["contacts"]
    assert not [u for u in _lib.CONTACT_UNITS if u in _lib.ALL_UNITS + _lib.TERMS_UNITS + _lib.ALL_ENV_UNITS]
    assert len(_lib.NOISE_UNITS) == 1 and len(_lib.TERMS_UNITS) == 1 and _lib.ALL_UNITS == _lib.UNITS + _lib.NOISE_UNITS
    src = inspect.getsource(_lib.build)
    assert "ALL_UNITS + TERMS_UNITS" in src and "ALL_ENV_UNITS + TERMS_UNITS" in src                  # what existing tests look for
    assert "ALL_UNITS + TERMS_UNITS + CONTACT_UNITS" in src and "ALL_ENV_UNITS + TERMS_UNITS + CONTACT_UNITS" in src
    assert "orr_bind_contact_outputs" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "openroborl_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(orr_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert "orr_bind_contact_outputs" in declared and declared <= set(_lib.EXPORTS), declared - set(_lib.EXPORTS)
    assert re.search(r"#define ORR_ABI_VERSION 5\b", header) and _abi.ABI_VERSION == 5          # one added entry point, no struct change
    assert re.search(r"int32_t orr_bind_contact_outputs\(orr_handle\* h, float\* contact_dev, float\* contact_ep_dev, float\* contact_log_dev\);", header)
    assert (_abi.CONTACT_OUT_DIM, _abi.CONTACT_EP_DIM) == (16, 8) and _abi.CONTACT_COLUMNS == ("normal", "friction_x", "friction_y", "normal_max")
    with open(os.path.join(_lib.CSRC, "orr_device.h")) as f:
        device_h = f.read()
    assert re.search(r"constexpr int kModeTerms = 4;", device_h) and re.search(r"constexpr int kModeContacts = 8;", device_h)
    with open(_lib.SRC) as f:
        main = f.read()
    # the same refusal texts as ever, as the main unit now puts them together: bind_three with the entry's name and texts, and the
    # shared format strings.  What the calls return on a device: tests/test_gpu_setters_refused.py
    for text in ('bind_three(h, "orr_bind_contact_outputs", &DevTables::contact_out, &orr_handle::contacts_on, contact_dev, contact_ep_dev, contact_log_dev,',
                 '"%s: null handle"', '"contact_dev needs contact_ep_dev (the totals of the current episode)"',
                 '"the contact buffers must be 16-byte aligned (rows of 16 and 8 floats)", "contact outputs");',
                 '"%s: friction anchors (orr_model::friction_anchor) and %s cannot be combined"'):
        assert text in main, text
    probe = variant_probe.lib(tmp_path_factory)
    for entry in ("orr_reset", "orr_step", "orr_debug_physics"):
        assert probe.choose({"contacts", "anchors"}, entry) == (
            "kRefused", entry + ": friction anchors (orr_model::friction_anchor) and contact outputs (orr_bind_contact_outputs) cannot be combined")
    for entry in ("orr_debug_replay_step", "orr_debug_replay_reset"):        # no contact variant, so no refusal either
        assert probe.choose({"contacts", "anchors"}, entry) == ("kAnchor", None)
    # the main unit calls the contact variants and cannot compile them
    with open(os.path.join(_lib.CSRC, "orr_env_kernels.h")) as f:
        kernels_h = f.read()
    for inst in ("launch_step<kModeContacts | 0, 1, false, true, true>", "launch_step<kModeContacts | kModeTerms | 0, 1, false, true, true>",
                 "launch_step<kModeContacts | 1, 1, false, false>"):
        assert "extern template StepLaunch " + inst + ";" in kernels_h, inst
    L = _lib.load()
    for name in _lib.EXPORTS:
        assert hasattr(L, name), name
    assert L.orr_bind_contact_outputs.argtypes == [C.c_void_p] * 4 and L.orr_bind_contact_outputs.restype is C.c_int32


def test_a_null_handle_is_refused_by_name():
    L = _lib.load()
    buf = (C.c_float * 16)()
    assert L.orr_bind_contact_outputs(None, None, None, None) == -1 and b"orr_bind_contact_outputs" in L.orr_last_error()
    assert L.orr_bind_contact_outputs(None, C.addressof(buf), C.addressof(buf), None) == -1 and b"orr_bind_contact_outputs: null handle" in L.orr_last_error()


def test_kwarg_validation():
    sig = inspect.signature(envmod.VecQuadrupedEnv.__init__)
    assert sig.parameters["contact_outputs"].default is False
    assert inspect.signature(envmod.VecQuadrupedEnv.episode_log).parameters["with_contacts"].default is False
    assert "contact_outputs" not in inspect.signature(envmod.LegacyListEnv.__init__).parameters
    for name in ("bind_contact_outputs", "foot_contact", "foot_forces", "foot_peak_force", "episode_gait"):
        assert callable(getattr(envmod.VecQuadrupedEnv, name)), name
    import torch
    if not torch.cuda.is_available():          # with a GPU the constructor goes on; tests/test_gpu_contact_outputs.py covers that side
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            envmod.VecQuadrupedEnv(num_robot=1, robot="laikago", motion_file="laikago_pace", contact_outputs=True)
    # anything but a bool is refused ahead of everything that needs the device
    for bad in (1, 0, "yes", None, [True], 1.0):
        with pytest.raises(ValueError, match="contact_outputs"):
            envmod.VecQuadrupedEnv(num_robot=1, robot="laikago", motion_file="laikago_pace", contact_outputs=bad)


# ---- 2. the trace reduction -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reduce_trace_against_a_per_substep_loop(dtype):
    rng = np.random.RandomState(0)
    n, rep = 5, 33
    trace = rng.normal(0.0, 0.3, (n, rep, 48)).astype(dtype)
    trace[:, :, 0:12:3] = np.abs(trace[:, :, 0:12:3]) * (rng.rand(n, rep, 4) < 0.6)        # normal impulses: >= 0, open contacts 0
    trace[1, :, 0:3] = 0.0                                                                  # a leg in the air for the whole step
    got = cl.reduce_trace(trace)
    assert got.shape == (n, 4, 4) and got.dtype == dtype
    for i in range(n):
        for leg in range(4):
            acc, top = [dtype(0), dtype(0), dtype(0)], dtype(0)
            for s in range(rep):
                for d in range(3):
                    acc[d] = dtype(acc[d] + trace[i, s, 3 * leg + d])
                top = max(top, trace[i, s, 3 * leg])
            assert [x.tobytes() for x in got[i, leg]] == [x.tobytes() for x in acc + [top]], (i, leg)
    assert not got[1, 0].any() and (got[:, :, 3] <= got[:, :, 0]).all() and (got[:, :, 3] >= 0).all()


# ---- 3. the floor rule with the oracle alone ------------------------------------------------------------------------------------------
def test_floor_rule_with_the_float32_oracle_in_the_devices_place():
    """The inputs of the GPU test's product-path comparison (N = 37 mixed, train mode, randomiser on, no auto-reset, seed 3, 40 steps,
    each robot's shipped policy on the float64 oracle's observation + N(0, 0.05) from RandomState(11)).  Every step starts from the
    float64 run's record; the float32 parity build stands where the device stands on the GPU: q = the 99th percentile of |f32 - f64|
    over the live cells, cell bound 4 q + 2^-22 max(1, |ref|), at most 0.5 % of the live leg-steps with a cell over it (the device's
    cap of 2 % holds with it), dead leg-steps exactly zero unless within that share, at least 1000 live leg-steps.
    Measured: q99 2.9e-5 .. 3.5e-5 N s over four seeds."""
    cfg, models, clips, robot_type, clip_id = cl.mixed_setup()
    o64 = cl.TracedOracle(cfg, models, clips, cl.N, robot_type, clip_id)
    o32 = cl.TracedOracle(cfg, models, clips, cl.N, robot_type, clip_id, f32=True)
    rng = np.random.RandomState(cl.ACTION_SEED)
    obs = o64.orc.reset()
    ref, f32 = [], []
    for k in range(cl.STEPS):
        act = cl.policy_actions(obs, robot_type, rng)
        state, counters = o64.orc.state.copy(), o64.orc.counters.copy()
        f32.append(o32.step_from(state, counters, act))
        ref.append(o64.step_from(state, counters, act))
        obs = o64.orc.obs.copy()
    o64.close(); o32.close()
    r = cl.floor_rule(np.stack(ref), np.stack(f32), dev=np.stack(f32))
    print("CONTACT_OUTPUTS floor rule, oracle alone (%d robots x %d steps): %s" % (cl.N, cl.STEPS, cl.describe(r)))
    assert r["live"] >= cl.MIN_LIVE
    assert 0 < r["q"] < 1e-3                                 # float32 is not exact; a run that lost the state would be off by O(0.1)
    assert r["f32_share"] <= cl.F32_SHARE
    assert r["dev_share"] <= cl.DEVICE_SHARE                 # the float32 build in the device's place, dead leg-steps included
    sums = np.stack(ref)
    assert sums[..., 0].max() > 0.5 and (sums[..., 3] <= sums[..., 0] + 1e-15).all()       # sums of order 1 N s
