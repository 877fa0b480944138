"""No GPU: the host side of the sensor noise (orr_set_sensor_noise; Minitaur._observation_noise_stdev) - the env's validation, the
arithmetic of the draw rule's Philox blocks, the fixture that the reference's own classes produced with the device's draws
(tests/golden/task_laikago_sensor_noise.npz: its recorded normals are the host predictor's, its call-site counts the asserted ones),
the new translation unit (compiles for gfx950 with its three kernels, without a spilled vector register) and the loader's tables."""
import ctypes as C
import math
import os
import re
import sys
import tempfile

import numpy as np
import pytest

from openroborl_amd import _abi, _lib, env as envmod
from tests import oracle_lib as ol
from tests import variant_probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ol.GOLDEN, "task_laikago_sensor_noise.npz")
ENV_STEP, REPLAY = "_Z15orr_step_kernelILi60ELi1ELb0ELb1ELb1EE", "_Z15orr_step_kernelILi54ELi1ELb0ELb1ELb1EE"
RESET = "_Z23orr_sensor_reset_kernelILb1EE"


# ---- 1. validation ---------------------------------------------------------------------------------------------------------------------
def test_sensor_noise_spec_accepts_and_refuses():
    s = envmod.sensor_noise_spec(None)
    assert [getattr(s, f) for f in _abi.SENSOR_NOISE_FIELDS] == [0.0] * 5 and not envmod.sensor_noise_on(s)
    s = envmod.sensor_noise_spec((0.02, 0.5, 0.25, 0.03, 0.1))
    assert [getattr(s, f) for f in _abi.SENSOR_NOISE_FIELDS] == [float(np.float32(v)) for v in (0.02, 0.5, 0.25, 0.03, 0.1)]
    assert envmod.sensor_noise_on(s)
    assert envmod.sensor_noise_on(envmod.sensor_noise_spec(np.array([0, 0, 0, 0, 1e-3])))
    assert envmod.sensor_noise_on(envmod.sensor_noise_spec([0, 0, 0, 1e-3, 0]))
    # velocity and torque alone select nothing: they have no consumer
    assert not envmod.sensor_noise_on(envmod.sensor_noise_spec([0.0, 0.5, 0.5, 0.0, 0.0]))
    assert C.sizeof(_abi.OrrSensorNoise) == 20
    for k, name in enumerate(_abi.SENSOR_NOISE_FIELDS):
        for bad in (float("nan"), -1e-3, math.inf):
            v = [0.01] * 5
            v[k] = bad
            with pytest.raises(ValueError, match=name):
                envmod.sensor_noise_spec(v)
        v = [0.01] * 5
        v[k] = "x"
        with pytest.raises(ValueError, match=name):
            envmod.sensor_noise_spec(v)
    for bad in ([0.1] * 4, [0.1] * 6, 0.1, "0.1,0,0,0,0", {"motor_angle_std": 0.1}, [[0.1] * 5], True):
        with pytest.raises(ValueError, match="observation_noise_stdev"):
            envmod.sensor_noise_spec(bad)


def test_the_keyword_reaches_every_constructor():
    import inspect
    assert "observation_noise_stdev" in inspect.signature(envmod.VecQuadrupedEnv.__init__).parameters
    assert "observation_noise_stdev" in inspect.signature(envmod.LegacyListEnv.__init__).parameters
    assert inspect.signature(envmod.build_env).parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD       # passed through to the env
    assert callable(envmod.VecQuadrupedEnv.set_sensor_noise)
    sys.path.insert(0, ROOT)
    import train
    assert train.sensor_noise_arg("0.01,0,0,0.02,0.1") == [0.01, 0.0, 0.0, 0.02, 0.1]
    import argparse
    for bad in ("0.01,0,0,0.02", "a,b,c,d,e"):
        with pytest.raises(argparse.ArgumentTypeError):
            train.sensor_noise_arg(bad)


# ---- 2. the blocks ---------------------------------------------------------------------------------------------------------------------
def test_sensor_noise_block_arithmetic():
    assert int(envmod.sensor_noise_block(0, 0, 0)) == 0x10000000
    assert int(envmod.sensor_noise_block(3, 17, 5)) == 0x10000000 + (3 << 9) + (17 << 4) + 5
    assert int(envmod.sensor_noise_block((1 << 19) - 1, 31, 15)) == 0x1FFFFFFF < 0x20000000
    for bad in ((-1, 0, 0), (1 << 19, 0, 0), (0, 32, 0), (0, 0, 16), (0, -1, 0)):
        with pytest.raises(ValueError):
            envmod.sensor_noise_block(*bad)
    # no collision between steps, slots or lanes: the whole grid of a few i, every slot in use, every lane
    i = np.concatenate([np.arange(0, 40), [1000, (1 << 19) - 2, (1 << 19) - 1]])
    I, S, Ln = np.meshgrid(i, np.arange(0, 20), np.arange(0, 16), indexing="ij")
    blocks = envmod.sensor_noise_block(I, S, Ln).ravel()
    assert len(np.unique(blocks)) == blocks.size
    assert blocks.min() >= 0x10000000 and blocks.max() < 0x20000000
    # none with the episode's other blocks: 0..7 (the reset's draws), 8 + s (clip switching), the task noise's
    others = np.concatenate([np.arange(0, 8), 8 + np.arange(0, 1 << 20, 997), [8 + (1 << 24)], envmod.NOISE_RESET_BLOCK + np.arange(0, 9),
                             np.asarray(envmod.tar_noise_block(np.arange(0, 1 << 20, 997))), [int(envmod.tar_noise_block())]])
    assert not np.intersect1d(blocks, others).size
    assert (others[others >= 0x10000000] >= 0x20000000).all()
    assert 4 * 0x1FFFFFFF + 3 < 1 << 32          # a draw index is 4 * block + word, 32 bits


def test_sensor_noise_normals_are_normal_pairs():
    u = np.array([[0.1, 0.2, 0.3, 0.4], [0.0, 0.0, 0.999, 0.75]])
    z = envmod.sensor_noise_normals(u)
    a0, a1 = envmod.normal_pair(u[:, 0], u[:, 1])
    b0, b1 = envmod.normal_pair(u[:, 2], u[:, 3])
    np.testing.assert_array_equal(z, np.stack([a0, a1, b0, b1], axis=-1))
    assert z[1, 0] == 0.0 and z[1, 1] == 0.0


# ---- 3. the fixture --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def normals(L, seed, robot, ep, i, slot, lane):
    blk = int(envmod.sensor_noise_block(i, slot, lane))
    return envmod.sensor_noise_normals([L.orc_uniform(seed, robot, ep, 4 * blk + w) for w in range(4)])


def test_the_fixtures_normals_are_the_host_predictors(golden):
    """Every recorded normal, site by site, equals sensor_noise_normals of orc_uniform at sensor_noise_block's block, bit for bit."""
    g, L = golden, ol.lib()
    seed, n = int(g["seed"]), int(g["num_robot"])
    ep = 0
    for kind, idx in g["marks"]:
        idx = int(idx)
        if kind == 0.0:
            ep += 1
            for r in range(n):
                hist = np.stack([normals(L, seed, r, ep, 0, envmod.SENSOR_SLOT_HIST, c) for c in range(16)])     # [16, 4]
                np.testing.assert_array_equal(g["reset/z_hist"][idx, r], hist[:, [0, 1, 2]].T)
                np.testing.assert_array_equal(g["reset/z_target"][idx, r], normals(L, seed, r, ep, 0, envmod.SENSOR_SLOT_TARGET, 0)[0:3])
        else:
            for r in range(n):
                i = int(g["step/noise_i"][idx, r])
                assert i == int(g["step/env_step_counter"][idx, r])       # 1 + the counter before the step = the counter after it
                sub = np.stack([[normals(L, seed, r, ep, i, s, m) for m in range(12)] for s in range(17)])        # [17, 12, 4]
                z0 = np.stack([sub[k >> 1, :, 2 * (k & 1)] for k in range(33)])
                z1 = np.stack([sub[k >> 1, :, 2 * (k & 1) + 1] for k in range(33)])
                np.testing.assert_array_equal(g["step/z_clip"][idx, r], z0)
                first = bool(g["step/first"][idx, r])
                np.testing.assert_array_equal(g["step/z_lerp"][idx, r], z1 if first else np.zeros((33, 12)))
                filt = np.array([normals(L, seed, r, ep, i, envmod.SENSOR_SLOT_FILTER, m)[0] for m in range(12)])
                np.testing.assert_array_equal(g["step/z_filter"][idx, r], filt if first else np.zeros(12))
                hist = np.array([normals(L, seed, r, ep, i, envmod.SENSOR_SLOT_HIST, c)[0] for c in range(16)])
                np.testing.assert_array_equal(g["step/z_hist"][idx, r], hist)
                np.testing.assert_array_equal(g["step/z_target"][idx, r], normals(L, seed, r, ep, i, envmod.SENSOR_SLOT_TARGET, 0)[0:3])
    assert ep == g["reset/z_hist"].shape[0] >= 2


def test_the_fixtures_content(golden):
    g = golden
    a, v, t, r, d = (float(x) for x in g["sensor_noise"])
    assert (a, r, d) == (0.02, 0.03, 0.1) and v == 0.5 and t == 0.5       # the inert deviations are present, and large
    assert not bool(g["randomizer"]) and int(g["num_robot"]) == 4
    # the call-site counts: a reset 3 readings x 3 getters + the target observation's rpy; a step 33 clip readings + 3 sensor readings + 1
    # target rpy, and in an episode's first step 33 interpolation starts + 1 filter initialisation more
    assert (g["reset/calls"] == 10).all()
    first = g["step/first"].astype(bool)
    assert (g["step/calls"][first] == 71).all() and (g["step/calls"][~first] == 37).all()
    assert first.any() and (~first).any()
    assert (first == (g["step/noise_i"] == 1)).all()
    assert (g["step/z_lerp"][~first] == 0).all() and (g["step/z_filter"][~first] == 0).all()
    assert (g["step/z_lerp"][first] != 0).all() and (g["step/z_clip"] != 0).all()
    # an active clip whose result the noise decides, and a first-step interpolation start that passes the clip (its draw moves a torque)
    active, noisy = g["step/clip_active"].astype(bool), g["step/clip_noisy"].astype(bool)
    assert (active & noisy).any()
    assert (~active[first]).any()
    # the three readings of a reset are three draws
    zh = g["reset/z_hist"]
    assert (zh[:, :, 0] != zh[:, :, 1]).all() and (zh[:, :, 1] != zh[:, :, 2]).all() and (zh[:, :, 0] != zh[:, :, 2]).all()
    # the noise is in the recorded observation: the newest motor-angle words of a step differ from the control observation's by sigma z
    obs = g["step/obs"].astype(np.float64)
    co = g["step/ctrl_obs"][:, :, 0:12]
    wrapped = (co + np.pi) % (2 * np.pi) - np.pi
    np.testing.assert_allclose(obs[:, :, 48:84].reshape(obs.shape[0], -1, 3, 12)[:, :, 0], wrapped + a * g["step/z_hist"][:, :, 0:12], atol=1e-6)
    assert os.path.getsize(GOLDEN) < 1 << 20


# ---- 4. the unit and the tables --------------------------------------------------------------------------------------------------------
def test_the_sensor_unit_compiles_for_gfx950_with_its_three_kernels_and_no_spill():
    """orr_kernels_sensor.hip with the flags of its row: the env step on top of everything (MODE 32 | 16 | 8 | 4 | 0 = 60), the parity
    replay (MODE 32 | 16 | 4 | 2 = 54) and the reset orr_sensor_reset_kernel<true>, nothing else; no spilled vector register, no scratch access in
    the sub-step loop."""
    from tests import test_step_kernel_no_fence as nf
    (name, src, flags, hashed), = _lib.SENSOR_UNITS
    assert name == "sensor" and not hashed and flags is _lib.HIPCC_FLAGS and src in _lib.DEPS and src == _lib.SRC_SENSOR
    with tempfile.TemporaryDirectory() as d:
        asm = nf.compile_unit(src, flags, d)
    bodies = nf.kernel_bodies(asm)
    assert sorted(re.match(r"(_Z15orr_step_kernelILi\d+ELi\dELb\dELb\dELb\dEE)", s).group(1) for s in bodies) == sorted([ENV_STEP, REPLAY]), sorted(bodies)
    assert set(re.findall(r"^(_Z\d+orr_\w*reset_kernelI\w+?EE)v\S*:", asm, re.M)) == {RESET}       # its own reset kernel, none of orr_reset_kernel's
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats
    assert [s + "E" for s, _ in isa_stats.SENSOR_STEP_KERNELS] == [ENV_STEP] and len(isa_stats.ACTUATOR_STEP_KERNELS) == 1
    for sym in (ENV_STEP, REPLAY, RESET):
        res = isa_stats.resources(asm, sym)
        assert res is not None and int(res[5]) == 0, (sym, res)          # no spilled VGPR
        assert int(res[4]) <= 512, res                                   # one wave per SIMD
    insts, labels = isa_stats.parse_kernel(asm.split("\n"), ENV_STEP[:-1])[:2]
    lo, hi = isa_stats.substep_loop(insts, labels)
    assert hi - lo > 2000 and isa_stats.scratch_accesses(insts[lo:hi + 1]) == 0
    side = isa_stats.loop_side_blocks(insts, labels, lo, hi)
    assert isa_stats.scratch_accesses([insts[i] for i in side]) == 0


def test_unit_tables_exports_and_sizes(tmp_path_factory):
    assert [u[0] for u in _lib.SENSOR_UNITS] == ["sensor"]
    older = _lib.ALL_UNITS + _lib.TERMS_UNITS + _lib.CONTACT_UNITS + _lib.ACTUATOR_UNITS
    assert not [u for u in _lib.SENSOR_UNITS if u in older] and len(older) == 10
    assert len(_lib.ACTUATOR_UNITS) == 1 and _lib.ALL_UNITS == _lib.UNITS + _lib.NOISE_UNITS           # the older tables stay
    assert "orr_set_sensor_noise" in _lib.EXPORTS and "orr_sizeof_sensor_noise" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "openroborl_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define ORR_ABI_VERSION 5\b", header) and _abi.ABI_VERSION == 5                    # additive
    assert re.search(r"int32_t orr_set_sensor_noise\(orr_handle\* h, const orr_sensor_noise\* noise_host\);", header)
    assert "float motor_angle_std, motor_velocity_std, motor_torque_std, base_rpy_std, base_rpy_rate_std;" in header
    assert "NO consumer" in header and "0x10000000 + (i << 9) + (slot << 4) + lane" in header
    with open(os.path.join(_lib.CSRC, "orr_device.h")) as f:
        assert "constexpr int kModeSensor = 32;" in f.read()
    with open(_lib.SRC) as f:
        main = f.read()
    # the same refusal texts as ever, as the main unit now puts them together: the setters' shared helpers (check_stds, anchor_conflict)
    # with the entry's name and their one format string each.  What the calls return on a device: tests/test_gpu_setters_refused.py
    for text in ("orr_set_sensor_noise: null handle", 'check_stds("orr_set_sensor_noise", stds)', '"%s: %s must be a finite standard deviation >= 0"',
                 'anchor_conflict(h, "orr_set_sensor_noise", "sensor noise")',
                 '"%s: friction anchors (orr_model::friction_anchor) and %s cannot be combined"'):
        assert text in main, text
    probe = variant_probe.lib(tmp_path_factory)
    for entry in ("orr_step", "orr_reset", "orr_debug_replay_step", "orr_debug_replay_reset"):
        assert probe.choose({"sensor", "actuator"}, entry) == ("kSensor", None)                       # sensor noise first
        assert probe.choose({"sensor", "actuator", "anchors"}, entry) == (
            "kRefused", entry + ": friction anchors (orr_model::friction_anchor) and sensor noise (orr_set_sensor_noise) cannot be combined")
    L = _lib.load()
    for name in _lib.EXPORTS:
        assert hasattr(L, name), name
    assert L.orr_sizeof_sensor_noise() == C.sizeof(_abi.OrrSensorNoise) == 20
    assert L.orr_set_sensor_noise(None, None) == -1 and b"orr_set_sensor_noise: null handle" in L.orr_last_error()
