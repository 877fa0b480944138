"""No GPU: the host side of the task noise (orr_set_task_noise; ImitationTask's perturb_init_state_prob / tar_obs_noise) - the new
translation unit and probe compile for gfx950, the struct layout, the float64 predictors of openroborl_amd/env.py against numpy and
against the fixture recorded from the reference's own Python (tests/golden/make_golden_init_noise.py), and the kwargs' validation."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from openroborl_amd import _abi, _lib, env as envmod
from tests import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ol.GOLDEN, "task_laikago_noise.npz")


def test_the_noise_unit_compiles_for_gfx950_with_its_three_kernels_and_no_fence():
    """orr_kernels_noise.hip with the flags of its row: the env step, its parity replay and the reset, NOISE = true behind CLIPS = true
    (the mangled names keep the prefixes the tools look kernels up by); like the other units' step kernels (tests/
    test_step_kernel_no_fence.py) without a cache write-back, and without a spilled vector register."""
    from tests import test_step_kernel_no_fence as nf
    (name, src, flags, hashed), = _lib.NOISE_UNITS
    assert name == "noise" and not hashed and flags is _lib.HIPCC_FLAGS and src in _lib.DEPS
    assert _lib.ALL_UNITS == _lib.UNITS + _lib.NOISE_UNITS and _lib.ALL_ENV_UNITS == _lib.ENV_UNITS + _lib.NOISE_UNITS
    with tempfile.TemporaryDirectory() as d:
        asm = nf.compile_unit(src, flags, d)
    bodies = nf.kernel_bodies(asm)
    assert sorted(bodies) == sorted(s for s in bodies if re.match(r"_Z15orr_step_kernelILi[02]ELi1ELb0ELb1ELb1EE", s)) and len(bodies) == 2, sorted(bodies)
    assert re.search(r"^_Z16orr_reset_kernelILb1ELb1EE\S*:", asm, re.M)
    nf.assert_no_cache_writeback(bodies)
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats
    sym, title = isa_stats.STEP_KERNELS[-1]
    assert "noise" in title and isa_stats.STEP_KERNELS[3][0] == "_Z15orr_step_kernelILi0ELi1ELb0ELb1ELb0E"
    res = isa_stats.resources(asm, sym)
    assert res is not None and int(res[5]) == 0, res          # no spilled VGPR
    insts, labels = isa_stats.parse_kernel(asm.split("\n"), sym)[:2]
    lo, hi = isa_stats.substep_loop(insts, labels)
    assert hi - lo > 2000 and isa_stats.scratch_accesses(insts[lo:hi + 1]) == 0


@pytest.mark.parametrize("defs", [["-DORR_GENERIC_PGS"], ["-DORR_PHASE_TIMERS"], ["-DORR_COUNT_DUAL_CONTACT"], ["-DORR_WAVE_TIMELINE"], ["-DORR_WAVES_PER_EU=2"]])
def test_the_kernel_tuning_knobs_compile_in_the_noise_unit_too(defs):
    """The development builds (tools/dev_build.py) pass their defines to every env unit, this one included: each of the knobs that
    tests/test_cpu_host.py keeps compiling in the four older units goes through the device compiler's front end here."""
    from tests import test_step_kernel_no_fence as nf
    r = nf.front_end_compiles(_lib.SRC_NOISE, defs)
    assert r.returncode == 0, "%s:\n%s" % (" ".join(defs), r.stderr[-1500:])


def test_the_noise_probe_compiles_for_gfx950():
    from tests import probe_noise_lib
    cmd = [c for c in probe_noise_lib.compile_command(os.devnull) if c not in ("-shared", "-fPIC")]
    r = subprocess.run(cmd + ["--cuda-device-only", "-fsyntax-only", "-Wno-unused-command-line-argument"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1500:]


def test_struct_layout_and_exports():
    L = _lib.load()
    assert L.orr_sizeof_task_noise() == C.sizeof(_abi.OrrTaskNoise) == 32
    assert [f[0] for f in _abi.OrrTaskNoise._fields_] == ["perturb_init_state_prob", "root_pos_std", "root_rot_std", "joint_pose_std", "root_vel_std",
                                                           "root_ang_vel_std", "joint_vel_std", "tar_heading_std"]
    assert {"orr_set_task_noise", "orr_sizeof_task_noise"} <= set(_lib.EXPORTS)
    # host-side argument checks need no device
    assert L.orr_set_task_noise(None, None) == -1 and b"orr_set_task_noise" in L.orr_last_error()


def test_normal_pair_is_box_muller():
    rng = np.random.RandomState(0)
    ua = rng.randint(0, 1 << 24, 100000) / float(1 << 24)
    ub = rng.randint(0, 1 << 24, 100000) / float(1 << 24)
    z0, z1 = envmod.normal_pair(ua, ub)
    r = np.sqrt(-2.0 * np.log(np.longdouble(1.0) - ua.astype(np.longdouble))).astype(np.float64)     # the definition, without log1p
    np.testing.assert_allclose(z0, r * np.cos(2 * np.pi * ub), atol=1e-13, rtol=0)
    np.testing.assert_allclose(z1, r * np.sin(2 * np.pi * ub), atol=1e-13, rtol=0)
    np.testing.assert_allclose(z0 * z0 + z1 * z1, -2.0 * np.log1p(-ua), atol=1e-12)
    assert abs(z0.mean()) < 0.02 and abs(z1.mean()) < 0.02 and abs(z0.std() - 1) < 0.02 and abs(z1.std() - 1) < 0.02
    # the ends of the radius' range: ua = 0 -> 0 exactly; ua = 1 - 2^-24 -> sqrt(48 ln 2) = 5.768
    for u in (0.0, 0.25, 0.5, 0.75):
        assert envmod.normal_pair(0.0, u) == (0.0, 0.0) or np.all(np.abs(envmod.normal_pair(0.0, u)) == 0.0)
    top = 1.0 - 2.0 ** -24
    z0, z1 = envmod.normal_pair(top, 0.0)
    assert abs(z0 - math.sqrt(48 * math.log(2))) < 1e-12 and z1 == 0.0
    z0, z1 = envmod.normal_pair(top, 0.25)
    assert abs(z0) < 1e-15 * 6 and abs(z1 - math.sqrt(48 * math.log(2))) < 1e-12
    assert np.isfinite(envmod.normal_pair(np.array([0.0, top]), np.array([0.5, 0.75]))).all()


def test_block_constants_and_indices():
    assert envmod.NOISE_RESET_BLOCK == 0x20000000 and envmod.NOISE_HEADING_BLOCK == 0x30000000
    d = envmod.init_perturb_draw_indices()
    assert d[0] == 4 * 0x20000000 and d[-1] == 4 * 0x20000008 + 3 and len(d) == 36 and d[-1] < 2 ** 32
    assert envmod.tar_noise_block() == 0x30000000 and envmod.tar_noise_block(0) == 0x30000001
    assert list(envmod.tar_noise_block(np.array([0, 5, 599]))) == [0x30000001, 0x30000006, 0x30000000 + 600]
    assert 4 * int(envmod.tar_noise_block(599)) + 1 < 2 ** 32                # orc_uniform's index is 32 bits wide
    # the reference's six (imitation_task.py:1201-1206)
    assert envmod.INIT_PERTURB_STD == {"root_pos_std": 0.025, "root_rot_std": 0.025 * np.pi, "joint_pose_std": 0.05 * np.pi, "root_vel_std": 0.1,
                                       "root_ang_vel_std": 0.05 * np.pi, "joint_vel_std": 0.05 * np.pi}


def test_the_zero_axis_is_no_rotation():
    U = np.full(36, 0.5)                    # a_i = -1 + 2 * 0.5 = 0
    d = envmod.init_perturb_draws(U, 1.0)
    assert d["perturbed"] and np.array_equal(d["rot"], [0.0, 0.0, 0.0, 1.0]) and not d["axis"].any() and np.isfinite(d["z"]).all()


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    L = ol.lib()
    seed, n = int(g["seed"]), int(g["num_robot"])
    u = lambda robot, ep, d: float(L.orc_uniform(seed, robot, ep, int(d)))
    return g, u, n


def qmul(a, b):      # Hamilton product, xyzw (transformations.quaternion_multiply)
    x1, y1, z1, w1 = a
    x0, y0, z0, w0 = b
    return np.array([x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0, -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0, x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0,
                     -x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0])


def test_fixture_perturbations_are_the_predictors(golden):
    """What the reference's _apply_state_perturb did with the device's draws = env.init_perturb_draws for the fixture's seed: the set of
    perturbed resets exactly, every offset to float64 rounding (the fixture's deviations are the reference's float64 ones, the
    predictor's the float32 ones the device holds: 6e-8 relative), the orientation as rot (x) reference rotation."""
    g, u, n = golden
    prob = float(g["noise"][0])
    pert = g["reset/perturbed"].astype(bool)
    assert pert.any() and not pert.all()
    for e in range(pert.shape[0]):
        for i in range(n):
            U = np.array([u(i, e + 1, d) for d in envmod.init_perturb_draw_indices()])
            p = envmod.init_perturb_draws(U, prob)
            assert bool(p["perturbed"]) == pert[e, i], (e, i)
            delta = g["reset/perturb_delta"][e, i]
            if not pert[e, i]:
                assert not delta.any()
                continue
            tol = dict(rtol=2e-7, atol=1e-15)
            np.testing.assert_allclose(delta[0:2], p["pos"], **tol)
            assert delta[2] == 0.0
            np.testing.assert_allclose(delta[7:9], p["vel"], **tol)
            assert delta[9] == 0.0
            np.testing.assert_allclose(delta[10:13], p["ang_vel"], **tol)
            np.testing.assert_allclose(delta[13:25], p["joints"], **tol)
            np.testing.assert_allclose(delta[25:37], p["joint_vel"], **tol)
            ref_rot = g["reset/ref_pose"][e, i, 3:7]
            np.testing.assert_allclose(g["reset/state37"][e, i, 3:7], qmul(p["rot"], ref_rot), atol=1e-8, rtol=0)


def test_fixture_heading_noises_are_the_predictors(golden):
    g, u, n = golden
    sigma = float(g["noise"][1])
    ep, s = 0, 0
    checked = 0
    for kind, idx in g["marks"]:
        idx = int(idx)
        if kind == 0.0:
            ep, s = ep + 1, 0
            blk, rec = int(envmod.tar_noise_block()), g["reset/heading_noise"][idx]
        else:
            blk, rec = int(envmod.tar_noise_block(s)), g["step/heading_noise"][idx]
            s += 1
        for i in range(n):
            z = float(envmod.normal_pair(u(i, ep, 4 * blk), u(i, ep, 4 * blk + 1))[0])
            assert abs(rec[i] - sigma * z) < 1e-15, (kind, idx, i)
            checked += 1
    assert checked == n * len(g["marks"]) and np.abs(g["step/heading_noise"]).max() > 0.1


def test_kwargs_validation():
    spec = envmod.task_noise_spec
    off = spec()
    assert off.perturb_init_state_prob == 0.0 and off.tar_heading_std == 0.0 and off.root_pos_std == np.float32(0.025)
    s = spec(0.5, [0.1, 7.0], {"root_vel_std": 0.2})                    # a list: the first entry, like the reference
    assert s.perturb_init_state_prob == 0.5 and s.tar_heading_std == np.float32(0.1) and s.root_vel_std == np.float32(0.2)
    assert s.joint_pose_std == np.float32(0.05 * np.pi) and spec(1.0, 0.3).tar_heading_std == np.float32(0.3)
    nan, inf = float("nan"), float("inf")
    for bad in (nan, -0.1, 1.5, inf, "0.5", True):
        with pytest.raises(ValueError, match="perturb_init_state_prob"):
            spec(bad)
    for bad in (nan, -0.1, inf, [nan], [-1.0], [], "x", [None]):
        with pytest.raises(ValueError, match="tar_obs_noise"):
            spec(0.0, bad)
    for k in envmod.INIT_PERTURB_STD:
        for bad in (nan, -1e-3, inf, "1"):
            with pytest.raises(ValueError, match=k):
                spec(0.5, None, {k: bad})
    with pytest.raises(ValueError, match="unknown"):
        spec(0.5, None, {"root_std": 0.1})
