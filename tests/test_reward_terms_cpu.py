"""No GPU: the host side of the per-term reward outputs (orr_bind_reward_terms) - the new translation unit compiles for gfx950 with
exactly its two step kernels, the loader's tables and exports, the entry point's host-side refusals, the env's kwarg, and what the
GPU test (tests/test_gpu_reward_terms.py) is bounded by: the fixtures' own identity reward == w . terms and the float32 parity oracle's
deviation from the reference's terms."""
import ctypes as C
import inspect
import os
import re
import sys
import tempfile

import numpy as np
import pytest

from openroborl_amd import _abi, _lib, env as envmod
from tests import reward_terms_lib as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_terms_unit_compiles_for_gfx950_with_its_two_kernels_no_fence_and_no_spill():
    """orr_kernels_terms.hip with the flags of its row: the env step and its parity replay with the terms on (MODE 4 and 6), CLIPS and
    NOISE true, nothing else; no cache write-back, no spilled vector register, no scratch access in the sub-step loop."""
    from tests import test_step_kernel_no_fence as nf
    (name, src, flags, hashed), = _lib.TERMS_UNITS
    assert name == "terms" and not hashed and flags is _lib.HIPCC_FLAGS and src in _lib.DEPS and src == _lib.SRC_TERMS
    with tempfile.TemporaryDirectory() as d:
        asm = nf.compile_unit(src, flags, d)
    bodies = nf.kernel_bodies(asm)
    assert sorted(re.match(r"(_Z15orr_step_kernelILi\dELi\dELb\dELb\dELb\dEE)", s).group(1) for s in bodies) == [
        "_Z15orr_step_kernelILi4ELi1ELb0ELb1ELb1EE", "_Z15orr_step_kernelILi6ELi1ELb0ELb1ELb1EE"], sorted(bodies)
    assert not re.search(r"^_Z16orr_reset_kernel\S*:", asm, re.M)            # the resets are the noise unit's
    nf.assert_no_cache_writeback(bodies)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats
    assert "noise" in isa_stats.STEP_KERNELS[-1][1] and "terms" not in isa_stats.STEP_KERNELS[-1][1]
    (sym, title), = isa_stats.TERMS_STEP_KERNELS
    assert "terms" in title and sym == "_Z15orr_step_kernelILi4ELi1ELb0ELb1ELb1E"
    for sym in (sym, sym.replace("Li4E", "Li6E")):
        res = isa_stats.resources(asm, sym)
        assert res is not None and int(res[5]) == 0, (sym, res)          # no spilled VGPR
        assert int(res[4]) <= 512, res                                   # one wave per SIMD
    insts, labels = isa_stats.parse_kernel(asm.split("\n"), isa_stats.TERMS_STEP_KERNELS[0][0])[:2]
    lo, hi = isa_stats.substep_loop(insts, labels)
    assert hi - lo > 2000 and isa_stats.scratch_accesses(insts[lo:hi + 1]) == 0
    side = isa_stats.loop_side_blocks(insts, labels, lo, hi)
    assert isa_stats.scratch_accesses([insts[i] for i in side]) == 0


@pytest.mark.parametrize("defs", [["-DORR_GENERIC_PGS"], ["-DORR_PHASE_TIMERS"], ["-DORR_COUNT_DUAL_CONTACT"], ["-DORR_WAVE_TIMELINE"], ["-DORR_WAVES_PER_EU=2"]])
def test_the_kernel_tuning_knobs_compile_in_the_terms_unit_too(defs):
    from tests import test_step_kernel_no_fence as nf
    r = nf.front_end_compiles(_lib.SRC_TERMS, defs)
    assert r.returncode == 0, "%s:\n%s" % (" ".join(defs), r.stderr[-1500:])


def test_unit_tables_and_exports():
    assert len(_lib.NOISE_UNITS) == 1 and _lib.ALL_UNITS == _lib.UNITS + _lib.NOISE_UNITS and _lib.ALL_ENV_UNITS == _lib.ENV_UNITS + _lib.NOISE_UNITS
    assert [u[0] for u in _lib.TERMS_UNITS] == ["terms"] and not [u for u in _lib.TERMS_UNITS if u in _lib.ALL_UNITS]
    src = inspect.getsource(_lib.build)
    assert "ALL_UNITS + TERMS_UNITS" in src and "ALL_ENV_UNITS + TERMS_UNITS" in src
    assert "orr_bind_reward_terms" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "openroborl_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(orr_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert "orr_bind_reward_terms" in declared and declared <= set(_lib.EXPORTS), declared - set(_lib.EXPORTS)
    assert re.search(r"#define ORR_ABI_VERSION 5\b", header) and _abi.ABI_VERSION == 5          # one added entry point, no struct change
    assert _abi.NUM_REWARD_TERMS == 5 and _abi.REWARD_TERM_NAMES == ("pose", "velocity", "end_effector", "root_pose", "root_velocity")
    assert envmod.VecQuadrupedEnv.TERM_NAMES == _abi.REWARD_TERM_NAMES
    L = _lib.load()
    for name in _lib.EXPORTS:
        assert hasattr(L, name), name
    assert L.orr_bind_reward_terms.argtypes == [C.c_void_p] * 4 and L.orr_bind_reward_terms.restype is C.c_int32


def test_a_null_handle_is_refused_by_name():
    L = _lib.load()
    buf = (C.c_float * 10)()
    assert L.orr_bind_reward_terms(None, None, None, None) == -1 and b"orr_bind_reward_terms" in L.orr_last_error()
    assert L.orr_bind_reward_terms(None, C.addressof(buf), C.addressof(buf), None) == -1 and b"orr_bind_reward_terms: null handle" in L.orr_last_error()


def test_kwarg_validation():
    sig = inspect.signature(envmod.VecQuadrupedEnv.__init__)
    assert sig.parameters["reward_terms"].default is False
    assert inspect.signature(envmod.VecQuadrupedEnv.episode_log).parameters["with_terms"].default is False
    assert "reward_terms" not in inspect.signature(envmod.LegacyListEnv.__init__).parameters
    import torch
    if not torch.cuda.is_available():          # with a GPU the constructor goes on; tests/test_gpu_reward_terms.py covers that side
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            envmod.VecQuadrupedEnv(num_robot=1, robot="laikago", motion_file="laikago_pace", reward_terms=True)
    # anything but a bool is refused ahead of everything that needs the device
    for bad in (1, 0, "yes", None, [True], 1.0):
        with pytest.raises(ValueError, match="reward_terms"):
            envmod.VecQuadrupedEnv(num_robot=1, robot="laikago", motion_file="laikago_pace", reward_terms=bad)


@pytest.mark.parametrize("name", rt.FIXTURES)
def test_fixture_reward_is_the_weighted_sum_of_its_terms(name):
    """reward == w . terms in the reference's own records, with the weights of orr_config (max deviation 0.0)."""
    g = rt.fixture(name)
    w = rt.weights(rt.fixture_config(g))
    assert abs(w.sum() - 1.0) < 1e-6
    dev = np.abs(g["step/terms"] @ rt.dec(w) - g["step/reward"]).max()
    print("REWARD_TERMS fixture %s: max |w . terms - reward| %.3e" % (name, dev))
    assert g["step/terms"].shape[-1] == 5 and (g["step/terms"] >= 0).all() and (g["step/terms"] <= 1).all()
    assert dev <= 1e-15


@pytest.mark.parametrize("name", rt.FIXTURES)
def test_float32_floor_of_the_terms(name):
    """The float32 parity oracle replays the fixture: its worst deviation from the reference's terms, per term, is what the device's
    terms are bounded by (2 x floor + 2^-22, tests/test_gpu_reward_terms.py).  Non-zero (float32 is not exact) and finite."""
    floor = rt.f32_floor(name)
    print("REWARD_TERMS float32 floor %s: %s" % (name, " ".join("%s %.3e" % (n, f) for n, f in zip(_abi.REWARD_TERM_NAMES, floor))))
    assert floor.shape == (5,) and np.isfinite(floor).all() and (floor > 0).all(), floor
    assert (floor < 1e-3).all(), floor                      # a replay that lost the fixture's states would be off by O(0.1)
    sums, length = rt.episode_sums(rt.fixture(name))
    assert length.max() >= 4 and (sums[length == 1] == rt.fixture(name)["step/terms"][length == 1]).all()
