"""External pushes (orr_set_push, orr_bind_push_outputs) without a GPU: every refusal of push_spec, the block arithmetic, the float64
predictor on the oracle's Philox stream, the ABI against the header's text, and the soundness of the inputs of the GPU physics comparison
(tests/test_gpu_push.py): the float32 parity oracle alone stays under the project's cap."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from openroborl_amd import _abi, _lib, env as envmod
from tests import actuator_lib as al
from tests import oracle_lib as ol
from tests import push_lib as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = dict(prob=0.25, lin_vel=(0.2, 0.6), lin_vel_z=0.2, ang_vel=0.5, grace_steps=2)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad, needle", [
    (dict(GOOD, prob=math.nan), "prob"), (dict(GOOD, prob=math.inf), "prob"), (dict(GOOD, prob=-0.1), "prob"), (dict(GOOD, prob=1.5), "prob"),
    (dict(GOOD, lin_vel=(math.nan, 0.6)), "lin_vel"), (dict(GOOD, lin_vel=(0.2, math.inf)), "lin_vel"), (dict(GOOD, lin_vel=(-0.2, 0.6)), "lin_vel"),
    (dict(GOOD, lin_vel=(0.7, 0.6)), "lin_vel"), (dict(GOOD, lin_vel=0.5), "lin_vel"), (dict(GOOD, lin_vel=(0.1, 0.2, 0.3)), "lin_vel"),
    (dict(GOOD, lin_vel_z=math.nan), "lin_vel_z"), (dict(GOOD, lin_vel_z=-0.2), "lin_vel_z"), (dict(GOOD, lin_vel_z=math.inf), "lin_vel_z"),
    (dict(GOOD, ang_vel=math.nan), "ang_vel"), (dict(GOOD, ang_vel=-0.5), "ang_vel"), (dict(GOOD, ang_vel="fast"), "ang_vel"),
    (dict(GOOD, interval_s=2.0), "prob and interval_s"), ({k: v for k, v in GOOD.items() if k != "prob"}, "prob and interval_s"),
    (dict({k: v for k, v in GOOD.items() if k != "prob"}, interval_s=0.0), "interval_s"),
    (dict({k: v for k, v in GOOD.items() if k != "prob"}, interval_s=0.01), "interval_s"),          # 0.033 / 0.01 > 1
    (dict(GOOD, grace_steps=-1), "grace_steps"), (dict(GOOD, grace_steps=1.5), "grace_steps"), (dict(GOOD, grace_steps=True), "grace_steps"),
    (dict(GOOD, lin_vel=(0.2, 100.5)), "lin_vel hi"), (dict(GOOD, lin_vel_z=101.0), "lin_vel_z"), (dict(GOOD, ang_vel=1e3), "ang_vel"),
    (dict(GOOD, strength=1.0), "strength"), ("hard", "push"), ([0.25, 0.2, 0.6], "push")])
def test_spec_refusals(bad, needle):
    with pytest.raises(ValueError) as e:
        envmod.push_spec(bad)
    assert needle in str(e.value)


def test_spec_values_and_interval():
    """None = all zero; the fields land where the struct has them; interval_s means prob = action_repeat * sim_dt / interval_s; the
    velocity bound itself is accepted."""
    z = envmod.push_spec(None)
    assert (z.prob, z.lin_lo, z.lin_hi, z.lin_z, z.ang, z.grace_steps) == (0.0, 0.0, 0.0, 0.0, 0.0, 0) and not envmod.push_on(z)
    s = envmod.push_spec(GOOD)
    f = lambda x: float(np.float32(x))
    assert (s.prob, s.lin_lo, s.lin_hi, s.lin_z, s.ang, s.grace_steps) == (f(0.25), f(0.2), f(0.6), f(0.2), f(0.5), 2) and envmod.push_on(s)
    s = envmod.push_spec(dict(interval_s=3.3, lin_vel=(0.0, 1.0)))
    assert s.prob == f(33 * 0.001 / 3.3) and (s.lin_z, s.ang, s.grace_steps) == (0.0, 0.0, 0)
    s = envmod.push_spec(dict(interval_s=2.0), action_repeat=10, sim_dt=0.002)
    assert s.prob == f(10 * 0.002 / 2.0)
    s = envmod.push_spec(dict(prob=1.0, lin_vel=(100.0, 100.0), lin_vel_z=100.0, ang_vel=100.0))
    assert s.prob == 1.0 and s.lin_hi == 100.0
    with pytest.raises(ValueError, match="lin_vel_z"):
        envmod.push_spec(dict(prob=0.5, lin_vel_z=60.0), max_coord_velocity=50.0)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_block_arithmetic():
    """Blocks A = 0x50000000 + 2 s and B = A + 1 for s < 2^27 lie in [0x50000000, 0x60000000), apart from the sensor-noise blocks (below
    0x20000000), the task noise's (0x2..., 0x3...) and the randomiser's two."""
    assert _abi.PUSH_BLOCK == 0x50000000
    s = np.array([0, 1, 2, 599, (1 << 27) - 1], dtype=np.int64)
    a, b = envmod.push_block(s)
    assert list(a[:3]) == [0x50000000, 0x50000002, 0x50000004] and (b == a + 1).all()
    assert a.min() >= 0x50000000 and b.max() == 0x5FFFFFFF < 0x60000000
    assert len(set(a) | set(b)) == 2 * len(s)                                   # no block serves two steps
    top_sensor = int(envmod.sensor_noise_block((1 << 19) - 1, 31, 15))
    assert envmod.SENSOR_NOISE_BLOCK <= top_sensor < 0x20000000 == envmod.NOISE_RESET_BLOCK
    assert envmod.NOISE_RESET_BLOCK + 15 < envmod.NOISE_HEADING_BLOCK == 0x30000000
    assert int(envmod.tar_noise_block((1 << 27) - 1)) < _abi.RAND_BLOCK == 0x40000000 and _abi.RAND_BLOCK + 1 < a.min()
    for bad in (-1, 1 << 27):
        with pytest.raises(ValueError):
            envmod.push_block(bad)
    a0, b0 = envmod.push_block(7)
    assert (int(a0), int(b0)) == (0x5000000E, 0x5000000F)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def predictor_run(seed):
    L = ol.lib()
    spec = envmod.push_spec(GOOD)
    s = np.repeat(np.arange(40), 37)
    robot = np.tile(np.arange(37), 40)
    u8 = np.array([pl.stream_u8(L, seed, r, 1, k) for r, k in zip(robot, s)])
    return spec, s, u8, envmod.push_kick(spec, u8, s=s)


def test_predictor_on_the_oracles_stream():
    """37 robots x 40 steps of episode 1, seed 4: the kicked share of the robot-steps past the grace period lies within four binomial
    standard deviations of prob; |dv_xy| in [lin_lo, lin_hi], |dv_z| <= lin_z, |dw_k| <= ang; nothing below grace_steps; an unkicked
    robot's kick is exactly zero; the same seed gives the same bits, another seed other kicks."""
    spec, s, u8, (kicked, dv, dw) = predictor_run(4)
    assert ((u8 >= 0) & (u8 < 1)).all() and (u8 * 16777216.0 == np.rint(u8 * 16777216.0)).all()       # 24-bit fractions
    past = s >= spec.grace_steps
    assert not kicked[~past].any() and (u8[~past, 0] < spec.prob).any()          # the grace period suppressed kicks that the draw asked for
    n, p = int(past.sum()), float(spec.prob)
    assert abs(kicked[past].sum() - n * p) <= 4.0 * math.sqrt(n * p * (1 - p)), (int(kicked.sum()), n * p)
    mag = np.hypot(dv[kicked, 0], dv[kicked, 1])
    eps = 1e-12
    assert (mag >= spec.lin_lo - eps).all() and (mag <= spec.lin_hi + eps).all() and mag.max() - mag.min() > 0.3
    assert (np.abs(dv[kicked, 2]) <= spec.lin_z).all() and (np.abs(dw[kicked]) <= spec.ang).all()
    assert (dv[kicked, 0] < 0).any() and (dv[kicked, 1] < 0).any() and (dv[kicked, 2] < 0).any() and (dw[kicked] < 0).any()    # every direction
    assert not dv[~kicked].any() and not dw[~kicked].any()
    again = predictor_run(4)[3]
    assert all(np.array_equal(x, y) for x, y in zip(again, (kicked, dv, dw)))
    other = predictor_run(5)[3]
    assert not np.array_equal(other[0], kicked)
    # without an angular bound block B is not used
    k2, dv2, dw2 = envmod.push_kick(envmod.push_spec(dict(GOOD, ang_vel=0.0)), u8, s=s)
    assert np.array_equal(k2, kicked) and np.array_equal(dv2, dv) and not dw2.any()


def test_abi_against_header():
    """Struct, entry points, row size and the draw rule's blocks of include/openroborl_hip.h against _abi.py and the built library."""
    with open(os.path.join(ROOT, "include", "openroborl_hip.h")) as f:
        header = f.read()
    m = re.search(r"typedef struct orr_push \{(.*?)\} orr_push;", header, re.S)
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+);", m.group(1), re.M)
    assert fields == [("float", "prob"), ("float", "lin_lo"), ("float", "lin_hi"), ("float", "lin_z"), ("float", "ang"), ("int32_t", "grace_steps")]
    assert [f[0] for f in _abi.OrrPush._fields_] == [n for _, n in fields] and C.sizeof(_abi.OrrPush) == 24
    assert re.search(r"int32_t orr_set_push\(orr_handle\* h, const orr_push\* push_host\);", header)
    assert re.search(r"int32_t orr_sizeof_push\(void\);", header)
    assert re.search(r"int32_t orr_bind_push_outputs\(orr_handle\* h, float\* push_dev[^;]*\);", header)
    assert re.search(r"#define ORR_PUSH_ROW 8\b", header) and _abi.PUSH_ROW == 8
    assert re.search(r"#define ORR_ABI_VERSION 5\b", header) and _abi.ABI_VERSION == 5       # additive
    assert "0x50000000 + 2 s" in header and "0x60000000" in header
    for name in ("orr_set_push", "orr_sizeof_push", "orr_bind_push_outputs"):
        assert name in _lib.EXPORTS
    assert _lib.PUSH_UNITS == [("push", _lib.SRC_PUSH, _lib.HIPCC_FLAGS, False)]
    L = _lib.load()
    assert L.orr_sizeof_push() == C.sizeof(_abi.OrrPush)
    assert L.orr_set_push(None, None) == -1 and b"orr_set_push: null handle" in L.orr_last_error()
    assert L.orr_bind_push_outputs(None, None) == -1 and b"orr_bind_push_outputs: null handle" in L.orr_last_error()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_inputs_of_the_gpu_physics_comparison_are_sound():
    """push_lib.cpu_run: the float64 oracle with the predictor's kicks (added to the record's LINVEL / ANGVEL, rounded to float32 as the
    device holds it), from each pre-step record the float32 parity oracle; the floor rule per rigid field.  The float32 oracle alone must
    leave at most 0.5 % of the cells of any field over the bound (the project's cap: a condition on the inputs, not a measurement), and
    the unkicked float64 step must lie outside the bound in more than 10 % of all cells - else the GPU comparison could not tell a
    device that applies the kick from one that only reports it.
    Measured on the real stream, env seed 4 (push_lib.SEED), action seed 11: 374 kicks in 1480 robot-steps; float32 oracle over the
    bound in at most 0.006 % of the cells of a field (Q; 0 in the others); the unkicked step outside the bound in 24.2 % of all cells."""
    R = pl.cpu_run()
    ok = ~R["nan"]
    per, outside = pl.shares(R["ref"], R["f32"], R["free"], ok=ok)
    print("PUSH cpu run: %d kicks in %d robot-steps, %d non-finite; the unkicked float64 step outside the bound in %.1f %% of all cells" % (
        int(R["kicked"].sum()), R["kicked"].size, int(R["nan"].sum()), 100 * outside))
    for name, r in per.items():
        print("PUSH cpu run %s: %s | unkicked outside %.1f %%" % (name, al.describe(r), 100 * r["free_share"]))
        assert r["f32_share"] <= al.F32_SHARE, "the inputs are at fault: " + name
    assert outside > 0.10
    assert 0.15 * R["kicked"].size < R["kicked"].sum() < 0.35 * R["kicked"].size
    assert (R["s"] == 0).sum() > pl.N                      # auto-reset: episodes ended and began inside the run
