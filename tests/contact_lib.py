"""What tests/test_contact_outputs_cpu.py and tests/test_gpu_contact_outputs.py share: the reduction of the CPU oracle's sub-step trace
(orc_set_substep_trace) to the layout of contact_out, the inputs of the product-path comparison (mixed batch, each robot's shipped
policy + seeded noise), and the floor rule that bounds the device's contact sums by the float32 parity oracle's own deviation."""
import ctypes as C
import functools
import os

import numpy as np

from openroborl_amd import _abi, config, motion, robots
from tests import oracle_lib as ol
from tests.gpu_kit import CLIP, MIXED

POLICY = {"laikago": "policy_laikago_pace.npz", "mini_cheetah": "policy_minicheetah_trot.npz"}
N, STEPS, SEED, ACTION_SEED, ACTION_STD = 37, 40, 3, 11, 0.05      # the product-path comparison: ten waves, the last with one valid robot
F32_SHARE, DEVICE_SHARE, MIN_LIVE = 0.005, 0.02, 1000               # shares of live leg-steps that may hold a cell over the bound
ULP = 2.0 ** -22


def reduce_trace(trace):
    """Oracle trace [n][action_repeat][>= 12] (words 0..11 = (n, t1, t2) x leg) -> [n, 4, 4] in contact_out's layout: per leg the
    sums of the three impulses over the sub-steps and the largest normal impulse, added in sub-step order from 0 in the trace's own
    number format (float32 for the parity build: the device's order and format), the maximum from 0 too."""
    trace = np.asarray(trace)
    n, rep = trace.shape[0], trace.shape[1]
    lam = trace[:, :, 0:12].reshape(n, rep, 4, 3)
    out = np.zeros((n, 4, 4), dtype=trace.dtype)
    for s in range(rep):
        out[:, :, 0:3] = out[:, :, 0:3] + lam[:, s]
        out[:, :, 3] = np.maximum(out[:, :, 3], lam[:, s, :, 0])
    return out


def mixed_setup(n=N, seed=SEED, **cfg_kw):
    """(cfg, models, clips, robot_type, clip_id) as VecQuadrupedEnv(num_robot=n, mixed_robots=MIXED, motion_file=[their clips], mode="train",
    enable_randomizer=True, auto_reset=False, seed=seed) builds them"""
    cfg_kw.setdefault("auto_reset", False)
    cfg = config.make_config(n, sim_params=config.load_sim_params(None), mode="train", enable_randomizer=True, seed=seed, num_procs=1, legacy_grid=False, **cfg_kw)
    models = [None] * _abi.MAX_ROBOT_TYPES
    for name in MIXED:
        models[robots.ROBOT_TYPE_ID[name]] = robots.ROBOTS[name]()
    clips = [motion.MotionClip(CLIP[name]) for name in MIXED]
    robot_type = np.array([robots.ROBOT_TYPE_ID[MIXED[i % len(MIXED)]] for i in range(n)], dtype=np.int32)
    clip_id = np.array([i % len(MIXED) for i in range(n)], dtype=np.int32)
    return cfg, models, clips, robot_type, clip_id


@functools.lru_cache(maxsize=None)
def policies():
    """{robot type id: the shipped policy's weights (float32)}"""
    out = {}
    for name in MIXED:
        W = np.load(os.path.join(ol.GOLDEN, POLICY[name]))
        out[robots.ROBOT_TYPE_ID[name]] = {k: W[k].astype(np.float32) for k in W.files}
    return out


def policy_actions(obs, robot_type, rng, std=ACTION_STD):
    """Each robot's shipped policy applied in numpy (float32) to its observation, + N(0, std) from `rng`, clipped to +-2 pi: float32 [n, 12]"""
    obs = np.asarray(obs, dtype=np.float32)
    act = np.zeros((obs.shape[0], 12), dtype=np.float32)
    for t, w in policies().items():
        m = robot_type == t
        h = np.maximum(obs[m] @ w["model__pi_fc0__w_0"] + w["model__pi_fc0__b_0"], 0.0)
        h = np.maximum(h @ w["model__pi_fc1__w_0"] + w["model__pi_fc1__b_0"], 0.0)
        act[m] = h @ w["model__pi__w_0"] + w["model__pi__b_0"]
    act = act + rng.normal(0.0, std, act.shape).astype(np.float32)
    return np.clip(act, -2 * np.pi, 2 * np.pi).astype(np.float32)


class TracedOracle(object):
    """An OracleEnv (float64, or the float32 parity build) with the sub-step trace on"""

    def __init__(self, cfg, models, clips, n, robot_type, clip_id, f32=False):
        self.orc = ol.OracleEnv(cfg, models, clips, n, robot_type=robot_type, clip_id=clip_id, f32="parity" if f32 else False)
        L = self.orc.L
        self.words = int(L.orc_trace_words())
        self.trace = np.zeros((n, int(cfg.action_repeat), self.words), dtype=self.orc.dt)
        L.orc_set_substep_trace.argtypes = [C.c_void_p, C.POINTER(C.c_float if f32 else C.c_double)]
        L.orc_set_substep_trace(self.orc.h, self.orc.P(self.trace))

    def step_from(self, state64, counters, act):
        """One env step of every robot from the given records (float64 layout) and counters -> reduce_trace of the step, float64 [n, 4, 4]"""
        self.orc.state[:] = state64.astype(self.orc.dt)
        self.orc.counters[:] = counters
        self.trace[:] = 0
        self.orc.step(act)
        return reduce_trace(self.trace).astype(np.float64)

    def close(self):
        self.orc.L.orc_set_substep_trace(self.orc.h, None)
        self.orc.close()


def floor_rule(ref, f32, dev=None):
    """ref, f32 (, dev): [steps, n, 4, 4] contact rows of the float64 oracle, of the float32 parity oracle and of the device, every step
    started from the same record.  A leg-step is live when the float64 normal sum is > 0; q = the 99th percentile of |f32 - ref| over
    the live cells; cell bound = 4 q + 2^-22 max(1, |ref|).  -> dict: q, live, the share of live leg-steps with a cell over the bound
    for f32 and for dev (dev's also counts the dead leg-steps that are not exactly zero), and dev's worst cell."""
    ref, f32 = np.asarray(ref, dtype=np.float64), np.asarray(f32, dtype=np.float64)
    live = ref[..., 0] > 0
    q = float(np.percentile(np.abs(f32 - ref)[live], 99)) if live.any() else 0.0
    bound = 4.0 * q + ULP * np.maximum(1.0, np.abs(ref))
    out = {"q": q, "live": int(live.sum()), "leg_steps": int(live.size)}
    over32 = (np.abs(f32 - ref) > bound).any(axis=-1)
    out["f32_share"] = float((over32 & live).sum()) / max(out["live"], 1)
    out["f32_dead_nonzero"] = int(((f32 != 0).any(axis=-1) & ~live).sum())
    if dev is not None:
        dev = np.asarray(dev, dtype=np.float64)
        err = np.abs(dev - ref)
        over = (err > bound).any(axis=-1) & live
        dead_nonzero = (dev != 0).any(axis=-1) & ~live
        out["dev_share"] = float(over.sum() + dead_nonzero.sum()) / max(out["live"], 1)
        out["dev_dead_nonzero"] = int(dead_nonzero.sum())
        k = np.unravel_index(np.argmax(np.where(live[..., None], err, 0.0)), err.shape)
        out["dev_worst"] = (float(err[k]), float(ref[k]), tuple(int(x) for x in k))
    return out


def describe(r):
    s = "q99 %.3e N s | live leg-steps %d of %d | float32 oracle over the bound %.3f %% (dead non-zero %d)" % (
        r["q"], r["live"], r["leg_steps"], 100 * r["f32_share"], r["f32_dead_nonzero"])
    if "dev_share" in r:
        s += " | device over the bound %.3f %% (dead non-zero %d), worst cell |d| %.3e at ref %.4f (step, robot, leg, column) %s" % (
            (100 * r["dev_share"], r["dev_dead_nonzero"]) + r["dev_worst"])
    return s
