#!/usr/bin/env python3
"""Golden fixture of the task noise (ImitationTask's perturb_init_state_prob / tar_obs_noise) from the reference's OWN Python.

Run ONLY in the build container (needs /root/reference; the GPU box never has it):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_init_noise.py

The pipeline of make_golden_task.py (WrapperEnv -> LocomotionGymEnv -> Minitaur + ImitationTask over the scripted client
tests/golden/fake_bullet.py), reused by import, with the one-clip Laikago task of run.py:58-64 and perturb_init_state_prob = 0.5,
tar_obs_noise = [0.1]: make_golden_task.py's ImitationTask constructor is replaced by one that passes these two arguments (the
reference class itself, unmodified).

Draws.  Each task instance's _rand_uniform / _randn is replaced, by call site, with the device's value for the same key: the oracle's
orc_uniform(seed, robot index, episode, index) (the device's Philox stream) at the indices of include/openroborl_hip.h,
orr_set_task_noise, pushed through the float64 normal_pair of openroborl_amd/env.py:
    reset:  26 ref-state-init, 27 time offset (as make_golden_clip_switch.py), then U(0) = draw 4 * 0x20000000 (the perturbation test);
            in _apply_state_perturb the axis is U(1..3) (lo + (hi - lo) u) and the _randn calls consume z0, z1, ... in call order, a
            vector call consecutive ones, z_2j / z_2j+1 = normal_pair(U(4 + 2j), U(5 + 2j))
    build_target_obs:  z0 of normal_pair(word 0, word 1) of block 0x30000000 + i, i = 0 at a reset, 1 + s in the step whose env step
            counter before the step is s
The number of draws per reset (3 uniform calls + 1 normal, or 4 uniform calls + 8 normal calls = 32 values + 1) and per step (1 normal)
is asserted, and that both perturbed and unperturbed resets were recorded.  Draws 0..25 (randomiser) are off.

Output (committed): task_laikago_noise.npz.  Beyond make_golden_task.py's per-step arrays (stored as in make_golden_clip_switch.py):
per reset and robot whether it was perturbed, the perturbation = teleported state - reference state (37 words, rigid-state layout) and
the heading noise; per step the heading noise.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
import make_golden_task as mgt  # noqa: E402  (sets up the reference's import path and working directory)
from openroborl_amd import env as envmod  # noqa: E402
from tests import oracle_lib as ol  # noqa: E402

SEED = int(os.environ.get("ORR_GOLDEN_SEED", 3))
PROB, SIGMA = 0.5, 0.1
N, EPISODES, EP_STEPS = 8, 3, int(os.environ.get("ORR_GOLDEN_EP_STEPS", 5))


class Draws(object):
    """The device's draws for the reference's call sites (see the module docstring)."""

    def __init__(self, seed):
        self.L = ol.lib()
        self.seed = seed
        self.ep = 0          # episode of the device's stream (the first replayed reset is episode 1)
        self.obs_i = 0       # index of the next target observation of the episode: 0 at a reset, 1 + s in a step
        self.live = False    # before the first recorded reset (the env constructor's reset): arbitrary values, not recorded

    def u(self, robot, k):
        return float(self.L.orc_uniform(self.seed, robot, self.ep if self.live else 0, int(k)))

    def U(self, robot):
        return np.array([self.u(robot, d) for d in envmod.init_perturb_draw_indices()])

    def install(self, task, robot):
        task._cnt = {"uni": 0, "uni3": 0, "randn": 0, "z": 0, "heading": 0}
        task._heading_noise = 0.0

        def uniform(lo, hi, size=None, _t=task):
            site, outer = sys._getframe(1).f_code.co_name, sys._getframe(2).f_code.co_name
            if site == "_apply_state_perturb":
                assert list(size) == [3] and (lo, hi) == (-1, 1)
                _t._cnt["uni3"] += 1
                return lo + (hi - lo) * self.U(robot)[1:4]
            assert size is None
            log = False
            if site == "reset":
                if _t._cnt["uni"] == 0:       # imitation_task.py:183: reference state initialisation
                    k, log = 26, True
                else:                         # :194: the perturbation test
                    assert _t._cnt["uni"] == 2 and (lo, hi) == (0.0, 1.0)
                    k = int(envmod.init_perturb_draw_indices()[0])
            elif site == "_reset_motion_time_offset" or (site == "_sample_time_offset" and outer == "_reset_motion_time_offset"):
                k, log = 27, True
            else:
                raise AssertionError("unexpected draw site %s / %s" % (site, outer))
            _t._cnt["uni"] += 1
            v = lo + (hi - lo) * self.u(robot, k)
            if log:                       # make_golden_task.reset_record reads the ref-state-init and time-offset draws from _draws
                _t._draws.append((lo, hi, v))
            return v

        def randn(mean, std, size=None, _t=task):
            site = sys._getframe(1).f_code.co_name
            if site == "build_target_obs":
                assert size is None and mean == 0
                blk = int(envmod.tar_noise_block(None if self.obs_i == 0 else self.obs_i - 1))
                z = float(envmod.normal_pair(self.u(robot, 4 * blk), self.u(robot, 4 * blk + 1))[0])
                _t._cnt["heading"] += 1
                _t._heading_noise = std * z
                return std * z + mean
            assert site == "_apply_state_perturb" and mean == 0, site
            n = 1 if size is None else int(np.prod(size))
            z = envmod.init_perturb_draws(self.U(robot), PROB)["z"][_t._cnt["z"]:_t._cnt["z"] + n]
            assert len(z) == n
            _t._cnt["z"] += n
            _t._cnt["randn"] += 1
            return std * (float(z[0]) if size is None else z.reshape(size)) + mean

        task._rand_uniform = uniform
        task._randn = randn


def main():
    D = Draws(SEED)
    ref_cls = mgt.imitation_task.ImitationTask

    def task_factory(**kw):
        return ref_cls(perturb_init_state_prob=PROB, tar_obs_noise=[SIGMA], **kw)
    mgt.imitation_task = types.SimpleNamespace(ImitationTask=task_factory)

    orig_build, orig_reset, orig_step = mgt.build, mgt.reset_record, mgt.step_record

    def build(*a, **kw):
        env, robots, tasks = orig_build(*a, **kw)
        for i, t in enumerate(tasks):
            D.install(t, i)                # replaces make_golden_task's logging wrapper of _rand_uniform (the draws log themselves)
        return env, robots, tasks

    def zero(t):
        t._cnt = {k: 0 for k in t._cnt}

    def reset_record(env, robots, tasks, fake):
        D.live = True
        D.ep += 1
        D.obs_i = 0
        for t in tasks:
            zero(t)
        out = orig_reset(env, robots, tasks, fake)
        for i, t in enumerate(tasks):
            pert = t._cnt["uni3"] == 1
            assert t._cnt == ({"uni": 3, "uni3": 1, "randn": 8, "z": 32, "heading": 1} if pert else
                              {"uni": 3, "uni3": 0, "randn": 0, "z": 0, "heading": 1}), t._cnt
            assert pert == (D.u(i, envmod.init_perturb_draw_indices()[0]) < PROB)
            rp, rv = np.asarray(t._ref_pose, dtype=np.float64), np.asarray(t._ref_vel, dtype=np.float64)
            ref = np.concatenate([rp[0:7], rv[0:6], rp[7:19], rv[6:18]])       # the rigid-state layout of state37
            out[i].update(perturbed=float(pert), perturb_delta=out[i]["state37"] - ref, heading_noise=float(t._heading_noise))
            if not pert:
                assert not out[i]["perturb_delta"].any()
        D.obs_i = 1
        return out

    def step_record(env, robots, tasks, fake, actions):
        for t in tasks:
            zero(t)
        out, done = orig_step(env, robots, tasks, fake, actions)
        for i, t in enumerate(tasks):
            assert t._cnt == {"uni": 0, "uni3": 0, "randn": 0, "z": 0, "heading": 1}, t._cnt
            out[i].update(heading_noise=float(t._heading_noise))
        D.obs_i += 1
        return out, done

    mgt.build, mgt.reset_record, mgt.step_record = build, reset_record, step_record
    out = mgt.run("laikago", N, False, EP_STEPS, EP_STEPS, 30000000, seed=SEED, total_steps=EPISODES * EP_STEPS, events={})
    pert = out["reset/perturbed"].astype(bool)
    assert pert.shape == (EPISODES, N), pert.shape        # every episode ran into its time limit: EPISODES whole-env resets
    assert pert.any() and not pert.all(), "the seed must give perturbed and unperturbed resets"
    out["seed"] = np.float64(SEED)
    out["noise"] = np.array([PROB, SIGMA])
    # size: the device consumes float32 - store the bulky per-sub-step arrays and the observations as float32, drop the reward terms
    traj = out.pop("step/traj_f32").astype(np.float64)
    traj[..., 3:7] = out.pop("step/traj_quat")
    out["step/traj"] = traj.astype(np.float32)
    for k in ("step/tau_urdf", "step/obs", "reset/obs"):
        out[k] = out[k].astype(np.float32)
    for k in ("step/terms", "step/ctrl_obs", "step/filtered_action", "step/action_mutated"):
        out.pop(k)
    path = os.path.join(HERE, "task_laikago_noise.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("task_laikago_noise.npz %d KiB: %d robots, %d resets (%d of %d robot resets perturbed), %d steps, |heading noise| up to %.3f rad" % (
        size // 1024, N, pert.shape[0], pert.sum(), pert.size, out["step/done"].shape[0],
        max(np.abs(out["step/heading_noise"]).max(), np.abs(out["reset/heading_noise"]).max())))


if __name__ == "__main__":
    main()
