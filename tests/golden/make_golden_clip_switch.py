#!/usr/bin/env python3
"""Golden fixture of mid-episode clip switching (ImitationTask's clip_time_min / clip_time_max) from the reference's OWN Python.

Run ONLY in the build container (needs /root/reference; the GPU box never has it):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_clip_switch.py

The pipeline of make_golden_task.py (WrapperEnv -> LocomotionGymEnv -> Minitaur + ImitationTask over the scripted client
tests/golden/fake_bullet.py), reused by import, with a four-clip task: pace, trot, spin and a copy of backwards_trot with
"LoopMode": "Clamp" (every shipped clip wraps; a clamped clip ends its episode by MOTION_OVER), clip_time_min / clip_time_max set,
the rest as run.py:58-64.  make_golden_task.py builds one-clip tasks: its ImitationTask constructor is replaced by one that passes
these arguments (the reference class itself, unmodified).

Draws.  Each task instance's _randint / _rand_uniform is replaced, by call site, with the device's value for the same key: the oracle's
orc_uniform(seed, robot index, episode, index) (the device's Philox stream), mapped as the reference maps a uniform draw
(numpy: low + (high - low) u; randint(0, n) -> (m n) >> 24, m = the 24-bit integer of u):
    reset:  26 ref-state-init, 27 time offset, 28 clip, 29 first clip change (the extra _sample_ref_motion of the first reset,
            imitation_task.py:174, is skipped: it is overwritten by _reset_ref_motion)
    update of the env step whose counter before the step is s, when the clip changes: 32 + 4 s clip, 33 + 4 s next change,
            34 + 4 s time offset
The number of draws per reset (1 integer + 3 uniform) and per update (0, or 1 + 2) is asserted.  Draws 0..25 (randomiser) are off.

Output (committed): task_laikago_clipswitch.npz.  Beyond make_golden_task.py's per-step arrays (traj, torques and observations stored
as float32 to keep the file under 1 MiB; the device consumes float32): per step and robot the active clip, whether it switched, the
time offset, origin, PREV_PHASE, CLIP_CHANGE_TIME, reference pose / velocity, the old clip's phase-wrap flag at a switch and the smallest
|t - change time| seen by the switch test; per reset the clip and CLIP_CHANGE_TIME.  The switch interval is shorter than the
0.3 .. 0.8 s of a training run so that the file holds enough switches within its size.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
import make_golden_task as mgt  # noqa: E402  (sets up the reference's import path and working directory)
from tests import oracle_lib as ol  # noqa: E402

SEED = int(os.environ.get("ORR_GOLDEN_SEED", 2))
TMIN, TMAX = float(np.float32(0.05)), float(np.float32(0.15))     # float32-exact: the device holds the bounds as float32
NAMES = ["laikago_pace", "laikago_trot", "laikago_spin", "laikago_backwards_trot_clamp"]


def clamped_copy(dst_dir):
    with open(os.path.join(mgt.MOTIONS, "laikago_backwards_trot.txt")) as f:
        clip = json.load(f)
    assert clip["LoopMode"] == "Wrap"
    clip["LoopMode"] = "Clamp"
    dst = os.path.join(dst_dir, "laikago_backwards_trot_clamp.txt")
    with open(dst, "w") as f:
        json.dump(clip, f)
    return dst


class Draws(object):
    """The device's draws for the reference's call sites (see the module docstring)."""

    def __init__(self, seed):
        self.L = ol.lib()
        self.seed = seed
        self.ep = 0          # episode of the device's stream (the first replayed reset is episode 1)
        self.s = 0           # env step counter of the episode before the current step
        self.live = False    # before the first recorded reset (the env constructor's reset): arbitrary values, not recorded

    def u(self, robot, k):
        return float(self.L.orc_uniform(self.seed, robot, self.ep if self.live else 0, int(k)))

    def install(self, task, robot):
        task._robot_idx = robot
        task._cnt = {"int": 0, "uni": 0}
        task._gap = np.inf      # smallest |t - change time| the switch test saw this step
        task._wrap = False
        orig_check = task._check_change_clip

        def randint(lo, hi, size=None, _t=task):
            assert size is None and lo == 0
            site, outer = sys._getframe(1).f_code.co_name, sys._getframe(2).f_code.co_name
            assert site == "_sample_ref_motion", site
            if outer == "reset":          # imitation_task.py:174: the first reset's extra draw, overwritten right after
                return 0
            if outer == "_reset_ref_motion":
                k = 28
            else:
                assert outer == "_update_ref_motion", outer
                k = 32 + 4 * self.s
                old = _t.get_active_motion()
                _t._wrap = old.calc_phase(_t._get_motion_time()) < _t._prev_motion_phase
            _t._cnt["int"] += 1
            m = int(round(self.u(robot, k) * (1 << 24)))
            return (m * int(hi)) >> 24

        def uniform(lo, hi, size=None, _t=task):
            assert size is None
            site, outer = sys._getframe(1).f_code.co_name, sys._getframe(2).f_code.co_name
            log = False
            if site == "reset":
                k, log = 26, True
            elif site == "_reset_motion_time_offset" or (site == "_sample_time_offset" and outer == "_reset_motion_time_offset"):
                k, log = 27, True
            elif site == "_sample_time_offset":
                assert outer == "_update_ref_motion", outer
                k = 34 + 4 * self.s
            elif site == "_reset_clip_change_time":
                k = 29 if outer == "_reset_ref_motion" else 33 + 4 * self.s
                assert outer in ("_reset_ref_motion", "_update_ref_motion"), outer
            else:
                raise AssertionError("unexpected draw site %s / %s" % (site, outer))
            _t._cnt["uni"] += 1
            v = lo + (hi - lo) * self.u(robot, k)
            if log:                       # make_golden_task.reset_record reads the ref-state-init and time-offset draws from _draws
                _t._draws.append((lo, hi, v))
            return v

        def check(_t=task):
            t = _t._get_motion_time()
            if np.isfinite(_t._clip_change_time):
                _t._gap = min(_t._gap, abs(t - _t._clip_change_time))
            return orig_check()

        task._randint = randint
        task._rand_uniform = uniform
        task._check_change_clip = check


def main():
    tmp = tempfile.mkdtemp()
    files = [os.path.join(mgt.MOTIONS, n + ".txt") for n in NAMES[:3]] + [clamped_copy(tmp)]
    D = Draws(SEED)
    ref_cls = mgt.imitation_task.ImitationTask

    def task_factory(**kw):
        kw["ref_motion_filenames"] = files
        return ref_cls(clip_time_min=TMIN, clip_time_max=TMAX, **kw)
    mgt.imitation_task = types.SimpleNamespace(ImitationTask=task_factory)

    orig_build, orig_reset, orig_step = mgt.build, mgt.reset_record, mgt.step_record

    def build(*a, **kw):
        env, robots, tasks = orig_build(*a, **kw)
        for i, t in enumerate(tasks):
            D.install(t, i)                # replaces make_golden_task's logging wrapper of _rand_uniform (the draws log themselves)
        return env, robots, tasks

    def reset_record(env, robots, tasks, fake):
        D.live = True
        D.ep += 1
        D.s = 0
        for t in tasks:
            t._cnt = {"int": 0, "uni": 0}
        out = orig_reset(env, robots, tasks, fake)
        for i, t in enumerate(tasks):
            assert t._cnt == {"int": 1, "uni": 3}, t._cnt
            out[i].update(clip_id=float(t._active_motion_id), clip_change_time=float(t._clip_change_time))
        return out

    def step_record(env, robots, tasks, fake, actions):
        before = [t._active_motion_id for t in tasks]
        for t in tasks:
            t._cnt = {"int": 0, "uni": 0}
            t._gap, t._wrap = np.inf, False
        out, done = orig_step(env, robots, tasks, fake, actions)
        for i, t in enumerate(tasks):
            switched = t._cnt["int"] == 1
            assert t._cnt == ({"int": 1, "uni": 2} if switched else {"int": 0, "uni": 0}), t._cnt
            out[i].update(clip_id=float(t._active_motion_id), clip_before=float(before[i]), switched=float(switched),
                          wrap_at_switch=float(switched and t._wrap), gap=float(t._gap), warmup=float(t._curr_episode_warmup),
                          time_offset=float(t._motion_time_offset), origin_rot=np.array(t._origin_offset_rot, dtype=np.float64),
                          clip_change_time=float(t._clip_change_time), motion_over=float(t.is_motion_over()))
        D.s += 1
        return out, done

    mgt.build, mgt.reset_record, mgt.step_record = build, reset_record, step_record
    out = mgt.run("laikago", 2, False, 600, 600, 30000000, seed=SEED, total_steps=int(os.environ.get("ORR_GOLDEN_STEPS", 70)), events={})
    out["clip"] = np.array(",".join(NAMES))
    out["clip_names"] = np.array(NAMES)
    out["seed"] = np.float64(SEED)
    out["clip_time"] = np.array([TMIN, TMAX])
    # size: the device consumes float32 - store the bulky per-sub-step arrays and the observations as float32, drop the reward terms
    traj = out.pop("step/traj_f32").astype(np.float64)
    traj[..., 3:7] = out.pop("step/traj_quat")
    out["step/traj"] = traj.astype(np.float32)
    for k in ("step/tau_urdf", "step/obs", "reset/obs"):
        out[k] = out[k].astype(np.float32)
    for k in ("step/terms", "step/ctrl_obs", "step/filtered_action", "step/action_mutated"):
        out.pop(k)
    path = os.path.join(HERE, "task_laikago_clipswitch.npz")
    np.savez_compressed(path, **out)
    sw = out["step/switched"].astype(bool)
    print("task_laikago_clipswitch.npz %d KiB: %d steps, %d resets, %d switches (%d same clip, %d warm-up, %d phase wrap), "
          "smallest gap %.3g s, motion-over ends on the clamped clip %d" % (
              os.path.getsize(path) // 1024, sw.shape[0], out["reset/clip_id"].shape[0], sw.sum(),
              (sw & (out["step/clip_id"] == out["step/clip_before"])).sum(), (sw & (out["step/warmup"] > 0)).sum(),
              (out["step/wrap_at_switch"] > 0).sum(), out["step/gap"].min(),
              ((out["step/done"] > 0) & (out["step/motion_over"] > 0) & (out["step/clip_id"] == 3)).sum()))


if __name__ == "__main__":
    main()
