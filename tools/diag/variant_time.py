"""Step time of a variant of the step kernel against its baseline, 4096 robots, same process, alternated (train semantics):
python tools/diag/variant_time.py --case noise|terms|contacts|actuator|sensor|randomizer|push|anchor

  noise     the task-noise variant against the clip-set variant (a two-clip set, so that the plain env runs the clip-set variant)
  terms     reward terms on top of task noise               (two-clip set, noise on in all at one setting: prob 0.5, sigma 0.1)
  contacts  contact outputs, then reward terms as well, on top of task noise (the same set and noise); also the logged episodes' gait
  actuator  torque limits 20 / 30 / 40 N m per leg + actuator outputs on top of contact outputs + reward terms (all three bindings on)
            against that variant (MODE 12), the same set and noise; in between the actuator variant WITHOUT limits, which computes what
            MODE 12 computes: the kernel's own cost apart from what the limits do to the robots (a robot that cannot hold itself up
            falls or folds into its joint limits: an episode's end is an auto-reset inside the launch, a joint near its bound a
            joint-limit row in the solver, off the sub-step's common path); also the episodes each env finished while timed, the
            share of its robots with a joint-limit row at the end, and the logged episodes' actuator statistics
  sensor    sensor noise (motor angle 0.01 rad, rpy 0.02 rad, rpy rate 0.1 rad/s) on top of the actuator variant with all three bindings on
            and no limits, the same set and task noise; in between the sensor variant with motor_angle_std = 0, which skips the
            sub-steps' draws: the cost of the step end's draws apart from the sub-step loop's
  randomizer the table-driven randomiser ("all_params": the built-in six ranges as a table), then the params buffer as well, on top of the
            sensor variant (all three deviations and bindings on, the same set and task noise): the cost of the table-driven reset and
            of the row's store, both outside the sub-step loop; also the episodes each env finished (auto-resets) while timed
  push      external pushes on top of the randomiser variant with everything else equal (the table "all_params", all three deviations
            and bindings on, the same set and task noise): the push variant at prob 0 with the outputs bound - the cost of the two
            settings' loads, block A, the sine / cosine and the row's store, all outside the sub-step loop - then at prob 0.02
            (lin_vel 0.2 .. 0.6, lin_vel_z 0.2, ang_vel 0.5: block B too, and what the kicks do to the robots); also the episodes each
            env finished (auto-resets) while timed and the kicks per launch
  anchor    the friction-anchor variant against the default kernel (the task's own clip, no noise)

Every env gets 300 warm-up steps of stress actions, then 5 rounds of 300 back-to-back launches with fixed actions go round the envs in
turn, so that every variant sees the same clocks; the median per env and its cost against the first env are printed.  `anchor` used to
be a script of its own that timed 500 launches once per env, one env after the other: its older single-shot figures (HISTORY.md,
profiles/r11_ab.txt) are not comparable with what this prints."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from openroborl_amd import _abi  # noqa: E402
from openroborl_amd.env import VecQuadrupedEnv  # noqa: E402

N, WARMUP, ROUNDS, LAUNCHES = 4096, 300, 5, 300
TWO_CLIPS = dict(motion_file=["laikago_pace", "laikago_trot"])
NOISE = dict(perturb_init_state_prob=0.5, tar_obs_noise=[0.1])
# case -> (kwargs of all its envs, ((name, kwargs of this env), ...)); the first env is the baseline
CASES = {
    "noise": (TWO_CLIPS, (("clip sets", {}), ("clip sets + task noise", NOISE))),
    "terms": (dict(TWO_CLIPS, **NOISE), (("task noise", {}), ("task noise + reward terms", dict(reward_terms=True)))),
    "contacts": (dict(TWO_CLIPS, **NOISE), (("task noise", {}), ("task noise + contact outputs", dict(contact_outputs=True)),
                                            ("task noise + contact outputs + reward terms", dict(contact_outputs=True, reward_terms=True)))),
    "actuator": (dict(TWO_CLIPS, contact_outputs=True, reward_terms=True, **NOISE),
                 (("task noise + contact outputs + reward terms", {}),
                  ("the same + actuator outputs, no limits", dict(actuator_outputs=True)),
                  ("the same + torque limits 20 / 30 / 40 + actuator outputs", dict(torque_limits=[20.0, 30.0, 40.0] * 4, actuator_outputs=True)))),
    "sensor": (dict(TWO_CLIPS, contact_outputs=True, reward_terms=True, actuator_outputs=True, **NOISE),
               (("task noise + contact outputs + reward terms + actuator outputs", {}),
                ("the same + sensor noise on rpy 0.02 / rpy rate 0.1 only", dict(observation_noise_stdev=[0.0, 0.0, 0.0, 0.02, 0.1])),
                ("the same + sensor noise on motor angle 0.01 / rpy 0.02 / rpy rate 0.1", dict(observation_noise_stdev=[0.01, 0.0, 0.0, 0.02, 0.1])))),
    "randomizer": (dict(TWO_CLIPS, contact_outputs=True, reward_terms=True, actuator_outputs=True, observation_noise_stdev=[0.01, 0.0, 0.0, 0.02, 0.1], **NOISE),
                   (("task noise + all three outputs + sensor noise", {}),
                    ("the same + the randomiser's table (all_params)", dict(randomizer_config="all_params")),
                    ("the same + the randomiser's table (all_params) + params buffer", dict(randomizer_config="all_params", randomizer_params=True)))),
    "push": (dict(TWO_CLIPS, contact_outputs=True, reward_terms=True, actuator_outputs=True, observation_noise_stdev=[0.01, 0.0, 0.0, 0.02, 0.1],
                  randomizer_config="all_params", **NOISE),
             (("task noise + all three outputs + sensor noise + the randomiser's table", {}),
              ("the same + push at prob 0, outputs bound", dict(push=dict(prob=0.0, lin_vel=(0.2, 0.6), lin_vel_z=0.2, ang_vel=0.5), push_outputs=True)),
              ("the same + push at prob 0.02, outputs bound", dict(push=dict(prob=0.02, lin_vel=(0.2, 0.6), lin_vel_z=0.2, ang_vel=0.5), push_outputs=True)))),
    "anchor": ({}, (("default", {}), ("friction anchors", dict(model_overrides={"laikago": {"friction_anchor": 1}})))),
}

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--case", required=True, choices=sorted(CASES))
case = ap.parse_args().case
common, variants = CASES[case]

envs, acts = [], []
for name, kw in variants:
    env = VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=N, mode="train", auto_reset=True, seed=7, **common, **kw)
    obs = env.reset()
    g = torch.Generator(device=env.device).manual_seed(0)
    act = torch.empty(N, 12, device=env.device)
    for k in range(WARMUP):
        env.stress_actions(obs, torch.randn(N, 12, device=env.device, generator=g) * 0.125, act)
        obs, r, d, _ = env.step(act)
    envs.append(env); acts.append(act)
ms = [[] for _ in variants]
finished = [-int(env.counters[_abi.CNT_EPISODES].item()) for env in envs]
for rnd in range(ROUNDS):                 # alternated: every variant sees the same clocks
    for j, env in enumerate(envs):
        ms[j].append(env.time_steps(acts[j], LAUNCHES) / LAUNCHES)
med = [sorted(m)[ROUNDS // 2] for m in ms]
for (name, _), m, mid in zip(variants, ms, med):
    print("%-44s %.4f ms per step (median of %d x %d back-to-back launches, fixed actions; all: %s)" % (
        name, mid, ROUNDS, LAUNCHES, " ".join("%.4f" % x for x in m)))
for (name, _), mid in zip(variants[1:], med[1:]):
    print("%s against %s: %+.2f %%" % (name, variants[0][0], 100.0 * (mid / med[0] - 1.0)))
if case == "contacts":
    gait = envs[1].episode_gait()
    print("gait of the logged episodes (stress actions): duty %s, mean normal force [N] %s" % (
        " ".join("%.3f" % x for x in gait.get("duty", [])), " ".join("%.1f" % x for x in gait.get("normal_force", []))))
if case == "push":
    for (name, _), env in zip(variants[1:], envs[1:]):
        print("%-76s %.1f robots kicked in the last launch" % (name, float(env.push_out[:, 6].sum().item())))
if case in ("randomizer", "push"):
    for (name, _), env, f0 in zip(variants, envs, finished):
        print("%-68s %.1f episodes ended (auto-resets) per launch while timed" % (name, (f0 + int(env.counters[_abi.CNT_EPISODES].item())) / float(ROUNDS * LAUNCHES)))
if case == "actuator":
    for (name, _), env, f0 in zip(variants, envs, finished):
        m = env.models[int(env.robot_type[0])]
        dirj, offj = np.zeros(12), np.zeros(12)
        for mot in range(12):
            dirj[int(m["joint_of_motor"][mot])], offj[int(m["joint_of_motor"][mot])] = m["motor_dir"][mot], m["motor_offset"][mot]
        a = dirj * (env.field("Q").cpu().numpy().astype(np.float64) - offj)             # the kinematic angle the bounds are given for
        room = np.minimum(a - np.asarray(m["joint_lo"]), np.asarray(m["joint_hi"]) - a) - float(env.cfg.limit_activation)
        print("%-58s %.1f episodes ended (auto-resets) per launch while timed; %.1f %% of the robots end with a joint-limit row" % (
            name, (f0 + int(env.counters[_abi.CNT_EPISODES].item())) / float(ROUNDS * LAUNCHES), 100.0 * (room < 0).any(axis=1).mean()))
    print("actuator statistics of the logged episodes (stress actions): %s" % " ".join("%s %.4g" % kv for kv in sorted(envs[2].episode_actuator_stats().items())))
for env in envs:
    env.close()
