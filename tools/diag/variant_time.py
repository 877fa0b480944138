"""Step time of a variant of the step kernel against its baseline, 4096 robots, same process, alternated (train semantics):
python tools/diag/variant_time.py --case noise|terms|contacts|anchor

  noise     the task-noise variant against the clip-set variant (a two-clip set, so that the plain env runs the clip-set variant)
  terms     reward terms on top of task noise               (two-clip set, noise on in all at one setting: prob 0.5, sigma 0.1)
  contacts  contact outputs, then reward terms as well, on top of task noise (the same set and noise); also the logged episodes' gait
  anchor    the friction-anchor variant against the default kernel (the task's own clip, no noise)

Every env gets 300 warm-up steps of stress actions, then 5 rounds of 300 back-to-back launches with fixed actions go round the envs in
turn, so that every variant sees the same clocks; the median per env and its cost against the first env are printed.  `anchor` used to
be a script of its own that timed 500 launches once per env, one env after the other: its older single-shot figures (HISTORY.md,
profiles/r11_ab.txt) are not comparable with what this prints."""
import argparse
import sys

import torch

sys.path.insert(0, '.')
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
for env in envs:
    env.close()
