"""Step time of the contact-output variant of the step kernel against the task-noise variant's, 4096 robots, same process, alternated
(train semantics, a two-clip set, noise on in both at the same setting: prob 0.5, sigma 0.1): python tools/diag/contacts_time.py"""
import sys, torch
sys.path.insert(0, '.')
from openroborl_amd.env import VecQuadrupedEnv
CASES = (("task noise", {}), ("task noise + contact outputs", dict(contact_outputs=True)),
         ("task noise + contact outputs + reward terms", dict(contact_outputs=True, reward_terms=True)))
envs, acts = [], []
for name, kw in CASES:
    env = VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=4096, mode="train", auto_reset=True, seed=7,
                          motion_file=["laikago_pace", "laikago_trot"], perturb_init_state_prob=0.5, tar_obs_noise=[0.1], **kw)
    obs = env.reset()
    g = torch.Generator(device=env.device).manual_seed(0)
    act = torch.empty(4096, 12, device=env.device)
    for k in range(300):
        env.stress_actions(obs, torch.randn(4096, 12, device=env.device, generator=g) * 0.125, act)
        obs, r, d, _ = env.step(act)
    envs.append(env); acts.append(act)
ms = [[] for _ in CASES]
for rnd in range(5):                      # alternated: every variant sees the same clocks
    for j, env in enumerate(envs):
        ms[j].append(env.time_steps(acts[j], 300) / 300)
for (name, _), m in zip(CASES, ms):
    print("%-44s %.4f ms per step (median of 5 x 300 back-to-back launches, fixed actions; all: %s)" % (name, sorted(m)[2], " ".join("%.4f" % x for x in m)))
for j in (1, 2):
    print("%s cost %+.2f %%" % (CASES[j][0][13:], 100.0 * (sorted(ms[j])[2] / sorted(ms[0])[2] - 1.0)))
gait = envs[1].episode_gait()
print("gait of the logged episodes (stress actions): duty %s, mean normal force [N] %s" % (
    " ".join("%.3f" % x for x in gait.get("duty", [])), " ".join("%.1f" % x for x in gait.get("normal_force", []))))
for env in envs:
    env.close()
