"""Step time of the reward-terms variant of the step kernel against the task-noise variant's, 4096 robots, same process, alternated
(train semantics, a two-clip set, noise on in both at the same setting: prob 0.5, sigma 0.1): python tools/diag/terms_time.py"""
import sys, torch
sys.path.insert(0, '.')
from openroborl_amd.env import VecQuadrupedEnv
CASES = (("task noise", {}), ("task noise + reward terms", dict(reward_terms=True)))
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
ms = [[], []]
for rnd in range(5):                      # alternated: both variants see the same clocks
    for j, env in enumerate(envs):
        ms[j].append(env.time_steps(acts[j], 300) / 300)
for (name, _), m in zip(CASES, ms):
    print("%-26s %.4f ms per step (median of 5 x 300 back-to-back launches, fixed actions; all: %s)" % (name, sorted(m)[2], " ".join("%.4f" % x for x in m)))
print("reward terms cost %+.2f %%" % (100.0 * (sorted(ms[1])[2] / sorted(ms[0])[2] - 1.0)))
for env in envs:
    env.close()
