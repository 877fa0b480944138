"""orr_shaped_reward against orr_privileged_obs, the existing kernel of its class (a launch-latency-sized gather of under 1 KB per robot),
4096 robots, same process, alternated (the protocol of tools/diag/privileged_time.py: every candidate is one captured graph of 1000
back-to-back launches, so that no host time sits between them; HIP events around a replay; medians of 5 alternated rounds after a
warm-up of 300 eager launches each):
python tools/diag/shaping_time.py
The env is the training one (train mode, randomiser) with actuator, contact and push outputs bound and all six weights non-zero, stepped
300 times first, so that the buffers hold what a rollout leaves in them."""
import sys

import torch

sys.path.insert(0, '.')
from openroborl_amd import _abi, _lib  # noqa: E402
from openroborl_amd.env import VecQuadrupedEnv  # noqa: E402

N, WARMUP, ROUNDS, LAUNCHES = 4096, 300, 5, 1000
SPEC = {"torque": 1e-5, "work": 0.05, "action_rate": 0.01, "action_accel": 0.005, "impact": 0.002, "failure": 0.7, "floor": 0.0}
dev = torch.device("cuda", 0)


def timed(graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / LAUNCHES


env = VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=N, mode="train", auto_reset=True, seed=7, contact_outputs=True,
                      push=dict(prob=0.02, lin_vel=(0.2, 0.6), lin_vel_z=0.2, ang_vel=0.5), push_outputs=True, reward_shaping=SPEC)
g = torch.Generator(device=dev).manual_seed(0)
o = env.reset()
a = torch.empty(N, 12, device=dev)
for k in range(WARMUP):
    env.stress_actions(o, torch.randn(N, 12, device=dev, generator=g) * 0.125, a)
    o, r, d, _ = env.step(a)
rows = torch.empty(N, _abi.PRIV_DIM, device=dev)
out = torch.empty(N, device=dev)


def shaped():
    _lib.check(env.L.orr_shaped_reward(env.h, a.data_ptr(), env.imitation_reward.data_ptr(), env.done.data_ptr(), out.data_ptr(), env._stream()), env.L)


names = ["orr_privileged_obs (contact + push outputs bound)", "orr_shaped_reward (six weights, actuator + contact outputs bound)"]
fns = [lambda: env.privileged_obs(out=rows, done=env.done), shaped]
graphs = []
for fn in fns:
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(LAUNCHES):
            fn()
    gr.replay()
    graphs.append(gr)
torch.cuda.synchronize()
ms = [[] for _ in fns]
for _ in range(ROUNDS):
    for j, gr in enumerate(graphs):
        ms[j].append(timed(gr))
med = [sorted(m)[ROUNDS // 2] for m in ms]
for name, m, mid in zip(names, ms, med):
    print("%-70s %.3f us (median of %d x %d back-to-back launches; all: %s)" % (name, 1e3 * mid, ROUNDS, LAUNCHES, " ".join("%.3f" % (1e3 * x) for x in m)))
print("orr_shaped_reward against orr_privileged_obs: ratio %.3f" % (med[1] / med[0]))
env.close()
