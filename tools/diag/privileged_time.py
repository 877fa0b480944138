"""The privileged critic's two kernels against what they sit next to, 4096 robots, same process, alternated (the protocol of
tools/diag/variant_time.py: medians of 5 x 300 back-to-back launches, every candidate sees the same clocks; the 300 launches are one
captured graph, so that no host time sits between them):
python tools/diag/privileged_time.py [--alt-policy-lib PATH]

  forward   orr_policy_forward_priv, orr_policy_forward_teacher and orr_policy_forward_teacher with value = NULL (the labelling call of
            distillation: no critic) against orr_policy_forward, random weights; with --alt-policy-lib also orr_policy_forward_priv of a
            second build of csrc/orr_policy.hip (e.g. -DORR_POLICY_PRIV_SPLIT=0: the critic's layer 0 at pipeline depth 1 instead of
            12 + 1 k-groups), loaded next to the shipped library and run on the same packed weights
  history   orr_policy_forward_history (a history student: the encoder 512 -> 256 -> 48 in front of the teacher's pass) against
            orr_policy_forward_teacher, each with and without a value buffer, and orr_history_push per launch (out of place, no resets)
  row       orr_privileged_obs with contact and push outputs bound against the env step of the same env (train mode, randomiser, pushes
            at prob 0.02)"""
import argparse
import ctypes as C
import sys

import torch

sys.path.insert(0, '.')
from openroborl_amd import _abi, policy_hip, ppo  # noqa: E402
from openroborl_amd.env import VecQuadrupedEnv  # noqa: E402

N, WARMUP, ROUNDS, LAUNCHES = 4096, 300, 5, 300

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--alt-policy-lib", default="")
args = ap.parse_args()
dev = torch.device("cuda", 0)


def timed(graph):
    """ms per launch of a graph of LAUNCHES back-to-back launches (no host time between them: the row's kernel is shorter than a Python call)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / LAUNCHES


def report(names, fns):
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
        print("%-52s %.4f ms (median of %d x %d back-to-back launches; all: %s)" % (name, mid, ROUNDS, LAUNCHES, " ".join("%.4f" % x for x in m)))
    for name, mid in zip(names[1:], med[1:]):
        print("%s against %s: %+.2f %% (ratio %.4f)" % (name, names[0], 100.0 * (mid / med[0] - 1.0), mid / med[0]))
    return med


# ---- forward ----
model = ppo.ActorCritic(dev, seed=3, priv_dim=_abi.POLICY_PRIV_DIM)
plain = {k: v.detach().clone() for k, v in model.p.items()}
plain["model/vf_fc0/w:0"] = plain["model/vf_fc0/w:0"][:160].contiguous()
fp, f0 = policy_hip.FusedActorCritic(model.p, dev, std=0.125), policy_hip.FusedActorCritic(plain, dev, std=0.125)
g = torch.Generator(device=dev).manual_seed(0)
obs, priv, noise = (torch.randn(N, c, device=dev, generator=g) for c in (160, _abi.POLICY_PRIV_DIM, 12))
act, raw, val = torch.empty(N, 12, device=dev), torch.empty(N, 12, device=dev), torch.empty(N, device=dev)
teacher = ppo.ActorCritic(dev, seed=3, priv_dim=_abi.POLICY_PRIV_DIM, actor_priv_dim=_abi.POLICY_PRIV_DIM)
ft = policy_hip.FusedActorCritic(teacher.p, dev, std=0.125)
mean = torch.empty(N, 12, device=dev)
names = ["orr_policy_forward", "orr_policy_forward_priv", "orr_policy_forward_teacher", "orr_policy_forward_teacher, value = NULL"]
fns = [lambda: f0.forward(obs, noise, out_action=act, out_raw=raw, out_value=val),
       lambda: fp.forward(obs, noise, out_action=act, out_raw=raw, out_value=val, priv=priv),
       lambda: ft.forward(obs, noise, out_action=act, out_raw=raw, out_value=val, priv=priv),
       lambda: ft.forward(obs, None, out_action=act, out_raw=raw, out_mean=mean, want_value=False, priv=priv)]
if args.alt_policy_lib:
    alt = C.CDLL(args.alt_policy_lib)
    alt.orr_policy_forward_priv.restype = C.c_int32
    alt.orr_policy_forward_priv.argtypes = fp.L.orr_policy_forward_priv.argtypes
    val_alt = torch.empty(N, device=dev)

    def run_alt():
        rc = alt.orr_policy_forward_priv(C.byref(fp.net), obs.data_ptr(), priv.data_ptr(), N, noise.data_ptr(), 0.125, 6.2831853, act.data_ptr(),
                                         raw.data_ptr(), val_alt.data_ptr(), None, fp._stream())
        assert rc == 0
    names.append("orr_policy_forward_priv, --alt-policy-lib")
    fns.append(run_alt)
med = report(names, fns)
# MFMAs per wave: 1728 plain, 1824 with the critic's 13th k-group pair (+96), 1920 with the actor's too (+96); 992 without the critic
print("orr_policy_forward_teacher against orr_policy_forward_priv: %+.2f %% (the MFMA counts give %+.2f %%)" % (100.0 * (med[2] / med[1] - 1.0), 100.0 * 96 / 1824))
print("orr_policy_forward_teacher, value = NULL against orr_policy_forward_teacher: ratio %.4f (the MFMA counts give %.4f)" % (med[3] / med[2], 992.0 / 1920.0))
if args.alt_policy_lib:
    fns[1](); run_alt(); torch.cuda.synchronize()
    print("the two builds' values are equal bit for bit: %s" % bool(torch.equal(val, val_alt)))

# ---- history ----
student = ppo.ActorCritic(dev, seed=3, priv_dim=_abi.POLICY_PRIV_DIM, actor_priv_dim=_abi.POLICY_PRIV_DIM, history=_abi.HISTORY_STEPS)
fh = policy_hip.FusedActorCritic(student.p, dev, std=0.125)
hist, hist2 = torch.randn(N, _abi.HISTORY_DIM, device=dev, generator=g), torch.empty(N, _abi.HISTORY_DIM, device=dev)
done = torch.zeros(N, dtype=torch.uint8, device=dev)
med = report(["orr_policy_forward_teacher", "orr_policy_forward_teacher, value = NULL", "orr_policy_forward_history", "orr_policy_forward_history, value = NULL",
              "orr_history_push"],
             [fns[2], fns[3], lambda: fh.forward(obs, noise, out_action=act, out_raw=raw, out_value=val, hist=hist),
              lambda: fh.forward(obs, None, out_action=act, out_raw=raw, out_mean=mean, want_value=False, hist=hist),
              lambda: policy_hip.history_push(obs, done, hist, hist2)])
# MFMAs per wave: the encoder adds 512 (layer 0) + 64 (layer 1, on three of the four waves) to the teacher's 1920, or 992 without the critic
print("orr_policy_forward_history against orr_policy_forward_teacher: ratio %.4f (the MFMA counts give %.4f)" % (med[2] / med[0], (1920.0 + 576.0) / 1920.0))
print("the same with value = NULL: ratio %.4f (the MFMA counts give %.4f)" % (med[3] / med[1], (992.0 + 576.0) / 992.0))

# ---- row ----
env = VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=N, mode="train", auto_reset=True, seed=7, contact_outputs=True,
                      push=dict(prob=0.02, lin_vel=(0.2, 0.6), lin_vel_z=0.2, ang_vel=0.5), push_outputs=True)
o = env.reset()
a = torch.empty(N, 12, device=dev)
for k in range(WARMUP):
    env.stress_actions(o, torch.randn(N, 12, device=dev, generator=g) * 0.125, a)
    o, r, d, _ = env.step(a)
rows = torch.empty(N, _abi.PRIV_DIM, device=dev)
report(["env step (push variant, contact + push outputs)", "orr_privileged_obs"],
       [lambda: env.step_into(a, env.obs, env.reward, env.done), lambda: env.privileged_obs(out=rows, done=env.done)])
env.close()
