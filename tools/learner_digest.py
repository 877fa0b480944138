"""A digest of what every learner computes, to compare two checkouts bit for bit (development aid): for each learner and option set a
fixed-seed model and fixed-seed inputs, two update() calls, and a SHA-256 over the returned stats and all parameters.

usage:  python tools/learner_digest.py --device cpu                 the four torch learners (ppo.*), B = 512 / minibatch 256
        python tools/learner_digest.py --device cuda [--batch 8192 --minibatch 4096]
                                                                   the four fused learners (learner_hip.*), captured and eager
        python tools/learner_digest.py --device cuda --trace        the eager cases again, printing every orr_* entry point they call with
                                                                   its scalar (non-pointer) arguments, in order
Equal code gives equal lines; diff the output of two trees.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from openroborl_amd import ppo  # noqa: E402

HIST = dict(priv_dim=48, actor_priv_dim=48, history=16)
# (name, learner, ActorCritic's arguments, the learner's arguments, the names of update()'s tensors in its order)
CASES = [
    ("ppo-fixed-std", "PPO", {}, {}, ("obs", "act", "adv", "ret")),
    ("ppo-learn-std-kl-clip", "PPO", dict(learn_std=True), dict(ent_coef=0.01, kl_target=0.01, max_grad_norm=0.5), ("obs", "act", "adv", "ret")),
    ("ppo-privileged-obs-norm", "PPO", dict(priv_dim=48, obs_norm=True), {}, ("obs", "act", "adv", "ret")),
    ("ppo-history-latent-0", "PPOHistory", HIST, dict(latent_coef=0.0), ("obs", "hist", "priv", "act", "adv", "ret")),
    ("ppo-history-latent-0.5", "PPOHistory", HIST, dict(latent_coef=0.5), ("obs", "hist", "priv", "act", "adv", "ret")),
    ("ppo-history-learn-std", "PPOHistory", dict(HIST, learn_std=True), dict(latent_coef=0.5, ent_coef=0.01, kl_stop=0.05),
     ("obs", "hist", "priv", "act", "adv", "ret")),
    ("distill", "Distill", {}, {}, ("obs", "act")),
    ("distill-history", "DistillHistory", HIST, {}, ("hist", "priv")),
    ("distill-history-action", "DistillHistory", HIST, dict(action_coef=0.5, latent_coef=0.5), ("hist", "priv")),
]
SCALARS = (C.c_int32, C.c_int64, C.c_float, C.c_double)


class Recorder(object):
    """The loaded library with every orr_* call printed: the entry's name and its arguments that are not pointers."""

    def __init__(self, lib):
        self.lib = lib

    def __getattr__(self, name):
        f = getattr(self.lib, name)
        if not name.startswith("orr_") or all(t in SCALARS for t in f.argtypes or ()):       # a size query: no launch
            return f

        def call(*args):
            show = lambda a, t: ("NULL" if a is None else "*") if t not in SCALARS else repr(C.c_float(a).value if t is C.c_float else a)   # noqa: E731
            print("  %s(%s)" % (name, ", ".join(show(a, t) for a, t in zip(args, f.argtypes))))
            return f(*args)
        return call


def run(case, dev, B, M, use_graph, trace):
    name, kind, model_args, args, order = case
    g = torch.Generator().manual_seed(1)
    d = {k: torch.randn(B, c, generator=g).to(dev) for k, c in (("obs", 160), ("hist", 512), ("priv", 48), ("act", 12))}
    d["act"] *= 0.2
    d.update(adv=torch.randn(B, generator=g).to(dev), ret=torch.randn(B, generator=g).to(dev))
    model = ppo.ActorCritic(dev, seed=3, **model_args)
    if model_args.get("obs_norm"):
        model.update_obs_norm(d["obs"] * 2.0 + 1.0, d["priv"] * 0.5 - 1.0)       # statistics away from the identity
    more = dict(priv=d["priv"]) if (kind == "PPO" and model_args.get("priv_dim")) else {}
    if args.get("action_coef"):
        more = dict(obs=d["obs"], target_mean=d["act"])
    if dev.type == "cuda":
        from openroborl_amd import _lib, learner_hip
        if trace:
            _lib._lib = Recorder(_lib.load())
            print("%s eager" % name)
        learner = getattr(learner_hip, "Fused" + kind)(model, lr=1e-3, minibatch=M, use_graph=use_graph, **args)
    else:
        learner = getattr(ppo, kind)(model, lr=1e-3, minibatch=M, **args)
    gen = torch.Generator(device=dev).manual_seed(7)
    h = hashlib.sha256()
    for _ in range(1 if trace else 2):
        h.update(np.asarray(learner.update(*(d[k] for k in order), generator=gen, **more), dtype=np.float64).tobytes())
    for k in sorted(model.p):
        h.update(model.p[k].detach().cpu().numpy().tobytes())
    if trace:
        _lib._lib = _lib._lib.lib
    else:
        print("%-26s %-8s %s" % (name, ("graph" if use_graph else "eager") if dev.type == "cuda" else "torch", h.hexdigest()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--minibatch", type=int, default=256)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    dev = torch.device(a.device)
    if a.trace and dev.type != "cuda":
        ap.error("--trace records the fused learners: --device cuda")
    for case in CASES:
        for use_graph in ((False,) if (a.trace or dev.type != "cuda") else (True, False)):
            run(case, dev, a.batch, a.minibatch, use_graph, a.trace)


if __name__ == "__main__":
    main()
