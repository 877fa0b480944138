"""The update controls without a GPU: the C-ABI's exports, record size and refusals (include/openroborl_learner.h: orr_update_ctl,
orr_update_control, orr_adam_step_ctl), the torch yardsticks' arithmetic (ppo._UpdateControl) against float64 and against a host
restatement of the rules, and train.py's flags."""
import argparse
import ctypes as C
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_control_entry_points_and_the_record_size():
    from openroborl_amd import _abi, _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "openroborl_learner.h")).read()
    for name in ("orr_update_control", "orr_adam_step_ctl", "orr_update_control_partials", "orr_sizeof_update_ctl"):
        assert hasattr(L, name) and name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr), name
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert L.orr_sizeof_update_ctl() == C.sizeof(_abi.OrrUpdateCtl) == 4 * len(_abi.UPDATE_CTL_WORDS) == 48
    # every word of the struct is declared in the header, in the ctypes order
    body = hdr[hdr.index("typedef struct orr_update_ctl"):hdr.index("orr_update_ctl;")]
    assert tuple(re.findall(r"^\s*(?:float|int32_t)\s+(\w+);", body, re.M)) == _abi.UPDATE_CTL_WORDS
    assert int(re.search(r"#define ORR_UPDATE_CONTROL_BLOCK_FLOATS (\d+)", hdr).group(1)) == _abi.UPDATE_CONTROL_BLOCK_FLOATS
    blk = _abi.UPDATE_CONTROL_BLOCK_FLOATS
    assert [L.orr_update_control_partials(n) for n in (0, -5, 1, blk, blk + 1, 434701)] == [-1, -1, 1, 1, 2, (434701 + blk - 1) // blk]


def test_refusals_launch_nothing():
    """Every refusal of the two entry points returns a negative code with text; none of these paths reaches a launch (the test runs
    without a GPU, where a launch would be a different error)."""
    from openroborl_amd import _lib
    L = _lib.load()
    ok, odd = 0x10000, 0x10004            # never dereferenced: the checks come first

    def control(g=ok, n=8, kl=None, kl_stop=0.0, kl_target=0.0, lo=0.5, hi=2.0, partials=ok, ctl=ok):
        return L.orr_update_control(g, n, 1.0, 0.5, kl, kl_stop, kl_target, lo, hi, partials, ctl, None)

    cases = {"null g": dict(g=None), "null partials": dict(partials=None), "null ctl": dict(ctl=None), "misaligned g": dict(g=odd),
             "misaligned ctl": dict(ctl=odd), "misaligned partials": dict(partials=0x10002), "misaligned kl": dict(kl=0x10001, kl_stop=0.1),
             "n = 0": dict(n=0), "n < 0": dict(n=-4), "lo > hi": dict(lo=2.0, hi=1.0), "NaN bound": dict(lo=float("nan")),
             "kl_stop without kl": dict(kl_stop=0.1), "kl_target without kl": dict(kl_target=0.01)}
    for what, kw in cases.items():
        rc = control(**kw)
        assert rc < 0 and b"orr_update_control" in L.orr_last_error(), (what, rc, L.orr_last_error())

    def adam(p=ok, g=ok, m=ok, v=ok, n=8, flags=0, state=ok, ctl=ok):
        return L.orr_adam_step_ctl(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-5, 1.0, flags, state, ctl, None)

    cases = {"null p": dict(p=None), "null g": dict(g=None), "null m": dict(m=None), "null v": dict(v=None), "null state": dict(state=None),
             "null ctl": dict(ctl=None), "n = 0": dict(n=0), "unknown flag": dict(flags=2), "misaligned p": dict(p=odd),
             "misaligned g": dict(g=odd), "misaligned m": dict(m=odd), "misaligned v": dict(v=odd), "misaligned ctl": dict(ctl=odd)}
    for what, kw in cases.items():
        rc = adam(**kw)
        assert rc < 0 and b"orr_adam_step_ctl" in L.orr_last_error(), (what, rc, L.orr_last_error())


# ---- the torch yardsticks on the CPU ---------------------------------------------------------------------------------------------------

def _loss64(p, obs, act, adv, ret, old_logp, clip=0.2, std=0.125):
    import torch

    def mlp(net):
        h = torch.relu(obs @ p["model/%s_fc0/w:0" % net] + p["model/%s_fc0/b:0" % net])
        h = torch.relu(h @ p["model/%s_fc1/w:0" % net] + p["model/%s_fc1/b:0" % net])
        return h @ p["model/%s/w:0" % net] + p["model/%s/b:0" % net]
    var = std * std
    logp = (-0.5 * ((act - mlp("pi")) ** 2) / var - 0.5 * math.log(2.0 * math.pi * var)).sum(dim=1)
    ratio = torch.exp(logp - old_logp)
    surr = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv).mean()
    vf = ((mlp("vf")[:, 0] - ret) ** 2).mean()
    return surr + vf


def _batch(model, B, seed=0, shift=0.04):
    import torch
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(B, 160, generator=g)
    with torch.no_grad():
        mu = model.mean(obs)
    act = mu + 0.125 * torch.randn(B, 12, generator=g)
    old = (-0.5 * ((act - (mu + shift * torch.randn(B, 12, generator=g))) ** 2) / 0.125 ** 2 - 0.5 * math.log(2.0 * math.pi * 0.125 ** 2)).sum(dim=1)
    return obs, act, torch.randn(B, generator=g), torch.randn(B, generator=g), old


def test_clipped_update_matches_float64():
    """One update of one minibatch through ppo.PPO(max_grad_norm) against float64: loss and autograd, the clip formula, the first Adam step
    (m_hat = g, v_hat = g^2 at t = 1).  The bounds are test_one_ppo_update_matches_float64_cpu's."""
    import torch
    from openroborl_amd import ppo
    B, lr = 2048, 1e-4
    model = ppo.ActorCritic("cpu", seed=4)
    obs, act, adv, ret, old = _batch(model, B)
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in model.p.items()}
    _loss64(p64, obs.double(), act.double(), adv.double(), ret.double(), old.double()).backward()
    norm64 = math.sqrt(sum(float((v.grad ** 2).sum()) for v in p64.values()))
    for c, clips in ((0.5 * norm64, True), (2.0 * norm64, False)):
        m = ppo.ActorCritic("cpu", seed=4)
        before = {k: v.detach().clone() for k, v in m.p.items()}
        learner = ppo.PPO(m, lr=lr, adam_eps=1e-5, minibatch=B, max_grad_norm=c)
        learner.update(obs, act, adv, ret, old_logp=old, epochs=1, generator=torch.Generator().manual_seed(1))
        st = learner.control_stats()
        assert abs(st["grad_norm"] - norm64) < 2e-3 * norm64 and st["clipped"] == int(clips) and st["calls"] == 1
        scale64 = min(1.0, c / (norm64 + 1e-6))
        assert (scale64 < 1.0) == clips
        for k in sorted(m.p):
            g64 = scale64 * p64[k].grad
            step64 = -lr * g64 / (g64.abs() + 1e-5)
            step = (m.p[k].detach() - before[k]).double()
            big = g64.abs() > 1e-3                                   # away from the eps-dominated region
            assert big.any()
            assert (step - step64)[big].abs().max().item() < 2e-6, k
            assert step.abs().max().item() <= lr * (1 + 1e-3)


def _snapshots(model):
    """Clones of the parameters after every minibatch: the learners call model.mark_updated() there."""
    import torch
    snaps, orig = [], model.mark_updated

    def hook():
        orig()
        snaps.append(torch.cat([model.p[k].detach().reshape(-1) for k in sorted(model.p)]).clone())
    model.mark_updated = hook
    return snaps


def test_a_non_finite_minibatch_is_skipped_not_taken():
    import torch
    from openroborl_amd import ppo
    B, M = 1024, 256
    model = ppo.ActorCritic("cpu", seed=4)
    obs, act, adv, ret, old = _batch(model, B)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))
    adv[perm[2 * M]] = float("nan")                  # one row of the third minibatch
    learner = ppo.PPO(model, lr=1e-4, minibatch=M, max_grad_norm=1e9)
    snaps = _snapshots(model)
    learner.update(obs, act, adv, ret, old_logp=old, epochs=1, generator=torch.Generator().manual_seed(3))
    assert len(snaps) == 4
    assert torch.equal(snaps[1], snaps[2])           # bit-identical across the planted minibatch
    assert not torch.equal(snaps[0], snaps[1]) and not torch.equal(snaps[2], snaps[3]) and bool(torch.isfinite(snaps[3]).all())
    steps = {int(s["step"]) for s in learner.opt.state.values()}
    assert steps == {3}                              # the optimiser's step count did not advance
    st = learner.control_stats()
    assert st["skipped_nonfinite"] == 1 and st["calls"] == 3 and math.isfinite(st["grad_norm_max"])
    assert learner.control_stats()["skipped_nonfinite"] == 0        # reading clears the counters


def test_kl_stop_ends_an_update_and_the_next_one_steps_again():
    import torch
    from openroborl_amd import ppo
    B, M = 1024, 256
    model = ppo.ActorCritic("cpu", seed=4)
    obs, act, adv, ret, _ = _batch(model, B)
    with torch.no_grad():
        old = model.log_prob(obs, act)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))
    old = old.clone()
    old[perm[2 * M:]] += 0.5                         # the last two minibatches' old log-probabilities: their KL is e^-0.5 - 1 + 0.5 = 0.107
    learner = ppo.PPO(model, lr=1e-5, minibatch=M, kl_stop=0.05)
    snaps = _snapshots(model)
    out = learner.update(obs, act, adv, ret, old_logp=old, epochs=1, generator=torch.Generator().manual_seed(3))
    assert len(out) == 2                             # a fixed-std model still returns its two stats
    kls = learner.kls
    assert max(kls[:2]) < 0.05 * 0.95 and min(kls[2:]) > 0.05 * 1.05, kls
    assert not torch.equal(snaps[0], snaps[1]) and torch.equal(snaps[1], snaps[2]) and torch.equal(snaps[2], snaps[3])
    assert {int(s["step"]) for s in learner.opt.state.values()} == {2}
    st = learner.control_stats()
    assert st["skipped_kl"] == 2 and st["calls"] == 4 and st["skipped_nonfinite"] == 0
    # the stop holds for one update(): the next one (its KL is ~0: old_logp is the current policy's) takes all four steps
    learner.update(obs, act, adv, ret, old_logp=None, epochs=1, generator=torch.Generator().manual_seed(4))
    assert {int(s["step"]) for s in learner.opt.state.values()} == {6} and learner.control_stats()["skipped_kl"] == 0


def kl_rule(mult, kl, target, lo, hi):
    """The host restatement of the KL-adaptive rule in float32 (orr_update_control, kl_target > 0)."""
    f = np.float32
    mult, kl, target = f(mult), f(kl), f(target)
    if kl > f(2.0) * target:
        return float(max(f(lo), mult / f(1.5)))
    if f(0.0) < kl < f(0.5) * target:
        return float(min(f(hi), mult * f(1.5)))
    return float(mult)


def test_kl_target_multiplies_and_clamps():
    import torch
    from openroborl_amd import ppo
    model = ppo.ActorCritic("cpu", seed=4)
    t, lo, hi, lr = 0.01, 0.4, 2.0, 1e-4
    learner = ppo.PPO(model, lr=lr, minibatch=64, kl_target=t, kl_lr_bounds=(lo, hi))
    for p in model.parameters():
        p.grad = torch.full_like(p, 1e-3)
    seq = [0.0, 0.4 * t, 0.4 * t, 0.4 * t, 0.6 * t, 1.9 * t, 2.1 * t, 2.1 * t, 2.1 * t, 2.1 * t, 2.1 * t, float("nan"), 0.4 * t]
    want, mults, taken = 1.0, [], 0
    for kl in seq:
        stepped = learner._step(torch.tensor(kl))
        if math.isfinite(kl):
            want = kl_rule(want, kl, t, lo, hi)
        assert stepped == math.isfinite(kl)
        taken += int(stepped)
        mults.append(learner.kl_lr_mult)
        assert learner.kl_lr_mult == want
        if stepped:
            assert learner.opt.param_groups[0]["lr"] == float(np.float32(lr) * np.float32(1.0) * np.float32(want))
    assert max(mults) == hi and min(mults) == np.float32(lo) and mults[0] == 1.0 and mults[4] == mults[5] == hi       # both clamps, and the dead band
    assert {int(s["step"]) for s in learner.opt.state.values()} == {taken} and learner.control_stats()["skipped_nonfinite"] == 1


def test_lr_multiplier_and_distill_learners():
    """set_lr_mult goes through the optimiser's param group; with 0 the parameters stand while the moments move and the step counts - that
    is what tells the multiplier from a skip.  Distill and DistillHistory take max_grad_norm and set_lr_mult."""
    import torch
    from openroborl_amd import ppo
    model = ppo.ActorCritic("cpu", seed=4)
    obs, act, adv, ret, old = _batch(model, 256)
    learner = ppo.PPO(model, lr=1e-4, minibatch=256)
    before = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()
    learner.set_lr_mult(0.0)
    learner.update(obs, act, adv, ret, old_logp=old)
    assert torch.equal(before, torch.cat([p.detach().reshape(-1) for p in model.parameters()]))
    state = list(learner.opt.state.values())
    assert all(int(s["step"]) == 1 for s in state) and any(float(s["exp_avg"].abs().max()) > 0 for s in state)
    learner.set_lr_mult(0.5)
    learner.update(obs, act, adv, ret, old_logp=old)
    assert learner.opt.param_groups[0]["lr"] == float(np.float32(1e-4) * np.float32(0.5))
    student = ppo.ActorCritic("cpu", seed=5)
    d = ppo.Distill(student, lr=1e-3, minibatch=128, max_grad_norm=1e-6)
    d.set_lr_mult(0.25)
    d.update(obs, torch.ones(256, 12))
    st = d.control_stats()
    assert st["clipped"] == 2 and st["lr_mult"] == 0.25 and d.opt.param_groups[0]["lr"] == float(np.float32(1e-3) * np.float32(0.25))
    hs = ppo.ActorCritic("cpu", seed=5, priv_dim=48, actor_priv_dim=48, history=16)
    dh = ppo.DistillHistory(hs, lr=1e-3, minibatch=128, max_grad_norm=1e-3)
    dh.update(torch.randn(256, 512), torch.randn(256, 48))
    assert dh.control_stats()["clipped"] == 2


def test_bad_control_arguments_are_refused():
    import pytest
    from openroborl_amd import ppo
    model = ppo.ActorCritic("cpu", seed=4)
    for kw in (dict(max_grad_norm=0.0), dict(max_grad_norm=float("nan")), dict(kl_stop=-1.0), dict(kl_target=float("inf")),
               dict(kl_target=0.01, kl_lr_bounds=(2.0, 1.0)), dict(kl_target=0.01, kl_lr_bounds=(0.0, 1.0))):
        with pytest.raises(ValueError):
            ppo.PPO(model, **kw)


# ---- train.py -----------------------------------------------------------------------------------------------------------------------------

def _train():
    sys.path.insert(0, ROOT)
    import train
    return train


def test_train_flags_and_the_linear_schedule():
    import pytest
    train = _train()
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--torch-learner", action="store_true")
    train.control_args(ap)
    args = ap.parse_args([])
    assert train.control_kwargs(args) == {} and not train.control_on(args) and train.lr_mult(args, 7) == 1.0
    args = ap.parse_args("--iters 4 --max-grad-norm 0.5 --lr-schedule linear --kl-stop 0.05 --kl-target 0.01 --kl-lr-bounds 0.1 4".split())
    assert train.control_on(args)
    assert train.control_kwargs(args) == {"max_grad_norm": 0.5, "kl_stop": 0.05, "kl_target": 0.01, "kl_lr_bounds": (0.1, 4.0), "device_lr": True}
    assert [train.lr_mult(args, it) for it in range(5)] == [1.0, 0.75, 0.5, 0.25, 0.0]
    args = ap.parse_args("--iters 3 --lr-schedule linear --torch-learner".split())
    assert train.control_kwargs(args) == {}                      # the torch learners need no switch for set_lr_mult
    assert [train.lr_mult(args, it) for it in range(3)] == [1.0, 1.0 - 1.0 / 3.0, 1.0 - 2.0 / 3.0]
    with pytest.raises(SystemExit):
        train.control_kwargs(ap.parse_args(["--kl-stop", "0.1"]), kl=False)
    with pytest.raises(SystemExit):
        train.control_kwargs(ap.parse_args(["--kl-lr-bounds", "0.1", "2"]))
    with pytest.raises(SystemExit):
        ap.parse_args(["--lr-schedule", "cosine"])
    src = open(os.path.join(ROOT, "train.py")).read()
    assert src.count("control_kwargs(args") == 7 and src.count("learner.set_lr_mult(lr_mult(args, it))") == 3     # all six learners, all three loops
