"""PPO on a history policy without a GPU: the declarations and host-side refusals of orr_policy_forward_history_priv and orr_latent_backward,
ppo.PPOHistory against a float64 computation of the stated loss written out here, ActorCritic.act(critic_priv=), the refusals that stay, and
train.py's argument refusals in child processes.

Tolerances: the gradients' are tests/test_gpu_teacher.py's for FusedPPO (2e-3 of the gradient's scale, cosine above 0.99999)."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from openroborl_amd import _abi, _lib, ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 48
ENC = ("model/enc_fc0/w:0", "model/enc_fc0/b:0", "model/enc_fc1/w:0", "model/enc_fc1/b:0")


def _policy(seed, learn_std=True, gain=30.0):
    """A history policy with random biases and actor outputs of O(1) (tests/test_history_cpu.py's student), its log-stds apart"""
    m = ppo.ActorCritic("cpu", seed=seed, priv_dim=48, actor_priv_dim=48, history=16, learn_std=learn_std)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for k, v in m.p.items():
            if k.endswith("/b:0"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
        m.p["model/pi/w:0"].mul_(gain)
        if learn_std:
            m.p[ppo.LOGSTD].add_(0.2 * torch.randn(1, 12, generator=g))
    return m


def _batch(model, seed=4):
    """obs, hist, priv, actions, old log-probabilities (of a shifted mean: ratios on both sides of the clip), advantages, returns"""
    g = torch.Generator().manual_seed(seed)
    obs, hist, priv = torch.randn(B, 160, generator=g), torch.randn(B, 512, generator=g), torch.randn(B, 48, generator=g)
    with torch.no_grad():
        mu = model.mean(obs, hist=hist)
        std = model.p[ppo.LOGSTD].exp() if model.learn_std else 0.125
        act = mu + std * torch.randn(B, 12, generator=g)
        old = model.log_prob(obs, act + 0.04 * torch.randn(B, 12, generator=g), hist=hist)
    adv = torch.randn(B, generator=g)
    adv[::7] = 0.0
    return obs, hist, priv, act, old, adv, torch.randn(B, generator=g)


def _terms64(p, obs, hist, priv, act, old, adv, ret, clip=0.2):
    """The stated loss's terms in float64, written out: z = relu(hist W0 + b0) W1 + b1; the actor on obs | z, the critic on obs | priv"""
    obs, hist, priv, act, old, adv, ret = (x.double() for x in (obs, hist, priv, act, old, adv, ret))
    z = torch.relu(hist @ p["model/enc_fc0/w:0"] + p["model/enc_fc0/b:0"]) @ p["model/enc_fc1/w:0"] + p["model/enc_fc1/b:0"]

    def mlp(net, x):
        h = torch.relu(x @ p["model/%s_fc0/w:0" % net] + p["model/%s_fc0/b:0" % net])
        h = torch.relu(h @ p["model/%s_fc1/w:0" % net] + p["model/%s_fc1/b:0" % net])
        return h @ p["model/%s/w:0" % net] + p["model/%s/b:0" % net]
    mu, v = mlp("pi", torch.cat((obs, z), dim=1)), mlp("vf", torch.cat((obs, priv), dim=1))[:, 0]
    ls = p[ppo.LOGSTD]
    logp = (-0.5 * ((act - mu) * torch.exp(-ls)) ** 2 - ls - 0.5 * math.log(2.0 * math.pi)).sum(dim=1)
    ratio = torch.exp(logp - old)
    surr = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv).mean()
    return surr, ((v - ret) ** 2).mean(), ls.sum() + ppo.ENTROPY_CONST, ((z - priv) ** 2).sum(dim=1).mean()


def _close(model, want, names):
    for k in names:
        g32, g64 = model.p[k].grad.detach().double(), want[k]
        scale = g64.abs().max().item() + 1e-12
        cs = ((g32 * g64).sum() / (g32.norm() * g64.norm() + 1e-30)).item()
        print("%s: gradient error %.2e of its scale, 1 - cosine %.2e" % (k, (g32 - g64).abs().max().item() / scale, 1.0 - cs))
        assert (g32 - g64).abs().max().item() < 2e-3 * scale, k
        assert cs > 0.99999, k


@pytest.mark.parametrize("latent_coef", [0.0, 0.5])
def test_ppo_history_matches_float64_autograd_of_the_stated_loss(latent_coef):
    """One minibatch at lr = 0 (the parameters stand still): the stats and the gradients of every tensor - actor, critic, encoder, log-std."""
    model = _policy(2)
    data = _batch(model)
    names = sorted(model.p)
    assert len(names) == 17 and all(k in names for k in ENC) and ppo.LOGSTD in names       # 6 + 6 + 4 and the log-std
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in model.p.items()}
    surr, vf, ent, lat = _terms64(p64, *data)
    vf_coef, ent_coef = 0.7, 0.01
    grads = torch.autograd.grad(surr + vf_coef * vf - ent_coef * ent + latent_coef * lat, [p64[k] for k in names], retain_graph=True)
    want = dict(zip(names, grads))
    learner = ppo.PPOHistory(model, lr=0.0, minibatch=B, vf_coef=vf_coef, ent_coef=ent_coef, latent_coef=latent_coef)
    obs, hist, priv, act, old, adv, ret = data
    stats = learner.update(obs, hist, priv, act, adv, ret, old_logp=old, generator=torch.Generator().manual_seed(0))
    assert len(stats) == 6                                             # ppo.STAT_NAMES' five and the latent loss, whatever its coefficient
    for got, ref in ((stats[0], surr), (stats[1], vf), (stats[2], ent), (stats[5], lat)):
        assert abs(float(got) - ref.item()) < 2e-4 * max(1.0, abs(ref.item())), (float(got), ref.item())
    assert lat.item() > 1.0 and 0.0 < float(stats[4]) < 1.0           # some ratios are clipped, some are not
    _close(model, want, names)
    # the encoder's gradient through the actor alone: what latent_coef = 0 leaves, and not what 0.5 leaves
    alone = dict(zip(ENC, torch.autograd.grad(surr, [p64[k] for k in ENC])))
    assert all(float(alone[k].abs().max()) > 0.0 for k in ENC)
    if latent_coef == 0.0:
        _close(model, alone, ENC)
    else:
        assert float((model.p[ENC[3]].grad.double() - alone[ENC[3]]).abs().max()) > 1e-2 * float(alone[ENC[3]].abs().max())


def test_a_fixed_std_model_returns_three_stats_and_everything_moves():
    model = _policy(3, learn_std=False)
    obs, hist, priv, act, old, adv, ret = _batch(model)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    lr = 1e-3
    learner = ppo.PPOHistory(model, lr=lr, minibatch=16, latent_coef=0.0)
    stats = learner.update(obs, hist, priv, act, adv, ret, epochs=2, generator=torch.Generator().manual_seed(1))       # no old_logp: computed with hist
    assert len(stats) == 3 and all(math.isfinite(float(s)) for s in stats) and float(stats[2]) > 1.0
    for k in before:                                                   # actor, critic and - through the actor alone - the encoder
        moved = float((model.p[k].detach() - before[k]).abs().max())  # (Adam's first steps are about lr each; a lone bias may go back and forth)
        assert moved > (0.5 * lr if k in ENC else 0.0), (k, moved)
    assert getattr(model, "updates", 0) == 2 * 3


def test_ppo_history_refusals():
    plain, teacher = ppo.ActorCritic("cpu", seed=1), ppo.ActorCritic("cpu", seed=1, priv_dim=48, actor_priv_dim=48)
    for m in (plain, teacher):
        with pytest.raises(ValueError, match="history encoder"):
            ppo.PPOHistory(m)
    model = _policy(1)
    for kw in (dict(latent_coef=-0.5), dict(latent_coef=float("nan"))):
        with pytest.raises(ValueError, match="latent_coef"):
            ppo.PPOHistory(model, **kw)
    with pytest.raises(ValueError, match="ent_coef"):
        ppo.PPOHistory(_policy(1, learn_std=False), ent_coef=0.01)
    obs, hist, priv, act, old, adv, ret = _batch(model)
    learner = ppo.PPOHistory(model, minibatch=16)
    for bad in (lambda: learner.update(obs, hist[:, :500], priv, act, adv, ret), lambda: learner.update(obs, hist, priv[:, :47], act, adv, ret),
                lambda: learner.update(obs, hist[:B - 1], priv, act, adv, ret)):
        with pytest.raises(ValueError):
            bad()
    for v in model.p.values():
        assert v.grad is None                                          # a refused update computes nothing


def test_act_with_critic_priv_and_the_refusals_that_stay():
    model = _policy(5)
    obs, hist, priv, _, _, _, _ = _batch(model)
    noise = torch.randn(B, 12, generator=torch.Generator().manual_seed(9))
    latent = torch.empty(B, 48)
    a, raw, v = model.act(obs, hist=hist, critic_priv=priv, noise=noise, out_latent=latent)
    with torch.no_grad():
        mu, z = model.mean(obs, hist=hist), model.encode(hist)
        assert torch.equal(raw, mu + model.log_std.exp() * noise) and torch.equal(a, raw.clamp(-2.0 * math.pi, 2.0 * math.pi))
        assert torch.equal(v, model.value(obs, priv)) and torch.equal(latent, z)
        a0, raw0, v0 = model.act(obs, hist=hist, noise=noise)          # without: the estimate feeds the critic too
        assert torch.equal(raw0, raw) and torch.equal(v0, model.value(obs, z)) and float((v0 - v).abs().max()) > 1e-3
        assert torch.equal(model.log_prob(obs, raw, hist=hist), model.log_prob(obs, raw, priv=z))
    for bad in (lambda: model.act(obs, critic_priv=priv), lambda: model.act(obs, priv, critic_priv=priv), lambda: model.act(obs, hist=hist, critic_priv=priv[:, :47]),
                lambda: model.act(obs, hist=hist, critic_priv=priv[:B - 1]), lambda: model.act(obs, priv, hist=hist), lambda: model.mean(obs, priv, hist=hist),
                lambda: ppo.ActorCritic("cpu", seed=1, priv_dim=48, actor_priv_dim=48).act(obs, hist=hist, critic_priv=priv)):
        with pytest.raises(ValueError):
            bad()
    # what a history policy is refused by stays refused, and says where to go
    with pytest.raises(ValueError, match="PPOHistory"):
        ppo.PPO(model)
    with pytest.raises(ValueError, match="history"):
        ppo.Distill(model)


def test_the_entry_points_are_declared_and_refuse_on_the_host():
    policy_h = open(os.path.join(ROOT, "include", "openroborl_policy.h")).read()
    learner_h = open(os.path.join(ROOT, "include", "openroborl_learner.h")).read()
    assert re.search(r"int32_t orr_policy_forward_history_priv\(const orr_policy_net\* net, const orr_history_encoder\* enc, const float\* obs, "
                     r"const float\* hist,\s+const float\* priv, int32_t n, const float\* noise, float std, float clip, float\* action, float\* raw,\s+"
                     r"float\* value, float\* mean, float\* latent, void\* stream\);", policy_h)
    assert re.search(r"int32_t orr_latent_backward\(const float\* g0, const float\* w0zt, const float\* z, const float\* target_priv, int32_t m, "
                     r"float latent_coef,\s+float\* g_z, float\* partials, void\* stream\);", learner_h)
    assert re.search(r"#define ORR_LATENT_BACKWARD_ROWS\(m\) \(\(\(m\) \+ 15\) / 16\)", learner_h)
    assert re.search(r"#define ORR_LATENT_BACKWARD_PARTIAL_FLOATS\(m\) \(49 \* \(int64_t\)ORR_LATENT_BACKWARD_ROWS\(m\)\)", learner_h)
    assert re.search(r"#define ORR_COLSUM_MAX_JOBS 12\b", learner_h)                      # the constant stays: two launches instead
    for name in ("orr_policy_forward_history_priv", "orr_latent_backward"):
        assert name in _lib.EXPORTS
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert len(_abi.POLICY_FORWARD_HISTORY_PRIV_ARGS) == 15 and len(_abi.LATENT_BACKWARD_ARGS) == 9
    assert [_abi.latent_backward_rows(m) for m in (1, 15, 16, 17, 33, 16384)] == [1, 1, 1, 2, 3, 1024]
    L = _lib.load()
    assert L.orr_policy_forward_history_priv.argtypes == _abi.POLICY_FORWARD_HISTORY_PRIV_ARGS
    assert L.orr_latent_backward.argtypes == _abi.LATENT_BACKWARD_ARGS
    err = lambda: L.orr_last_error()   # noqa: E731
    # host-side refusals (no launch happens on these paths; the "pointers" are never read)
    net, enc = _abi.OrrPolicyNet(), _abi.OrrHistoryEncoder()
    for s, n in ((net, 12), (enc, 4)):
        for f, _ in s._fields_[:n]:
            setattr(s, f, 64)
    good = dict(net=net, enc=enc, obs=64, hist=64, priv=64, n=4, noise=64, action=64, raw=64, value=64, mean=64, latent=64)

    def fwd(**kw):
        a = dict(good, **kw)
        return L.orr_policy_forward_history_priv(a["net"], a["enc"], a["obs"], a["hist"], a["priv"], a["n"], a["noise"], 0.125, 6.0, a["action"], a["raw"],
                                                 a["value"], a["mean"], a["latent"], None)
    name = b"orr_policy_forward_history_priv"
    for kw in (dict(net=None), dict(enc=None), dict(obs=None), dict(hist=None), dict(action=None), dict(n=0), dict(n=-5), dict(priv=None)):
        assert fwd(**kw) == -1 and name + b": bad argument" in err(), kw               # priv = NULL with a value buffer among them
    for s, fields in ((net, [f for f, _ in net._fields_]), (enc, [f for f, _ in enc._fields_])):
        for f in fields:
            setattr(s, f, None)
            assert fwd() == -1 and name in err() and b"null pointer" in err(), f
            setattr(s, f, 64 + (4 if f.startswith("w") else 2))
            assert fwd() == -1 and name in err() and b"aligned" in err(), f
            setattr(s, f, 64)
    assert fwd(hist=64 + 4) == -1 and name + b": hist must be 16-byte aligned" in err()
    for kw in (dict(obs=64 + 2), dict(priv=64 + 2), dict(noise=64 + 1), dict(action=64 + 3), dict(raw=64 + 2), dict(value=64 + 1), dict(mean=64 + 2),
               dict(latent=64 + 2)):
        assert fwd(**kw) == -1 and name in err() and b"4-byte aligned" in err(), kw

    good = dict(g0=64, w0zt=64, z=64, tp=64, m=4, coef=0.5, g_z=64, partials=64)

    def lat(**kw):
        a = dict(good, **kw)
        return L.orr_latent_backward(a["g0"], a["w0zt"], a["z"], a["tp"], a["m"], a["coef"], a["g_z"], a["partials"], None)
    name = b"orr_latent_backward"
    for kw in (dict(g0=None), dict(w0zt=None), dict(g_z=None), dict(partials=None), dict(m=0), dict(m=-5), dict(z=None), dict(tp=None)):
        assert lat(**kw) == -1 and name + b": bad argument" in err(), kw               # z / target_priv = NULL with a coefficient among them
    for kw in (dict(w0zt=64 + 4), dict(w0zt=64 + 8)):
        assert lat(**kw) == -1 and name in err() and b"16-byte aligned" in err(), kw
    for kw in (dict(g0=64 + 2), dict(z=64 + 1), dict(tp=64 + 3), dict(g_z=64 + 2), dict(partials=64 + 2), dict(z=64 + 2, coef=0.0)):
        assert lat(**kw) == -1 and name in err() and b"4-byte aligned" in err(), kw


@pytest.mark.parametrize("argv,text", [
    (["--latent-coef", "0.5"], "--latent-coef belongs to --history-ppo"),
    (["--history-ppo", "--latent-coef", "-0.5"], "--latent-coef must not be negative"),
    (["--history-ppo", "--distill", "teacher.zip"], "--history-ppo is a mode of its own"),
    (["--history-ppo", "--history"], "--history-ppo is a mode of its own"),
    (["--history-ppo", "--privileged-critic"], "--history-ppo is a mode of its own"),
    (["--history-ppo", "--privileged-actor"], "--history-ppo is a mode of its own"),
    (["--history"], "--history belongs to --distill"),
])
def test_train_refuses_the_arguments_where_they_do_not_belong(argv, text):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + argv, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode != 0 and "train.py: " + text in out, out[-2000:]
