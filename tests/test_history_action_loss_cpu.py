"""The history student's action loss without a GPU: ppo.DistillHistory(action_coef, latent_coef) against a float64 computation written out
here, the default coefficients against a learner built without them (bit for bit), the frozen actor and critic, the ValueErrors, the
declaration and host-side refusals of orr_history_student_head, and train.py's argument refusals in child processes."""
import os
import re
import subprocess
import sys

import pytest
import torch

from openroborl_amd import _abi, _lib, ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, M = 32, 16


def _student(seed, gain=30.0):
    """tests/test_history_cpu.py's: random biases, actor outputs of O(1)"""
    m = ppo.ActorCritic("cpu", seed=seed, priv_dim=48, actor_priv_dim=48, history=16)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for k, v in m.p.items():
            if k.endswith("/b:0"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
        m.p["model/pi/w:0"].mul_(gain)
    return m


def _data(seed=4):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 512, generator=g), torch.randn(B, 48, generator=g), torch.randn(B, 160, generator=g), torch.randn(B, 12, generator=g))


def _losses64(p, hist, priv, obs, mean):
    """forward and both losses in float64, written out: z = relu(hist W0 + b0) W1 + b1; the actor on obs | z"""
    z = torch.relu(hist @ p["model/enc_fc0/w:0"] + p["model/enc_fc0/b:0"]) @ p["model/enc_fc1/w:0"] + p["model/enc_fc1/b:0"]
    h = torch.relu(torch.cat((obs, z), dim=1) @ p["model/pi_fc0/w:0"] + p["model/pi_fc0/b:0"])
    h = torch.relu(h @ p["model/pi_fc1/w:0"] + p["model/pi_fc1/b:0"])
    mu = h @ p["model/pi/w:0"] + p["model/pi/b:0"]
    return ((mu - mean) ** 2).sum(dim=1).mean(), ((z - priv) ** 2).sum(dim=1).mean()


@pytest.mark.parametrize("a,b", [(1.0, 0.0), (0.7, 0.3), (1.0, 0.5)])
def test_distill_history_with_an_action_loss_matches_float64(a, b):
    """One epoch of two minibatches at lr = 0: the parameters stand still, so each minibatch's losses and gradients are those of the float64
    computation on the same rows; then the first real step in closed form (Adam's first step is lr * sign-like g / (|g| + eps))."""
    student = _student(2)
    hist, priv, obs, mean = _data()
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in student.p.items()}
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(0))
    want = []
    for s in range(0, B, M):
        i = perm[s:s + M]
        act64, lat64 = _losses64(p64, hist[i].double(), priv[i].double(), obs[i].double(), mean[i].double())
        grads = torch.autograd.grad(a * act64 + b * lat64, [p64[k] for k in sorted(p64) if k.startswith("model/enc_")])
        want.append((act64.item(), lat64.item(), grads))
    learner = ppo.DistillHistory(student, lr=0.0, minibatch=M, action_coef=a, latent_coef=b)
    total = learner.update(hist, priv, 1, torch.Generator().manual_seed(0), obs=obs, target_mean=mean)
    act, lat = sum(w[0] for w in want) / 2, sum(w[1] for w in want) / 2
    print("losses: action %.6f (float64 %.6f), latent %.6f (%.6f)" % (learner.last_action_loss, act, learner.last_latent_loss, lat))
    assert abs(learner.last_action_loss - act) < 2e-4 * max(1.0, act) and abs(learner.last_latent_loss - lat) < 2e-4 * max(1.0, lat)
    assert abs(total - (a * act + b * lat)) < 2e-4 * max(1.0, a * act + b * lat)
    assert act > 0.1 and lat > 0.1
    # the gradients left behind are the last minibatch's
    enc = [k for k in sorted(student.p) if k.startswith("model/enc_")]
    for k, g64 in zip(enc, want[-1][2]):
        g32 = student.p[k].grad.detach().double()
        scale = g64.abs().max().item() + 1e-12
        cs = (g32 * g64).sum() / (g32.norm() * g64.norm() + 1e-30)
        print("%s: gradient error %.2e of its scale, 1 - cosine %.2e" % (k, (g32 - g64).abs().max().item() / scale, 1.0 - cs.item()))
        assert (g32 - g64).abs().max().item() < 2e-3 * scale, k
        assert cs.item() > 0.99999, k
    for k in student.p:
        if not k.startswith("model/enc_"):
            assert student.p[k].grad is None, k          # the frozen nets keep no gradient
    # a gradient that the latent loss alone does not have: the action loss reaches the encoder
    lat_only = torch.autograd.grad(_losses64(p64, hist.double(), priv.double(), obs.double(), mean.double())[1], p64["model/enc_fc1/b:0"])[0]
    both = torch.autograd.grad(sum(c * l for c, l in zip((a, b), _losses64(p64, hist.double(), priv.double(), obs.double(), mean.double()))),
                               p64["model/enc_fc1/b:0"])[0]
    assert (both - b * lat_only).abs().max().item() > 1e-3


def test_default_coefficients_are_the_learner_without_them_bit_for_bit():
    hist, priv, obs, mean = _data()
    finals = []
    for kw in (dict(), dict(action_coef=0.0, latent_coef=1.0)):
        student = _student(3)
        learner = ppo.DistillHistory(student, lr=1e-3, minibatch=M, **kw)
        losses = [learner.update(hist, priv, epochs=1, generator=torch.Generator().manual_seed(i)) for i in range(2)]
        assert learner.last_action_loss == 0.0 and abs(learner.last_latent_loss - losses[-1]) < 1e-6 * losses[-1]
        finals.append(({k: v.detach().clone() for k, v in student.p.items()}, losses))
    assert finals[0][1] == finals[1][1]
    for k in finals[0][0]:
        assert torch.equal(finals[0][0][k], finals[1][0][k]), k
    # obs and target_mean are accepted and ignored without an action loss
    student = _student(3)
    learner = ppo.DistillHistory(student, lr=1e-3, minibatch=M)
    for i in range(2):
        learner.update(hist, priv, 1, torch.Generator().manual_seed(i), obs=obs, target_mean=mean)
    for k in finals[0][0]:
        assert torch.equal(finals[0][0][k], student.p[k].detach()), k


def test_the_actor_and_the_critic_are_unchanged_and_the_action_loss_falls():
    student = _student(5)
    hist, priv, obs, mean = _data(7)
    before = {k: v.detach().clone() for k, v in student.p.items()}
    learner = ppo.DistillHistory(student, lr=1e-3, minibatch=M, action_coef=1.0, latent_coef=0.0)
    losses = [learner.update(hist, priv, 1, torch.Generator().manual_seed(i), obs=obs, target_mean=mean) for i in range(20)]
    assert losses[-1] < losses[0]
    moved = 0.0
    for k in student.p:
        if k.startswith("model/enc_"):
            moved = max(moved, (student.p[k].detach() - before[k]).abs().max().item())
        else:
            assert torch.equal(student.p[k].detach(), before[k]), k
    assert moved > 1e-3


def test_value_errors():
    student = _student(1)
    hist, priv, obs, mean = _data()
    learner = ppo.DistillHistory(student, minibatch=M, action_coef=0.5)
    for kw in (dict(), dict(obs=obs), dict(target_mean=mean), dict(obs=obs[:, :159], target_mean=mean), dict(obs=obs, target_mean=mean[:, :11]),
               dict(obs=obs[:B - 1], target_mean=mean), dict(obs=obs, target_mean=mean[:B - 1])):
        with pytest.raises(ValueError):
            learner.update(hist, priv, 1, None, **kw)
    for kw in (dict(action_coef=-1.0), dict(latent_coef=-0.5)):
        with pytest.raises(ValueError):
            ppo.DistillHistory(student, **kw)
    for k, v in student.p.items():
        assert v.grad is None, k                       # a refused update computes nothing


def test_the_entry_point_is_declared_and_refuses_on_the_host():
    learner = open(os.path.join(ROOT, "include", "openroborl_learner.h")).read()
    assert re.search(r"int32_t orr_history_student_head\(const orr_policy_net\* net, const float\* w2t, const float\* w1t, const float\* w0zt, "
                     r"const float\* obs, const float\* z,\s+const float\* target_mean, const float\* target_priv, int32_t m, float action_coef, "
                     r"float latent_coef, float\* g_z,\s+float\* mean, float\* partials, void\* stream\);", learner)
    assert re.search(r"#define ORR_STUDENT_HEAD_ROWS\(m\) \(\(\(m\) \+ 15\) / 16\)", learner)
    assert "orr_history_student_head" in _lib.EXPORTS and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert len(_abi.HISTORY_STUDENT_HEAD_ARGS) == 15
    assert [_abi.student_head_rows(m) for m in (1, 15, 16, 17, 33, 16384)] == [1, 1, 1, 2, 3, 1024]
    L = _lib.load()
    assert L.orr_history_student_head.argtypes == _abi.HISTORY_STUDENT_HEAD_ARGS
    # host-side refusals (no launch happens on these paths; the "pointers" are never read)
    net = _abi.OrrPolicyNet()
    for f in ("w0_pi", "b0_pi", "w1_pi", "b1_pi", "w2_pi", "b2_pi"):         # the critic's members stay NULL: they are not read
        setattr(net, f, 64)
    good = dict(net=net, w2t=64, w1t=64, w0zt=64, obs=64, z=64, tm=64, tp=64, m=4, g_z=64, mean=None, partials=64)

    def call(**kw):
        a = dict(good, **kw)
        return L.orr_history_student_head(a["net"], a["w2t"], a["w1t"], a["w0zt"], a["obs"], a["z"], a["tm"], a["tp"], a["m"], 1.0, 0.5, a["g_z"], a["mean"],
                                          a["partials"], None)
    err = lambda: L.orr_last_error()   # noqa: E731
    for kw in (dict(net=None), dict(w2t=None), dict(w1t=None), dict(w0zt=None), dict(obs=None), dict(z=None), dict(tm=None), dict(tp=None), dict(g_z=None),
               dict(partials=None), dict(m=0), dict(m=-5)):
        assert call(**kw) == -1 and b"orr_history_student_head: bad argument" in err(), kw
    for f in ("w0_pi", "b0_pi", "w1_pi", "b1_pi", "w2_pi", "b2_pi"):
        setattr(net, f, None)
        assert call() == -1 and b"orr_history_student_head" in err() and b"null pointer" in err(), f
        setattr(net, f, 64 + (4 if f.startswith("w") else 2))
        assert call() == -1 and b"orr_history_student_head" in err() and b"aligned" in err(), f
        setattr(net, f, 64)
    for kw in (dict(w2t=64 + 4), dict(w1t=64 + 8), dict(w0zt=64 + 12)):
        assert call(**kw) == -1 and b"orr_history_student_head" in err() and b"16-byte aligned" in err(), kw
    for kw in (dict(obs=64 + 2), dict(z=64 + 1), dict(tm=64 + 3), dict(tp=64 + 2), dict(g_z=64 + 2), dict(mean=64 + 1), dict(partials=64 + 2)):
        assert call(**kw) == -1 and b"orr_history_student_head" in err() and b"4-byte aligned" in err(), kw


@pytest.mark.parametrize("argv,text", [
    (["--distill-action-coef", "1"], "belong to --distill --history"),
    (["--distill-latent-coef", "0.5"], "belong to --distill --history"),
    (["--distill", "teacher.zip", "--distill-action-coef", "1"], "belong to --distill --history"),
    (["--distill", "teacher.zip", "--history", "--distill-action-coef", "-1"], "must not be negative"),
    (["--distill", "teacher.zip", "--history", "--distill-latent-coef", "-0.5"], "must not be negative"),
])
def test_train_refuses_the_coefficients_where_they_do_not_belong(argv, text):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + argv, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode != 0 and "train.py: --distill-action-coef / --distill-latent-coef " + text in out, out[-2000:]
