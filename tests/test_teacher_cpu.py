"""The teacher policy's host side without a GPU: ppo.ActorCritic(actor_priv_dim=48), the zip round trip of a teacher and of a student,
the torch path of the privileged actor against float64, and ppo.Distill against float64 autograd."""
import math
import os
import re

import numpy as np
import pytest
import torch

from openroborl_amd import _abi, _lib, policy as pol, ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mlp64(p, net, x):
    h = torch.relu(x @ p["model/%s_fc0/w:0" % net] + p["model/%s_fc0/b:0" % net])
    h = torch.relu(h @ p["model/%s_fc1/w:0" % net] + p["model/%s_fc1/b:0" % net])
    return h @ p["model/%s/w:0" % net] + p["model/%s/b:0" % net]


def _random_biases(m, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in m.p.items():
            if k.endswith("/b:0"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))


def test_both_entry_points_are_declared():
    policy = open(os.path.join(ROOT, "include", "openroborl_policy.h")).read()
    learner = open(os.path.join(ROOT, "include", "openroborl_learner.h")).read()
    assert re.search(r"int32_t orr_policy_forward_teacher\(const orr_policy_net\* net, const float\* obs, const float\* priv, int32_t n,", policy)
    assert re.search(r"int32_t orr_distill_head\(const float\* mean, const float\* target, int32_t m, float\* g_mean, float\* gb_mean,", learner)
    assert "orr_policy_forward_teacher" in _lib.EXPORTS and "orr_distill_head" in _lib.EXPORTS and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert len(_abi.POLICY_FORWARD_TEACHER_ARGS) == 12 and len(_abi.DISTILL_HEAD_ARGS) == 8
    L = _lib.load()
    assert L.orr_policy_forward_teacher.argtypes == _abi.POLICY_FORWARD_TEACHER_ARGS == L.orr_policy_forward_priv.argtypes
    assert L.orr_distill_head.argtypes == _abi.DISTILL_HEAD_ARGS
    # host-side refusals (no launch happens on these paths)
    net = _abi.OrrPolicyNet()
    assert L.orr_policy_forward_teacher(None, 16, 16, 4, None, 0.125, 6.28, 16, None, None, None, None) == -1
    assert b"orr_policy_forward_teacher" in L.orr_last_error()
    assert L.orr_policy_forward_teacher(net, 16, 16, 4, None, 0.125, 6.28, 16, None, None, None, None) == -1 and b"null pointer" in L.orr_last_error()
    assert L.orr_distill_head(None, None, 16, None, None, None, None, None) == -1 and b"orr_distill_head" in L.orr_last_error()
    assert L.orr_distill_head(16, 16, 0, 16, 16, 16, 16, None) == -1
    assert L.orr_distill_head(16, 20, 16, 16, 16, 16, 16, None) == -1 and b"16-byte aligned" in L.orr_last_error()


def test_actor_critic_widths_and_the_value_errors():
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.p.items()}   # noqa: E731
    plain, critic, teacher = ppo.ActorCritic("cpu", seed=3), ppo.ActorCritic("cpu", seed=3, priv_dim=48), ppo.ActorCritic("cpu", seed=3, priv_dim=48, actor_priv_dim=48)
    assert (plain.actor_priv_dim, critic.actor_priv_dim, teacher.actor_priv_dim) == (0, 0, 48) and teacher.priv_dim == 48
    assert shapes(plain)["model/pi_fc0/w:0"] == shapes(critic)["model/pi_fc0/w:0"] == (160, 512)
    assert shapes(teacher)["model/pi_fc0/w:0"] == shapes(teacher)["model/vf_fc0/w:0"] == (208, 512)
    for k in teacher.p:
        if "fc0/w" not in k:
            assert shapes(teacher)[k] == shapes(plain)[k], k
    # the same rule: N(0, 1) * sqrt(2) / sqrt(fan_in) with the new fan_in
    assert abs(float(teacher.p["model/pi_fc0/w:0"].detach().std()) * math.sqrt(208.0 / 2.0) - 1.0) < 0.02
    # actor_priv_dim = 0 is today's model, draw for draw
    for k in critic.p:
        assert torch.equal(ppo.ActorCritic("cpu", seed=3, priv_dim=48, actor_priv_dim=0).p[k].detach(), critic.p[k].detach()), k
    for kw in (dict(actor_priv_dim=48), dict(priv_dim=0, actor_priv_dim=48), dict(priv_dim=48, actor_priv_dim=32), dict(priv_dim=48, actor_priv_dim=-1)):
        with pytest.raises(ValueError):
            ppo.ActorCritic("cpu", **kw)
    g = torch.Generator().manual_seed(0)
    obs, priv, act = torch.randn(5, 160, generator=g), torch.randn(5, 48, generator=g), torch.randn(5, 12, generator=g)
    for call in (lambda: teacher.mean(obs), lambda: teacher.log_prob(obs, act), lambda: teacher.act(obs), lambda: teacher.act(obs, deterministic=True),
                 lambda: critic.mean(obs, priv), lambda: critic.log_prob(obs, act, priv), lambda: plain.mean(obs, priv), lambda: plain.act(obs, priv)):
        with pytest.raises(ValueError):
            call()
    # and the calls that are right
    assert tuple(teacher.mean(obs, priv).shape) == (5, 12) and tuple(teacher.log_prob(obs, act, priv).shape) == (5,)
    a, raw, v = teacher.act(obs, priv, deterministic=True)
    assert torch.equal(raw, teacher.mean(obs, priv).detach()) and torch.equal(v, teacher.value(obs, priv).detach())
    a, raw, v = critic.act(obs, priv, deterministic=True)               # a privileged critic alone: the actor does not see the row
    assert torch.equal(raw, critic.mean(obs).detach())


def test_zip_round_trip_keeps_both_widths_and_a_student_is_a_plain_policy(tmp_path):
    teacher = ppo.ActorCritic("cpu", seed=5, priv_dim=48, actor_priv_dim=48)
    _random_biases(teacher)
    path = str(tmp_path / "teacher.zip")
    pol.save_parameters_zip(path, teacher.state_dict())
    params = pol.load_parameters(path)
    assert params["model/pi_fc0/w:0"].shape == (208, 512) and params["model/vf_fc0/w:0"].shape == (208, 512)
    back = ppo.ActorCritic("cpu", params=params)
    assert back.priv_dim == 48 and back.actor_priv_dim == 48
    for k in teacher.p:
        assert torch.equal(back.p[k].detach(), teacher.p[k].detach()), k
    # a privileged critic's zip keeps a plain actor
    critic = ppo.ActorCritic("cpu", seed=5, priv_dim=48)
    pol.save_parameters_zip(path, critic.state_dict())
    back = ppo.ActorCritic("cpu", params=pol.load_parameters(path))
    assert back.priv_dim == 48 and back.actor_priv_dim == 0
    # a file whose actor is privileged and whose critic is not is refused
    bad = dict(teacher.state_dict())
    bad["model/vf_fc0/w:0"] = bad["model/vf_fc0/w:0"][:160]
    with pytest.raises(ValueError):
        ppo.ActorCritic("cpu", params=bad)
    # the student: a plain model, its zip loads as policy.MLPPolicy with the reference's shapes and computes the same mean
    student = ppo.ActorCritic("cpu", seed=6)
    _random_biases(student, 1)
    spath = str(tmp_path / "student.zip")
    pol.save_parameters_zip(spath, student.state_dict())
    sp = pol.load_parameters(spath)
    for name, shape in pol.SB_PARAMETER_LIST:
        assert sp[name].shape == shape, name
    mlp = pol.MLPPolicy.from_file(spath, "cpu")
    obs = torch.randn(9, 160, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        np.testing.assert_allclose(mlp.mean(obs).numpy(), student.mean(obs).numpy(), rtol=0, atol=1e-6)


def test_privileged_mean_matches_float64_and_zero_rows_give_the_plain_mean():
    teacher = ppo.ActorCritic("cpu", seed=3, priv_dim=48, actor_priv_dim=48)
    _random_biases(teacher)
    with torch.no_grad():
        teacher.p["model/pi/w:0"].mul_(30.0)
    g = torch.Generator().manual_seed(1)
    obs, priv = torch.randn(37, 160, generator=g) * 2.0, torch.randn(37, 48, generator=g) * 2.0
    with torch.no_grad():
        mu = teacher.mean(obs, priv)
    p64 = {k: v.detach().double() for k, v in teacher.p.items()}
    mu64 = _mlp64(p64, "pi", torch.cat((obs, priv), dim=1).double())
    assert float((mu.double() - mu64).abs().max()) < 2e-5 * max(1.0, float(mu64.abs().max()))
    assert float((mu64 - _mlp64(p64, "pi", torch.cat((obs, torch.zeros_like(priv)), dim=1).double())).abs().max()) > 1e-3     # the row matters
    # rows 160.. zeroed: the plain model with the first 160 rows
    plain = ppo.ActorCritic("cpu", seed=3)
    with torch.no_grad():
        teacher.p["model/pi_fc0/w:0"][160:] = 0.0
        for k in plain.p:
            if "/pi" in k:
                plain.p[k].copy_(teacher.p[k][:160] if k == "model/pi_fc0/w:0" else teacher.p[k])
        assert bool((teacher.mean(obs, priv) == plain.mean(obs)).all())


def test_distill_loss_and_gradients_match_float64_and_the_critic_is_untouched():
    B = 64
    teacher = ppo.ActorCritic("cpu", seed=1, priv_dim=48, actor_priv_dim=48)
    student = ppo.ActorCritic("cpu", seed=2)
    with torch.no_grad():
        teacher.p["model/pi/w:0"].mul_(30.0)
        student.p["model/pi/w:0"].mul_(30.0)         # gradients of the hidden layers well above Adam's epsilon
    _random_biases(student, 3)
    g = torch.Generator().manual_seed(4)
    obs, priv = torch.randn(B, 160, generator=g), torch.randn(B, 48, generator=g)
    with torch.no_grad():
        target = teacher.mean(obs, priv)
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in student.p.items()}
    loss64 = ((_mlp64(p64, "pi", obs.double()) - target.double()) ** 2).sum(dim=1).mean()
    loss64.backward()
    loss = ((student.mean(obs) - target) ** 2).sum(dim=1).mean()
    loss.backward()
    assert abs(loss.item() - loss64.item()) < 2e-4 * max(1.0, abs(loss64.item()))
    for k in sorted(student.p):
        if not k.startswith("model/pi"):
            assert student.p[k].grad is None and p64[k].grad is None, k
            continue
        g32, g64 = student.p[k].grad.detach().double(), p64[k].grad
        scale = g64.abs().max().item() + 1e-12
        assert (g32 - g64).abs().max().item() < 2e-3 * scale, (k, (g32 - g64).abs().max().item(), scale)
        cs = (g32 * g64).sum() / (g32.norm() * g64.norm() + 1e-30)
        assert cs.item() > 0.99999, (k, cs.item())
    # the learner: the first Adam step in closed form on the actor, nothing on the critic; the loss falls
    before = {k: v.detach().clone() for k, v in student.p.items()}
    for v in student.p.values():
        v.grad = None
    learner = ppo.Distill(student, lr=1e-4, adam_eps=1e-5, minibatch=B)
    first = learner.update(obs, target, epochs=1, generator=torch.Generator().manual_seed(0))
    assert abs(first - loss64.item()) < 2e-4 * max(1.0, abs(loss64.item()))
    for k in sorted(student.p):
        step = (student.p[k].detach() - before[k]).double()
        if not k.startswith("model/pi"):
            assert torch.equal(student.p[k].detach(), before[k]), k
            continue
        g64 = p64[k].grad
        big = g64.abs() > 1e-3
        assert big.any()
        assert (step - (-1e-4 * g64 / (g64.abs() + 1e-5)))[big].abs().max().item() < 2e-6, k
    last = [learner.update(obs, target, epochs=1, generator=torch.Generator().manual_seed(i)) for i in range(1, 20)][-1]
    assert last < first
    for k in student.p:
        if not k.startswith("model/pi"):
            assert torch.equal(student.p[k].detach(), before[k]), k
    with pytest.raises(ValueError):
        ppo.Distill(teacher)
