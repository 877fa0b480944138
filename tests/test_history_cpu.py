"""The history student's host side without a GPU: the three entry points' declarations and host-side refusals, ppo.ActorCritic(history=16),
the zip round trip, ppo.history_push on a hand-made sequence, and ppo.DistillHistory against float64 autograd."""
import io
import os
import re
import zipfile

import numpy as np
import pytest
import torch

from openroborl_amd import _abi, _lib, policy as pol, ppo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENC = {"model/enc_fc0/w:0": (512, 256), "model/enc_fc0/b:0": (256,), "model/enc_fc1/w:0": (256, 48), "model/enc_fc1/b:0": (48,)}


def _mlp64(p, net, x):
    h = torch.relu(x @ p["model/%s_fc0/w:0" % net] + p["model/%s_fc0/b:0" % net])
    h = torch.relu(h @ p["model/%s_fc1/w:0" % net] + p["model/%s_fc1/b:0" % net])
    return h @ p["model/%s/w:0" % net] + p["model/%s/b:0" % net]


def _enc64(p, hist):
    return torch.relu(hist @ p["model/enc_fc0/w:0"] + p["model/enc_fc0/b:0"]) @ p["model/enc_fc1/w:0"] + p["model/enc_fc1/b:0"]


def _student(seed, gain=30.0):
    m = ppo.ActorCritic("cpu", seed=seed, priv_dim=48, actor_priv_dim=48, history=16)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for k, v in m.p.items():
            if k.endswith("/b:0"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
        m.p["model/pi/w:0"].mul_(gain)
    return m


def test_the_three_entry_points_are_declared_and_refuse_on_the_host():
    policy = open(os.path.join(ROOT, "include", "openroborl_policy.h")).read()
    learner = open(os.path.join(ROOT, "include", "openroborl_learner.h")).read()
    assert re.search(r"int32_t orr_history_push\(const float\* obs, const uint8_t\* done, const float\* prev, float\* next, int32_t n, void\* stream\);", policy)
    assert re.search(r"int32_t orr_policy_forward_history\(const orr_policy_net\* net, const orr_history_encoder\* enc, const float\* obs, const float\* hist, int32_t n,", policy)
    assert re.search(r"int32_t orr_regress_head\(const float\* pred, const float\* target, int32_t m, int32_t c, float\* g, float\* gb, float\* stats, float\* workspace,", learner)
    for name, value in (("ORR_HISTORY_STEPS", 16), ("ORR_HISTORY_FRAME", 32), ("ORR_HISTORY_DIM", 512)):
        assert re.search(r"#define %s %d\b" % (name, value), policy), name
    assert (_abi.HISTORY_STEPS, _abi.HISTORY_FRAME, _abi.HISTORY_DIM) == (16, 32, 512) == (ppo.HISTORY_STEPS, ppo.HISTORY_FRAME, ppo.HISTORY_DIM)
    for name in ("orr_history_push", "orr_policy_forward_history", "orr_regress_head"):
        assert name in _lib.EXPORTS
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert len(_abi.HISTORY_PUSH_ARGS) == 6 and len(_abi.POLICY_FORWARD_HISTORY_ARGS) == 14 and len(_abi.REGRESS_HEAD_ARGS) == 9
    assert [f for f, _ in _abi.OrrHistoryEncoder._fields_] == ["w0", "b0", "w1", "b1"]
    L = _lib.load()
    assert L.orr_history_push.argtypes == _abi.HISTORY_PUSH_ARGS and L.orr_regress_head.argtypes == _abi.REGRESS_HEAD_ARGS
    assert L.orr_policy_forward_history.argtypes == _abi.POLICY_FORWARD_HISTORY_ARGS
    # host-side refusals (no launch happens on these paths; the "pointers" are never read)
    err = lambda: L.orr_last_error()   # noqa: E731
    for args in ((None, None, None, 1024, 4, None), (1024, None, None, None, 4, None), (1024, None, None, 4096, 0, None), (1024, None, None, 4096, -2, None),
                 (1024, 512, None, 4096, 4, None)):                        # a null obs, a null next, n <= 0, done without prev
        assert L.orr_history_push(*args) == -1 and b"orr_history_push: bad argument" in err(), args
    for args in ((1026, None, None, 4096, 4, None), (1024, 512, 4096 + 8, 1 << 20, 4, None), (1024, 512, 4096, (1 << 20) + 4, 4, None)):
        assert L.orr_history_push(*args) == -1 and b"orr_history_push" in err() and b"aligned" in err(), args
    n = 4
    for prev, nxt in ((4096, 4096 + 2048), (4096 + 2048 * n - 16, 4096), (4096, 4096 + 2048 * n - 16)):      # n rows of 2048 bytes: partly overlapping
        assert L.orr_history_push(1024, 512, prev, nxt, n, None) == -1 and b"orr_history_push" in err() and b"overlap" in err(), (prev, nxt)
    net, enc = _abi.OrrPolicyNet(), _abi.OrrHistoryEncoder()
    fwd = lambda net_p, enc_p, obs, hist, count, action=16: L.orr_policy_forward_history(net_p, enc_p, obs, hist, count, None, 0.125, 6.28, action, None,   # noqa: E731
                                                                                          None, None, None, None)
    for args in ((None, enc, 16, 16, 4), (net, None, 16, 16, 4), (net, enc, None, 16, 4), (net, enc, 16, None, 4), (net, enc, 16, 16, 0), (net, enc, 16, 16, 4, None)):
        assert fwd(*args) == -1 and b"orr_policy_forward_history: bad argument" in err(), args
    assert fwd(net, enc, 16, 16, 4) == -1 and b"orr_policy_net has a null pointer" in err()
    for f, _ in _abi.OrrPolicyNet._fields_:
        setattr(net, f, 64)
    assert fwd(net, enc, 16, 16, 4) == -1 and b"orr_history_encoder has a null pointer" in err() and b"orr_policy_forward_history" in err()
    enc.w0, enc.b0, enc.w1, enc.b1 = 64, 64, 64 + 4, 64
    assert fwd(net, enc, 16, 16, 4) == -1 and b"16-byte aligned" in err()
    enc.w1 = 64
    assert fwd(net, enc, 16, 16 + 4, 4) == -1 and b"hist must be 16-byte aligned" in err()
    assert fwd(net, enc, 16 + 2, 16, 4) == -1 and b"4-byte aligned" in err()
    assert L.orr_regress_head(None, None, 16, 48, None, None, None, None, None) == -1 and b"orr_regress_head: bad argument" in err()
    assert L.orr_regress_head(16, 16, 0, 48, 16, 16, 16, 16, None) == -1 and b"orr_regress_head" in err()
    for c in (0, 46, 68, -4):
        assert L.orr_regress_head(16, 16, 16, c, 16, 16, 16, 16, None) == -1 and b"multiple of 4, at most 64" in err(), c
    assert L.orr_regress_head(16, 20, 16, 48, 16, 16, 16, 16, None) == -1 and b"16-byte aligned" in err()


def test_actor_critic_with_a_history_encoder():
    teacher = ppo.ActorCritic("cpu", seed=3, priv_dim=48, actor_priv_dim=48)
    student = ppo.ActorCritic("cpu", seed=3, priv_dim=48, actor_priv_dim=48, history=16)
    assert teacher.history == 0 and student.history == 16
    assert {k: tuple(v.shape) for k, v in student.p.items() if k.startswith("model/enc_")} == ENC
    assert sorted(set(student.p) - set(teacher.p)) == sorted(ENC)
    # drawn after every other parameter: history = 0 is today's model, draw for draw - and so is the rest of a history student
    again = ppo.ActorCritic("cpu", seed=3, priv_dim=48, actor_priv_dim=48, history=0)
    for k in teacher.p:
        assert torch.equal(teacher.p[k].detach(), again.p[k].detach()) and torch.equal(teacher.p[k].detach(), student.p[k].detach()), k
    # the same rule: N(0, 1) * gain / sqrt(fan_in), gains sqrt(2) and 1; zero biases
    assert abs(float(student.p["model/enc_fc0/w:0"].detach().std()) * (512.0 / 2.0) ** 0.5 - 1.0) < 0.02
    assert abs(float(student.p["model/enc_fc1/w:0"].detach().std()) * 256.0 ** 0.5 - 1.0) < 0.03
    assert float(student.p["model/enc_fc0/b:0"].detach().abs().max()) == 0.0 and float(student.p["model/enc_fc1/b:0"].detach().abs().max()) == 0.0
    for kw in (dict(history=16), dict(priv_dim=48, history=16), dict(priv_dim=48, actor_priv_dim=48, history=8), dict(priv_dim=48, actor_priv_dim=48, history=-1)):
        with pytest.raises(ValueError):
            ppo.ActorCritic("cpu", **kw)
    # with params the presence of the encoder decides
    assert ppo.ActorCritic("cpu", params=student.state_dict()).history == 16 and ppo.ActorCritic("cpu", params=teacher.state_dict(), history=16).history == 0
    g = torch.Generator().manual_seed(0)
    obs, priv, hist = torch.randn(5, 160, generator=g), torch.randn(5, 48, generator=g), torch.randn(5, 512, generator=g)
    for call in (lambda: student.mean(obs, priv, hist=hist), lambda: student.act(obs, priv, hist=hist), lambda: teacher.mean(obs, hist=hist),
                 lambda: teacher.act(obs, hist=hist), lambda: teacher.encode(hist), lambda: student.mean(obs), lambda: student.act(obs),
                 lambda: ppo.PPO(student), lambda: ppo.Distill(student), lambda: ppo.DistillHistory(teacher)):
        with pytest.raises(ValueError):
            call()
    with torch.no_grad():
        z = student.encode(hist)
        assert tuple(z.shape) == (5, 48)
        assert torch.equal(student.mean(obs, hist=hist), student.mean(obs, z))
        a, raw, v = student.act(obs, hist=hist, deterministic=True)
        assert torch.equal(raw, student.mean(obs, z)) and torch.equal(v, student.value(obs, z))
        # the row itself still works: a history student is a teacher with an encoder
        assert torch.equal(student.act(obs, priv, deterministic=True)[1], student.mean(obs, priv))


def test_mean_from_the_history_matches_float64():
    student = _student(3)
    g = torch.Generator().manual_seed(1)
    obs, hist = torch.randn(37, 160, generator=g) * 2.0, torch.randn(37, 512, generator=g) * 2.0
    with torch.no_grad():
        mu, z = student.mean(obs, hist=hist), student.encode(hist)
    p64 = {k: v.detach().double() for k, v in student.p.items()}
    z64 = _enc64(p64, hist.double())
    mu64 = _mlp64(p64, "pi", torch.cat((obs.double(), z64), dim=1))
    assert float((z.double() - z64).abs().max()) < 2e-5 * max(1.0, float(z64.abs().max()))
    assert float((mu.double() - mu64).abs().max()) < 2e-5 * max(1.0, float(mu64.abs().max()))
    assert float(mu64.abs().max()) > 0.1
    assert float((mu64 - _mlp64(p64, "pi", torch.cat((obs.double(), torch.zeros_like(z64)), dim=1))).abs().max()) > 1e-3      # the history matters


def test_zip_round_trip_of_a_history_student_and_other_zips_are_unchanged(tmp_path):
    student = _student(5)
    path = str(tmp_path / "student.zip")
    pol.save_parameters_zip(path, student.state_dict())
    params = pol.load_parameters(path)
    for k, shape in ENC.items():
        assert params[k].shape == shape, k
    back = ppo.ActorCritic("cpu", params=params)
    assert back.history == 16 and back.actor_priv_dim == 48 and back.priv_dim == 48
    for k in student.p:
        assert torch.equal(back.p[k].detach(), student.p[k].detach()), k
    with zipfile.ZipFile(path) as z:
        import json
        names = json.loads(z.read("parameter_list"))
    assert names == [n for n, _ in pol.SB_PARAMETER_LIST] + [n for n, _ in pol.ENC_PARAMETER_LIST]       # behind the reference's list
    bad = dict(student.state_dict())
    bad["model/enc_fc1/w:0"] = bad["model/enc_fc1/w:0"][:, :47]
    with pytest.raises(ValueError):
        pol.save_parameters_zip(str(tmp_path / "bad.zip"), bad)
    # a zip without an encoder: what it was before the encoder existed - the reference's variable list and nothing else, in its order
    for i, model in enumerate((ppo.ActorCritic("cpu", seed=6), ppo.ActorCritic("cpu", seed=6, priv_dim=48, actor_priv_dim=48))):
        p = str(tmp_path / ("plain%d.zip" % i))
        pol.save_parameters_zip(p, model.state_dict())
        with zipfile.ZipFile(p) as z:
            assert z.namelist() == ["data", "parameter_list", "parameters"]
            assert json.loads(z.read("parameter_list")) == [n for n, _ in pol.SB_PARAMETER_LIST]
            assert np.load(io.BytesIO(z.read("parameters"))).files == [n for n, _ in pol.SB_PARAMETER_LIST]
        assert ppo.ActorCritic("cpu", params=pol.load_parameters(p)).history == 0


def test_history_push_on_a_hand_made_sequence_with_a_reset():
    n, steps, reset_at = 3, 20, 9                 # robot 1 resets at step 9; robot 2 at steps 9 and 10
    g = torch.Generator().manual_seed(2)
    obs = torch.randn(steps + 1, n, 160, generator=g)
    done = torch.zeros(steps, n, dtype=torch.bool)
    done[reset_at, 1] = done[reset_at, 2] = done[reset_at + 1, 2] = True
    frame = lambda o: torch.cat((o[:, 0:4], o[:, 12:24], o[:, 48:60], torch.zeros(o.shape[0], 4)), dim=1)   # noqa: E731
    assert torch.equal(ppo.history_frame(obs[0]), frame(obs[0]))
    hist = ppo.history_push(None, obs[0], None)
    assert tuple(hist.shape) == (n, 512)
    assert torch.equal(hist.view(n, 16, 32), frame(obs[0])[:, None, :].expand(n, 16, 32))
    start = [0] * n                                # the step whose observation began each robot's episode
    for k in range(steps):
        before = hist.clone()
        nxt = ppo.history_push(hist, obs[k + 1], done[k])
        assert torch.equal(hist, before)                            # the input is not written
        assert torch.equal(nxt, ppo.history_push(hist, obs[k + 1], done[k].to(torch.uint8)))     # flags as the env writes them
        hist = nxt
        h = hist.view(n, 16, 32)
        assert bool((h[:, :, 28:] == 0).all())                      # the pad words
        for i in range(n):
            if done[k, i]:
                start[i] = k + 1
            for s in range(16):
                src = max(k + 1 - s, start[i])                      # slot s: the frame of s steps ago, or the episode's first
                assert torch.equal(h[i, s], frame(obs[src])[i]), (k, i, s)
    assert start == [0, reset_at + 1, reset_at + 2]


def test_distill_history_matches_float64_and_trains_the_encoder_alone():
    B = 64
    student = _student(2)
    g = torch.Generator().manual_seed(4)
    hist, target = torch.randn(B, 512, generator=g), torch.randn(B, 48, generator=g)
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in student.p.items()}
    loss64 = ((_enc64(p64, hist.double()) - target.double()) ** 2).sum(dim=1).mean()
    loss64.backward()
    loss = ((student.encode(hist) - target) ** 2).sum(dim=1).mean()
    loss.backward()
    assert abs(loss.item() - loss64.item()) < 2e-4 * max(1.0, abs(loss64.item()))
    for k in sorted(student.p):
        if not k.startswith("model/enc_"):
            assert student.p[k].grad is None and p64[k].grad is None, k
            continue
        g32, g64 = student.p[k].grad.detach().double(), p64[k].grad
        scale = g64.abs().max().item() + 1e-12
        assert (g32 - g64).abs().max().item() < 2e-3 * scale, (k, (g32 - g64).abs().max().item(), scale)
        cs = (g32 * g64).sum() / (g32.norm() * g64.norm() + 1e-30)
        assert cs.item() > 0.99999, (k, cs.item())
    # the learner: the first Adam step in closed form on the encoder, nothing on the actor or the critic; the loss falls
    before = {k: v.detach().clone() for k, v in student.p.items()}
    for v in student.p.values():
        v.grad = None
    learner = ppo.DistillHistory(student, lr=1e-4, adam_eps=1e-5, minibatch=B)
    first = learner.update(hist, target, epochs=1, generator=torch.Generator().manual_seed(0))
    assert abs(first - loss64.item()) < 2e-4 * max(1.0, abs(loss64.item()))
    for k in sorted(student.p):
        if not k.startswith("model/enc_"):
            assert torch.equal(student.p[k].detach(), before[k]), k
            continue
        step = (student.p[k].detach() - before[k]).double()
        g64 = p64[k].grad
        big = g64.abs() > 1e-3
        assert big.any()
        assert (step - (-1e-4 * g64 / (g64.abs() + 1e-5)))[big].abs().max().item() < 2e-6, k
    last = [learner.update(hist, target, epochs=1, generator=torch.Generator().manual_seed(i)) for i in range(1, 20)][-1]
    assert last < first
    for k in student.p:
        if not k.startswith("model/enc_"):
            assert torch.equal(student.p[k].detach(), before[k]), k
