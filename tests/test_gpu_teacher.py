"""The teacher policy on the device (run with -m gpu on an MI355X):

  a-d. orr_policy_forward_teacher: mean and value against the float64 MLPs on cat(obs, priv), the tile's edges, the guard bands; against
       orr_policy_forward and orr_policy_forward_priv bit for bit where they compute the same thing; value = NULL; the refusals;
  e.   orr_distill_head against float64;
  f.   learner_hip.FusedDistill against ppo.Distill;
  g.   learner_hip.FusedPPO with a privileged actor against ppo.PPO and against float64;
  h.   rollout.GraphRollout(teacher=) against rollout.collect_rollout and against a twin env stepped by hand;
  i.   distillation learns: the fused loss trajectory is ppo.Distill's, and falls;
  j.   train.py --privileged-actor, --distill and --eval in child processes.

Tolerances: those of tests/test_gpu_privileged.py (forward pass: 2e-5 max(1, max|.|)) and tests/test_gpu_learner.py (loss head: 2e-5 of the
gradient's scale, x sqrt(m) for a sum over m; learners: losses rtol 2e-4 / atol 2e-5, parameters 0.02 steps lr at most and 2e-3 steps lr
on average; gradients 2e-3 of their scale and a cosine above 0.99999)."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.gpu_kit import mixed_env, short_episodes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.25
CLIP = 2.0 * math.pi
PUSH = dict(prob=1.0, lin_vel=(0.1, 0.4), lin_vel_z=0.1, ang_vel=0.3)


def mlp64(p, net, x):
    import torch
    h = torch.relu(x.double() @ p["model/%s_fc0/w:0" % net].double() + p["model/%s_fc0/b:0" % net].double())
    h = torch.relu(h @ p["model/%s_fc1/w:0" % net].double() + p["model/%s_fc1/b:0" % net].double())
    return h @ p["model/%s/w:0" % net].double() + p["model/%s/b:0" % net].double()


def teacher_model(dev, seed):
    """A teacher with random biases and an actor whose outputs are O(1) (the initialisation's gain of the output layer is 0.01)"""
    import torch
    from openroborl_amd import ppo
    model = ppo.ActorCritic(dev, seed=seed, priv_dim=48, actor_priv_dim=48)
    with torch.no_grad():
        for k, v in model.p.items():
            if k.endswith("/b:0"):
                v.copy_(torch.randn(v.shape, generator=torch.Generator().manual_seed(len(k))).to(dev) * 0.1)
        model.p["model/pi/w:0"].mul_(30.0)
    return model


# ---- a-d. the forward pass ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    """A teacher, its fused copy, the privileged-critic model with the first 160 rows of its actor, and the plain model with the first 160
    rows of both"""
    import torch
    from openroborl_amd import policy_hip
    dev = torch.device("cuda", 0)
    model = teacher_model(dev, 3)
    critic = {k: v.detach().clone() for k, v in model.p.items()}
    critic["model/pi_fc0/w:0"] = model.p["model/pi_fc0/w:0"].detach()[:160].clone()
    plain = dict(critic)
    plain["model/vf_fc0/w:0"] = model.p["model/vf_fc0/w:0"].detach()[:160].clone()
    return model, policy_hip.FusedActorCritic(model.p, dev, std=0.125), policy_hip.FusedActorCritic(critic, dev, std=0.125), \
        policy_hip.FusedActorCritic(plain, dev, std=0.125)


def raw_forward(fused, entry, obs, priv, noise, n, value=True, guard=16):
    """A C entry point with the test's own output buffers: n rows + a guard band in each"""
    import torch
    dev = obs.device
    outs = [torch.full((n + guard, c), SENTINEL, device=dev) for c in (12, 12, 1, 12)]      # action, raw, value, mean
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tail = (noise.data_ptr(), 0.125, CLIP, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr() if value else None, outs[3].data_ptr(), st)
    if entry == "plain":
        rc = fused.L.orr_policy_forward(C.byref(fused.net), obs.data_ptr(), n, *tail)
    else:
        fn = fused.L.orr_policy_forward_priv if entry == "priv" else fused.L.orr_policy_forward_teacher
        rc = fn(C.byref(fused.net), obs.data_ptr(), priv.data_ptr(), n, *tail)
    assert rc == 0, fused.L.orr_last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o[n:] == SENTINEL).all())                      # rows beyond n are not written
    if not value:
        assert bool((outs[2] == SENTINEL).all())
    return [o[:n] for o in outs]


def inputs(dev, n, seed):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(n, 160, generator=g, device=dev) * 2.0, torch.randn(n, 48, generator=g, device=dev) * 2.0,
            torch.randn(n, 12, generator=g, device=dev))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_forward_teacher_matches_float64(nets, n):
    import torch
    model, fused, fused_critic, _ = nets
    assert fused.priv_dim == 48 and fused.actor_priv_dim == 48 and fused_critic.actor_priv_dim == 0
    dev = model.device
    obs, priv, noise = inputs(dev, n, 100 + n)
    act, raw, val, mean = raw_forward(fused, "teacher", obs, priv, noise, n)
    x = torch.cat((obs, priv), dim=1)
    mu64, v64 = mlp64(model.p, "pi", x).detach(), mlp64(model.p, "vf", x).detach()[:, 0]
    err_m, err_v = float((mean.double() - mu64).abs().max()), float((val[:, 0].double() - v64).abs().max())
    print("n = %d: mean error %.2e of the bound %.2e, value error %.2e of the bound %.2e"
          % (n, err_m, 2e-5 * max(1.0, float(mu64.abs().max())), err_v, 2e-5 * max(1.0, float(v64.abs().max()))))
    assert err_m < 2e-5 * max(1.0, float(mu64.abs().max()))
    assert err_v < 2e-5 * max(1.0, float(v64.abs().max()))
    assert torch.equal(act, raw.clamp(-CLIP, CLIP))
    assert float((raw.double() - (mean.double() + 0.125 * noise.double())).abs().max()) < 1e-6 * max(1.0, float(raw.abs().max()))
    assert float(mu64.abs().max()) > 0.1                             # an actor whose output is not all but zero
    # through the Python layer: the same numbers, and the vector is required
    a2, r2, v2, m2 = fused.forward(obs, noise, want_mean=True, priv=priv)
    assert torch.equal(a2, act) and torch.equal(r2, raw) and torch.equal(v2, val[:, 0]) and torch.equal(m2, mean)
    with pytest.raises(ValueError):
        fused.forward(obs, noise)
    with pytest.raises(ValueError):
        fused.forward(obs, noise, priv=priv[:, :47].contiguous())
    # obs zeroed and ONE privileged column set: the mean moves as the float64 MLP says (a transposed or shifted tile would not)
    zero = torch.zeros_like(obs)
    base = mlp64(model.p, "pi", torch.cat((zero, torch.zeros_like(priv)), dim=1)).detach()
    for col in (0, 17, 47):
        one = torch.zeros_like(priv)
        one[:, col] = torch.linspace(-2.0, 2.0, n, device=dev) if n > 1 else 1.5
        m = raw_forward(fused, "teacher", zero, one, noise, n)[3]
        w64 = mlp64(model.p, "pi", torch.cat((zero, one), dim=1)).detach()
        assert float((m.double() - w64).abs().max()) < 2e-5 * max(1.0, float(w64.abs().max())), col
        assert float((w64 - base).abs().max()) > 1e-3, col                         # the column matters


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_forward_teacher_is_consistent_with_the_two_older_kernels(nets, n):
    import torch
    from openroborl_amd import policy_hip
    model, fused, fused_critic, fused_plain = nets
    dev = model.device
    obs, priv, noise = inputs(dev, n, 200 + n)
    # the same critic weights: the same value, bit for bit
    val = raw_forward(fused, "teacher", obs, priv, noise, n)[2]
    val_priv = raw_forward(fused_critic, "priv", obs, priv, noise, n)[2]
    assert torch.equal(val, val_priv)
    # rows 160.. of the actor's layer 0 zeroed: the plain kernel's actor
    p = {k: v.detach().clone() for k, v in model.p.items()}
    p["model/pi_fc0/w:0"][160:] = 0.0
    fused0 = policy_hip.FusedActorCritic(p, dev, std=0.125)
    act, raw, _, mean = raw_forward(fused0, "teacher", obs, priv, noise, n)
    act0, raw0, _, mean0 = raw_forward(fused_plain, "plain", obs, None, noise, n)
    assert bool((act == act0).all()) and bool((raw == raw0).all()) and bool((mean == mean0).all())      # ==: a signed zero does not matter


@pytest.mark.parametrize("n", [1, 17, 33])
def test_forward_teacher_without_a_value_buffer(nets, n):
    import torch
    model, fused, _, _ = nets
    obs, priv, noise = inputs(model.device, n, 300 + n)
    act, raw, _, mean = raw_forward(fused, "teacher", obs, priv, noise, n)
    act1, raw1, val1, mean1 = raw_forward(fused, "teacher", obs, priv, noise, n, value=False)       # (checks that its value tensor keeps the sentinel)
    assert torch.equal(act, act1) and torch.equal(raw, raw1) and torch.equal(mean, mean1)
    assert bool((val1 == SENTINEL).all())
    # the Python layer: no value, the mean into the caller's tensor, no noise = the clipped mean
    out_mean = torch.full((n, 12), SENTINEL, device=model.device)
    a2, r2, v2, m2 = fused.forward(obs, None, priv=priv, out_mean=out_mean, want_value=False)
    assert v2 is None and m2.data_ptr() == out_mean.data_ptr() and torch.equal(out_mean, mean)
    assert torch.equal(r2, mean) and torch.equal(a2, mean.clamp(-CLIP, CLIP))
    with pytest.raises(ValueError):
        fused.forward(obs, None, priv=priv, out_value=torch.empty(n, device=model.device), want_value=False)


def test_forward_teacher_refusals_write_nothing(nets):
    import torch
    from openroborl_amd import _abi
    model, fused, _, _ = nets
    dev, n = model.device, 5
    L = fused.L
    obs, priv, noise = inputs(dev, n + 1, 7)
    outs = [torch.full((n + 1, c), SENTINEL, device=dev) for c in (12, 12, 1, 12)]
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(net=None, obs_p=obs.data_ptr(), priv_p=priv.data_ptr(), count=n, action_p=outs[0].data_ptr(), value_p=outs[2].data_ptr()):
        return L.orr_policy_forward_teacher(C.byref(fused.net) if net is None else net, obs_p, priv_p, count, noise.data_ptr(), 0.125, CLIP, action_p,
                                            outs[1].data_ptr(), value_p, outs[3].data_ptr(), st)
    no_member, odd = _abi.OrrPolicyNet(), _abi.OrrPolicyNet()
    C.memmove(C.byref(no_member), C.byref(fused.net), C.sizeof(fused.net))
    C.memmove(C.byref(odd), C.byref(fused.net), C.sizeof(fused.net))
    no_member.b1_vf = None
    odd.w0_pi = fused.net.w0_pi + 4
    for kw, text in ((dict(net=C.POINTER(_abi.OrrPolicyNet)()), b"bad argument"), (dict(obs_p=None), b"bad argument"), (dict(priv_p=None), b"bad argument"),
                     (dict(action_p=None), b"bad argument"), (dict(count=0), b"bad argument"), (dict(count=-3), b"bad argument"),
                     (dict(net=C.byref(no_member)), b"null pointer"), (dict(net=C.byref(odd)), b"16-byte aligned"),
                     (dict(obs_p=obs.data_ptr() + 2), b"4-byte aligned"), (dict(value_p=outs[2].data_ptr() + 1), b"4-byte aligned")):
        rc = call(**kw)
        assert rc < 0 and text in L.orr_last_error() and b"orr_policy_forward_teacher" in L.orr_last_error(), (kw, rc, L.orr_last_error())
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == SENTINEL).all())
    assert call() == 0                                               # and the same call with everything in place
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o[:n] != SENTINEL).all()) and bool((o[n:] == SENTINEL).all())


# ---- e. the loss head -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 1000, 4096])
def test_distill_head_matches_float64(m):
    """m = 1: the smallest orr_ppo_head accepts; 1000: no multiple of the 256 rows of a workgroup (nor of a wave); 4096: several workgroups"""
    import torch
    from openroborl_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(m)
    mean, target = torch.randn(m, 12, device=dev, generator=g), torch.randn(m, 12, device=dev, generator=g) * 1.5
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    runs = []
    for _ in range(2):
        gm, gb, stats = torch.full((m + 4, 12), SENTINEL, device=dev), torch.full((16,), SENTINEL, device=dev), torch.full((4,), SENTINEL, device=dev)
        ws = torch.empty(int(L.orr_learner_workspace_floats(m, 16)), device=dev)
        _lib.check(L.orr_distill_head(mean.data_ptr(), target.data_ptr(), m, gm.data_ptr(), gb.data_ptr(), stats.data_ptr(), ws.data_ptr(), st), L)
        torch.cuda.synchronize()
        assert bool((gm[m:] == SENTINEL).all()) and bool((gb[12:] == SENTINEL).all()) and bool((stats[1:] == SENTINEL).all())
        runs.append((gm[:m].clone(), gb[:12].clone(), stats[:1].clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                     # fixed summation order: the same bits every time
    gm, gb, stats = runs[0]
    mu64 = mean.double().requires_grad_(True)
    loss64 = ((mu64 - target.double()) ** 2).sum(dim=1).mean()
    loss64.backward()
    scale = mu64.grad.abs().max().item()
    print("m = %d: g_mean error %.2e of its scale, loss error %.2e" % (m, (gm.double() - mu64.grad).abs().max().item() / scale, abs(stats[0].item() - loss64.item())))
    assert (gm.double() - mu64.grad).abs().max().item() < 2e-5 * scale
    assert (gb.double() - mu64.grad.sum(dim=0)).abs().max().item() < 2e-5 * scale * math.sqrt(m)
    assert abs(stats[0].item() - loss64.item()) < 2e-5 * max(1.0, abs(loss64.item()))


# ---- f, i. the distillation learner ---------------------------------------------------------------------------------------------------
_DATA = {}


def distill_data(dev, B):
    """obs [B,160] and the labels of a teacher (seed 7, actor outputs of O(1)) on them and on random privileged rows; computed once per B"""
    import torch
    if B not in _DATA:
        g = torch.Generator().manual_seed(B)
        obs, priv = torch.randn(B, 160, generator=g).to(dev), torch.randn(B, 48, generator=g).to(dev)
        with torch.no_grad():
            _DATA[B] = (obs, teacher_model(dev, 7).mean(obs, priv).contiguous())
    return _DATA[B]


@pytest.mark.parametrize("graph,B,M", [(True, 512, 256), (False, 512, 256), (True, 8192, 4096)])
def test_fused_distill_matches_the_torch_learner(graph, B, M):
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    lr = 1e-4
    obs, target = distill_data(dev, B)
    finals = []
    for rep in range(2):
        ref_model, model = ppo.ActorCritic(dev, seed=2), ppo.ActorCritic(dev, seed=2)
        before = {k: v.detach().clone() for k, v in model.p.items()}
        ref = ppo.Distill(ref_model, lr=lr, minibatch=M)
        fused = learner_hip.FusedDistill(model, lr=lr, minibatch=M, use_graph=graph)
        for k in before:
            assert torch.equal(model.p[k].detach(), before[k])       # re-homing the actor in the flat buffer keeps the values
        P = fused._plan(B, M)
        if M >= 4096:
            assert tuple(P["part0"].shape) == (16, 160, 512) and P["n_jobs"] == 5
        else:
            assert P["part0"] is None and P["n_jobs"] == 3
        steps = 2 * 2 * (B // M)
        for it in range(2):
            g1, g2 = torch.Generator(device=dev), torch.Generator(device=dev)
            g1.manual_seed(10 + it); g2.manual_seed(10 + it)
            s_ref = ref.update(obs, target, epochs=2, generator=g1)
            s_fused = fused.update(obs, target, epochs=2, generator=g2)
            print("losses: fused %.7f torch %.7f" % (s_fused, s_ref))
            np.testing.assert_allclose(s_fused, s_ref, rtol=2e-4, atol=2e-5)
        assert fused.steps_taken() == steps                          # the capture's warm-up steps were undone
        moved = 0.0
        for k in sorted(before):
            a, b = ref_model.p[k].detach(), model.p[k].detach()
            if not k.startswith("model/pi"):                         # the critic: untouched by both, bit for bit
                assert torch.equal(b, before[k]) and torch.equal(a, before[k]), k
                continue
            moved = max(moved, (b - before[k]).abs().max().item())
            assert (a - b).abs().max().item() < 0.02 * steps * lr, (k, (a - b).abs().max().item())
            assert (a - b).abs().mean().item() < 2e-3 * steps * lr, (k, (a - b).abs().mean().item())
        assert moved > 2 * lr
        assert fused.total == sum((v.numel() + 3) // 4 * 4 for k, v in model.p.items() if k.startswith("model/pi"))      # no critic slots, no critic moments
        finals.append(fused.flat_p.clone())
        if rep == 0:
            with pytest.raises(ValueError):
                fused.update(obs[:B - 1], target[:B - 1])
            with pytest.raises(ValueError):
                learner_hip.FusedDistill(ppo.ActorCritic(dev, seed=2, priv_dim=48, actor_priv_dim=48))
    assert torch.equal(finals[0], finals[1])                         # two identical runs: the same bits


def test_distillation_learns_and_follows_the_torch_trajectory():
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    B = 512
    obs, target = distill_data(dev, B)
    ref_model, model = ppo.ActorCritic(dev, seed=11), ppo.ActorCritic(dev, seed=11)        # (the teacher's seed is 7)
    ref, fused = ppo.Distill(ref_model, lr=1e-4, minibatch=B), learner_hip.FusedDistill(model, lr=1e-4, minibatch=B)
    g1, g2 = torch.Generator(device=dev).manual_seed(0), torch.Generator(device=dev).manual_seed(0)
    l_ref = [ref.update(obs, target, epochs=1, generator=g1) for _ in range(50)]
    l_fused = [fused.update(obs, target, epochs=1, generator=g2) for _ in range(50)]
    print("loss: first %.6f, last fused %.6f torch %.6f; largest relative difference %.2e"
          % (l_fused[0], l_fused[-1], l_ref[-1], max(abs(a - b) / abs(b) for a, b in zip(l_fused, l_ref))))
    np.testing.assert_allclose(l_fused, l_ref, rtol=2e-4, atol=2e-5)
    assert l_fused[-1] < l_fused[0]
    # the student's fused forward pass sees the trained weights
    model.enable_fused()
    with torch.no_grad():
        a, _, _ = model.act(obs[:64], deterministic=True)
        np.testing.assert_allclose(a.cpu().numpy(), model.mean(obs[:64]).clamp(-CLIP, CLIP).cpu().numpy(), atol=2e-5)


# ---- g. PPO with a privileged actor ---------------------------------------------------------------------------------------------------
def ppo_batch(dev, B, seed, model, margin=0.0):
    """tests/test_gpu_privileged.py's synthetic batch for a privileged actor.  margin > 0: only samples none of whose ACTOR pre-activations
    (float64) lies within `margin` of the ReLU's kink (see there)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    obs, priv = torch.randn(2 * B, 160, generator=g), torch.randn(2 * B, 48, generator=g)
    if margin > 0.0:
        p = {k: v.detach().cpu().double() for k, v in model.p.items()}
        z0 = torch.cat((obs, priv), dim=1).double() @ p["model/pi_fc0/w:0"] + p["model/pi_fc0/b:0"]
        z1 = torch.relu(z0) @ p["model/pi_fc1/w:0"] + p["model/pi_fc1/b:0"]
        keep = (z0.abs().min(dim=1).values > margin) & (z1.abs().min(dim=1).values > margin)
        assert int(keep.sum()) >= B
        obs, priv = obs[keep], priv[keep]
    obs, priv = obs[:B].to(dev), priv[:B].to(dev)
    with torch.no_grad():
        mu = model.mean(obs, priv)
    act = mu + 0.125 * torch.randn(B, 12, generator=g).to(dev)
    shifted = mu + 0.04 * torch.randn(B, 12, generator=g).to(dev)
    old = (-0.5 * ((act - shifted) ** 2) / 0.125 ** 2 - 0.5 * math.log(2.0 * math.pi * 0.125 ** 2)).sum(dim=1)
    adv = torch.randn(B, generator=g).to(dev)
    adv[::97] = 0.0
    ret = torch.randn(B, generator=g).to(dev)
    return obs, priv, act, old, adv, ret


@pytest.mark.parametrize("graph,B,M", [(True, 512, 256), (False, 512, 256), (True, 8192, 4096)])
def test_fused_ppo_with_a_privileged_actor_matches_the_torch_learner(graph, B, M):
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    lr = 1e-4
    ref_model, model = (ppo.ActorCritic(dev, seed=2, priv_dim=48, actor_priv_dim=48) for _ in range(2))
    obs, priv, act, old, adv, ret = ppo_batch(dev, B, 1, ref_model)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    ref = ppo.PPO(ref_model, lr=lr, minibatch=M)
    fused = learner_hip.FusedPPO(model, lr=lr, minibatch=M, use_graph=graph)
    P = fused._plan(B, M)
    assert tuple(P["xv"].shape) == (M, 208)
    if M >= 4096:
        assert tuple(P["part0_vf"].shape) == (16, 208, 512) and tuple(P["part0_pi"].shape) == (16, 208, 512)
        assert P["n_jobs"] == 10 and P["jobs"][9].cols == 208 * 512 and P["jobs"][7].cols == 208 * 512
    steps = 2 * 2 * (B // M)
    for it in range(2):
        g1, g2 = torch.Generator(device=dev), torch.Generator(device=dev)
        g1.manual_seed(10 + it); g2.manual_seed(10 + it)
        s_ref = ref.update(obs, act, adv, ret, old_logp=old, epochs=2, generator=g1, priv=priv)
        s_fused = fused.update(obs, act, adv, ret, old_logp=old, epochs=2, generator=g2, priv=priv)
        np.testing.assert_allclose(s_fused, s_ref, rtol=2e-4, atol=2e-5)
    assert fused.steps_taken() == steps
    moved = 0.0
    for k in sorted(before):
        a, b = ref_model.p[k].detach(), model.p[k].detach()
        moved = max(moved, (a - before[k]).abs().max().item())
        assert (a - b).abs().max().item() < 0.02 * steps * lr, (k, (a - b).abs().max().item())
        assert (a - b).abs().mean().item() < 2e-3 * steps * lr, (k, (a - b).abs().mean().item())
    assert moved > 2 * lr
    assert float((model.p["model/pi_fc0/w:0"].detach()[160:] - before["model/pi_fc0/w:0"][160:]).abs().max()) > 0.5 * lr   # the privileged rows train
    # without old_logp both learners compute it with the vector; the fused forward pass sees the updated weights
    s_ref = ref.update(obs, act, adv, ret, generator=torch.Generator(device=dev).manual_seed(3), priv=priv)
    s_fused = fused.update(obs, act, adv, ret, generator=torch.Generator(device=dev).manual_seed(3), priv=priv)
    np.testing.assert_allclose(s_fused, s_ref, rtol=2e-4, atol=2e-5)
    model.enable_fused()
    with torch.no_grad():
        a_fused, _, v_fused = model.act(obs[:256], priv[:256], deterministic=True)
        np.testing.assert_allclose(a_fused.cpu().numpy(), model.mean(obs[:256], priv[:256]).clamp(-CLIP, CLIP).cpu().numpy(), atol=2e-5)
        np.testing.assert_allclose(v_fused.cpu().numpy(), model.value(obs[:256], priv[:256]).cpu().numpy(), atol=2e-5)


@pytest.mark.parametrize("B", [256, 4096])
def test_fused_gradient_with_a_privileged_actor_matches_float64_cpu(B):
    """The gradient of model/pi_fc0/w:0 (208 rows) from the hand-written backward against float64 autograd; B = 4096: through part0_pi."""
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    model = ppo.ActorCritic(dev, seed=4, priv_dim=48, actor_priv_dim=48)
    with torch.no_grad():
        model.p["model/pi/w:0"].mul_(30.0)
    obs, priv, act, old, adv, ret = ppo_batch(dev, B, 0, model, margin=1e-4)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.p.items()}
    mu64 = mlp64(p64, "pi", torch.cat((obs, priv), dim=1).cpu())
    logp = (-0.5 * ((act.cpu().double() - mu64) ** 2) / 0.125 ** 2 - 0.5 * math.log(2.0 * math.pi * 0.125 ** 2)).sum(dim=1)
    ratio = torch.exp(logp - old.cpu().double())
    surr64 = -torch.min(ratio * adv.cpu().double(), torch.clamp(ratio, 0.8, 1.2) * adv.cpu().double()).mean()
    surr64.backward()
    learner = learner_hip.FusedPPO(model, lr=1e-4, minibatch=B, use_graph=False)
    P = learner._plan(B, B)
    with torch.no_grad():
        P["obs"].copy_(obs)
        P["priv"].copy_(priv)
        P["aux"][:, :12], P["aux"][:, 12], P["aux"][:, 13], P["aux"][:, 14] = act, old, adv, ret
        P["perm"].copy_(torch.arange(B, device=dev))
        learner._minibatch(P, 0)
    assert abs(P["stats"][0, 0].item() - surr64.item()) < 2e-4 * max(1.0, abs(surr64.item()))
    for k in ("model/pi_fc0/w:0", "model/pi_fc0/b:0", "model/pi_fc1/w:0", "model/pi/w:0"):
        g32, g64 = learner.g[k].detach().cpu().double(), p64[k].grad
        scale = g64.abs().max().item() + 1e-12
        print("%s: gradient error %.2e of its scale" % (k, (g32 - g64).abs().max().item() / scale))
        assert (g32 - g64).abs().max().item() < 2e-3 * scale, (k, (g32 - g64).abs().max().item(), scale)
        cs = (g32 * g64).sum() / (g32.norm() * g64.norm() + 1e-30)
        assert cs.item() > 0.99999, (k, cs.item())
    assert float(p64["model/pi_fc0/w:0"].grad[160:].abs().max()) > 0.0 and float(learner.g["model/pi_fc0/w:0"][160:].abs().max()) > 0.0


# ---- h. the rollout -------------------------------------------------------------------------------------------------------------------
def test_graph_rollout_with_a_teacher():
    """The eager first segment and the replayed ones equal collect_rollout on a twin env with the same noise and mask; teacher_mean[k] is the
    teacher's own forward pass on (obs[k], priv[k]); a third twin stepped with the expected per-robot actions ends in the same state."""
    import torch
    from openroborl_amd import ppo, rollout
    dev = torch.device("cuda:0")
    n, T = 64, 4
    kw = dict(seed=11, auto_reset=True, contact_outputs=True, push=PUSH, push_outputs=True, config_overrides=short_episodes())
    envs = [mixed_env(n, **kw) for _ in range(3)]
    students = [ppo.ActorCritic(dev, seed=1).enable_fused() for _ in range(2)]
    teachers = [teacher_model(dev, 5).enable_fused() for _ in range(3)]
    collector = rollout.GraphRollout(envs[1], students[1], T, teacher=teachers[1])
    assert collector.priv_dim == 0 and tuple(collector.priv.shape) == (T + 1, n, 48) and not bool(collector.teacher_mask.any())
    obs = [e.reset() for e in envs]
    priv = [None, None]
    gen = torch.Generator(device=dev).manual_seed(0)
    half = torch.zeros(n, dtype=torch.uint8, device=dev)
    half[::2] = 1
    masks = [torch.zeros_like(half), half, 1 - half]              # segment 0 eager, 1 captured, 2 replayed with the mask flipped in place
    ended = 0
    for seg in range(3):
        noise = torch.randn(T, n, 12, device=dev, generator=gen)
        collector.teacher_mask.copy_(masks[seg])                     # in place: no new capture
        graph_before = collector.graph
        a = rollout.collect_rollout(envs[0], students[0], T, obs=obs[0], noise=noise, priv=priv[0], teacher=teachers[0], teacher_mask=masks[seg])
        b = collector.collect(obs[1], noise=noise, priv=priv[1])
        if seg == 2:
            assert collector.graph is graph_before and graph_before is not None
        for k in ("obs", "actions", "rewards", "dones", "vpred", "last_obs", "priv", "last_priv", "teacher_mean"):
            assert torch.equal(a[k], b[k]), (seg, k)
        assert tuple(b["teacher_mean"].shape) == (T, n, 12) and tuple(b["priv"].shape) == (T, n, 48)
        m = masks[seg].bool()[:, None]
        for k in range(T):
            # the teacher's own forward pass on the recorded inputs, and the student's raw sample in "actions" whoever drove
            want_a, _, _, want_m = teachers[2].fused.forward(b["obs"][k].contiguous(), None, priv=b["priv"][k].contiguous(), want_mean=True)
            assert torch.equal(want_m, b["teacher_mean"][k]), (seg, k)
            s_clip, s_raw, _ = students[0].act(b["obs"][k].contiguous(), noise=noise[k])
            assert torch.equal(s_raw, b["actions"][k]), (seg, k)
            # the third twin: the teacher's clipped mean for the masked robots, the student's clipped sample for the others
            _, _, done, _ = envs[2].step(torch.where(m, want_a, s_clip).contiguous())
            want_p = envs[2].privileged_obs(done=done)
            assert torch.equal(want_p, b["priv"][k + 1] if k + 1 < T else b["last_priv"]), (seg, k)
        if seg > 0:
            assert float((b["teacher_mean"] - b["actions"]).abs().max()) > 1e-2       # (the two policies do differ)
        ended += int(b["dones"].sum())
        obs = [a["last_obs"], b["last_obs"]]
        priv = [a["last_priv"].clone(), b["last_priv"]]
        with torch.no_grad():                       # "the learner" moves the student's weights, and somebody the teachers'; all are told so
            for mdl in students + teachers:
                for k2 in sorted(mdl.p):
                    mdl.p[k2].mul_(1.01)
                mdl.mark_updated()
            teachers[2].fused.refresh()
    assert collector.graph is not None and ended >= 1
    assert torch.equal(envs[0].state.view(torch.int32), envs[1].state.view(torch.int32))
    assert torch.equal(envs[0].state.view(torch.int32), envs[2].state.view(torch.int32))
    with pytest.raises(ValueError):
        rollout.collect_rollout(envs[0], students[0], 1, obs=obs[0], teacher_mask=half)
    for e in envs:
        e.close()


# ---- j. train.py ----------------------------------------------------------------------------------------------------------------------
def test_train_a_teacher_distill_a_student_and_evaluate_both(tmp_path):
    from openroborl_amd import policy as pol
    teacher_zip, student_zip, log_path = str(tmp_path / "teacher.zip"), str(tmp_path / "student.zip"), str(tmp_path / "log.json")
    common = ["--num-robot", "64", "--horizon", "8", "--iters", "2", "--push", "0.05,0.2,0.5"]

    def run(*argv):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + list(argv), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        return r.stdout.decode()
    run("--privileged-actor", "--save", teacher_zip, *common)
    w = pol.load_parameters(teacher_zip)
    assert w["model/pi_fc0/w:0"].shape == (208, 512) and w["model/vf_fc0/w:0"].shape == (208, 512)
    run("--distill", teacher_zip, "--distill-beta", "0.5", "--distill-beta-iters", "2", "--save", student_zip, "--log", log_path, *common)
    log = json.load(open(log_path))
    assert log and log[-1]["iter"] == 1 and log[0]["teacher_driven"] == 32 and log[-1]["teacher_driven"] == 16
    for rec in log:
        assert math.isfinite(rec["distill_loss"]) and rec["distill_loss"] > 0.0 and math.isfinite(rec["mean_step_reward"])
    w = pol.load_parameters(student_zip)
    for name, shape in pol.SB_PARAMETER_LIST:
        assert w[name].shape == shape, name
    assert w["model/pi_fc0/w:0"].shape == (160, 512)
    for z in (teacher_zip, student_zip):
        rec = json.loads(run("--eval", z, "--num-robot", "16").strip().splitlines()[-1])
        assert rec["robots"] == 16 and math.isfinite(rec["return_mean"])
