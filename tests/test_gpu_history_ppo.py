"""PPO on a history policy on the device (run with -m gpu on an MI355X):

  a. orr_policy_forward_history_priv: the actor's outputs are orr_policy_forward_history's and the value orr_policy_forward_teacher's, bit for
     bit; value = NULL, latent = NULL; the critic really reads priv; the refusals;
  b. orr_latent_backward against float64 on the CPU, its column sums and loss share through orr_colsum_finish, its bitwise properties, its refusals;
  c. learner_hip.FusedPPOHistory against ppo.PPOHistory and against float64 autograd, eager against graph replay, a learn-std model;
  d. rollout.GraphRollout(critic_priv=True) against rollout.collect_rollout(critic_priv=True), and critic_priv=False against today's segment;
  e. train.py --history-ppo in child processes, from scratch and from the zip it saved, and --eval of the result.

Tolerances.  a: none, bits.  b: derived, no measured one: with u = 2^-24, |g_z - float64| <= 520 u (|g0| |W0z|^T + |latent term|) element by
element (the 512-term dot-product bound for any summation order, and a few roundings of the latent term); a sum of m terms within
m u sum|terms|.  c: those of tests/test_gpu_teacher.py (losses rtol 2e-4 / atol 2e-5, parameters 0.02 steps lr at most and 2e-3 steps lr on
average; gradients 2e-3 of their scale and a cosine above 0.99999)."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.gpu_kit import mixed_env, short_episodes
from tests.test_gpu_history import ENC, enc64, hinputs, raw_history, stream, student_model
from tests.test_gpu_teacher import CLIP, PUSH, SENTINEL, mlp64, raw_forward

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 5
SIZES = [1, 15, 16, 17, 33]           # one row; a workgroup's edge on both sides; a third workgroup
U = 2.0 ** -24


# ---- a. the forward pass --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hnets():
    import torch
    from openroborl_amd import policy_hip
    dev = torch.device("cuda", 0)
    model = student_model(dev, 3)
    return model, policy_hip.FusedActorCritic(model.p, dev, std=0.125)


def raw_history_priv(fused, obs, hist, priv, noise, n, value=True, latent=True, guard=16):
    """orr_policy_forward_history_priv with the test's own output buffers: n rows + a guard band in each"""
    import torch
    dev = obs.device
    outs = [torch.full((n + guard, c), SENTINEL, device=dev) for c in (12, 12, 1, 12, 48)]      # action, raw, value, mean, latent
    rc = fused.L.orr_policy_forward_history_priv(C.byref(fused.net), C.byref(fused.enc), obs.data_ptr(), hist.data_ptr(),
                                                 priv.data_ptr() if priv is not None else None, n, noise.data_ptr(), 0.125, CLIP, outs[0].data_ptr(),
                                                 outs[1].data_ptr(), outs[2].data_ptr() if value else None, outs[3].data_ptr(),
                                                 outs[4].data_ptr() if latent else None, stream(dev))
    assert rc == 0, fused.L.orr_last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o[n:] == SENTINEL).all())                      # rows beyond n are not written
    if not value:
        assert bool((outs[2] == SENTINEL).all())
    if not latent:
        assert bool((outs[4] == SENTINEL).all())
    return [o[:n] for o in outs]


@pytest.mark.parametrize("n", SIZES)
def test_forward_history_priv_is_the_history_kernels_actor_and_the_teacher_kernels_critic(hnets, n):
    import torch
    model, fused = hnets
    dev = model.device
    obs, hist, noise = hinputs(dev, n, 200 + n)
    priv = torch.randn(n, 48, device=dev, generator=torch.Generator(device=dev).manual_seed(300 + n)) * 2.0
    act, raw, val, mean, latent = raw_history_priv(fused, obs, hist, priv, noise, n)
    act_h, raw_h, val_h, mean_h, latent_h = raw_history(fused, obs, hist, noise, n)
    assert torch.equal(act, act_h) and torch.equal(raw, raw_h) and torch.equal(mean, mean_h) and torch.equal(latent, latent_h)
    val_t = raw_forward(fused, "teacher", obs, priv, noise, n)[2]
    assert torch.equal(val, val_t)
    # the critic really reads priv: its value is not the history kernel's (whose critic reads z), and it is float64's on obs | priv
    assert float((priv - latent).abs().max()) > 0.1 and float((val - val_h).abs().max()) > 1e-3
    v64 = mlp64(model.p, "vf", torch.cat((obs, priv), dim=1)).detach()[:, 0]
    assert float((val[:, 0].double() - v64).abs().max()) < 2e-5 * max(1.0, float(v64.abs().max()))
    # with priv = z it IS the history kernel's value
    assert torch.equal(raw_history_priv(fused, obs, hist, latent.contiguous(), noise, n)[2], val_h)
    # no value buffer (priv may then be NULL), no latent buffer: no other output bit changes
    for p in (priv, None):
        a1, r1, _, m1, z1 = raw_history_priv(fused, obs, hist, p, noise, n, value=False)
        assert torch.equal(a1, act) and torch.equal(r1, raw) and torch.equal(m1, mean) and torch.equal(z1, latent)
    a2, r2, v2, m2, _ = raw_history_priv(fused, obs, hist, priv, noise, n, latent=False)
    assert torch.equal(a2, act) and torch.equal(r2, raw) and torch.equal(m2, mean) and torch.equal(v2, val)
    # through the Python layers: the same numbers
    out_latent = torch.full((n, 48), SENTINEL, device=dev)
    a3, r3, v3, m3 = fused.forward(obs, noise, want_mean=True, hist=hist, critic_priv=priv, out_latent=out_latent)
    assert torch.equal(a3, act) and torch.equal(r3, raw) and torch.equal(v3, val[:, 0]) and torch.equal(m3, mean) and torch.equal(out_latent, latent)
    for bad in (lambda: fused.forward(obs, noise, critic_priv=priv), lambda: fused.forward(obs, noise, priv=priv, critic_priv=priv),
                lambda: fused.forward(obs, noise, hist=hist, critic_priv=priv[:, :47].contiguous()),
                lambda: fused.forward(obs, noise, hist=hist, critic_priv=priv.double())):
        with pytest.raises(ValueError):
            bad()


def test_act_with_critic_priv_runs_the_fused_kernel_and_matches_torch():
    import torch
    dev = torch.device("cuda:0")
    model = student_model(dev, 4)
    obs, hist, noise = hinputs(dev, 40, 9)
    priv = torch.randn(40, 48, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    with torch.no_grad():
        a0, r0, v0 = model.act(obs, hist=hist, critic_priv=priv, noise=noise)          # plain torch
        assert torch.equal(v0, model.value(obs, priv))
    model.enable_fused()
    a1, r1, v1 = model.act(obs, hist=hist, critic_priv=priv, noise=noise)
    for a, b in ((a1, a0), (r1, r0), (v1, v0)):
        assert float((a - b).abs().max()) < 2e-5 * max(1.0, float(b.abs().max()))
    assert torch.equal(model.act(obs, hist=hist, noise=noise)[1], r1)                   # the actor is the history kernel's
    for bad in (lambda: model.act(obs, critic_priv=priv), lambda: model.act(obs, hist=hist, critic_priv=priv[:39])):
        with pytest.raises(ValueError):
            bad()


def test_forward_history_priv_refusals_write_nothing(hnets):
    import torch
    from openroborl_amd import _abi
    model, fused = hnets
    dev, n = model.device, 5
    L = fused.L
    obs, hist, noise = hinputs(dev, n + 1, 7)
    priv = torch.randn(n + 1, 48, device=dev)
    outs = [torch.full((n + 1, c), SENTINEL, device=dev) for c in (12, 12, 1, 12, 48)]

    def call(net=None, enc=None, obs_p=obs.data_ptr(), hist_p=hist.data_ptr(), priv_p=priv.data_ptr(), count=n, action_p=outs[0].data_ptr(),
             value_p=outs[2].data_ptr(), latent_p=outs[4].data_ptr()):
        return L.orr_policy_forward_history_priv(C.byref(fused.net) if net is None else net, C.byref(fused.enc) if enc is None else enc, obs_p, hist_p,
                                                 priv_p, count, noise.data_ptr(), 0.125, CLIP, action_p, outs[1].data_ptr(), value_p, outs[3].data_ptr(),
                                                 latent_p, stream(dev))
    no_member, odd = _abi.OrrPolicyNet(), _abi.OrrPolicyNet()
    enc_null, enc_odd = _abi.OrrHistoryEncoder(), _abi.OrrHistoryEncoder()
    for dst, src in ((no_member, fused.net), (odd, fused.net), (enc_null, fused.enc), (enc_odd, fused.enc)):
        C.memmove(C.byref(dst), C.byref(src), C.sizeof(src))
    no_member.b1_vf = None
    odd.w0_pi = fused.net.w0_pi + 4
    enc_null.b1 = None
    enc_odd.w1 = fused.enc.w1 + 8
    for kw, text in ((dict(net=C.POINTER(_abi.OrrPolicyNet)()), b"bad argument"), (dict(enc=C.POINTER(_abi.OrrHistoryEncoder)()), b"bad argument"),
                     (dict(obs_p=None), b"bad argument"), (dict(hist_p=None), b"bad argument"), (dict(action_p=None), b"bad argument"),
                     (dict(count=0), b"bad argument"), (dict(count=-3), b"bad argument"), (dict(priv_p=None), b"bad argument"),
                     (dict(net=C.byref(no_member)), b"null pointer"), (dict(net=C.byref(odd)), b"16-byte aligned"),
                     (dict(enc=C.byref(enc_null)), b"orr_history_encoder has a null pointer"), (dict(enc=C.byref(enc_odd)), b"16-byte aligned"),
                     (dict(hist_p=hist.data_ptr() + 4), b"hist must be 16-byte aligned"), (dict(obs_p=obs.data_ptr() + 2), b"4-byte aligned"),
                     (dict(priv_p=priv.data_ptr() + 2), b"4-byte aligned"), (dict(value_p=outs[2].data_ptr() + 1), b"4-byte aligned"),
                     (dict(latent_p=outs[4].data_ptr() + 2), b"4-byte aligned")):
        rc = call(**kw)
        assert rc < 0 and text in L.orr_last_error() and b"orr_policy_forward_history_priv" in L.orr_last_error(), (kw, rc, L.orr_last_error())
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == SENTINEL).all())
    assert call() == 0                                               # and the same call with everything in place
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o[:n] != SENTINEL).all()) and bool((o[n:] == SENTINEL).all())


# ---- b. orr_latent_backward -----------------------------------------------------------------------------------------------------------
class Latent(object):
    """W0z [48][512] (rows 160..207 of an actor's layer 0), its packed transpose, and inputs for the largest size + GUARD rows; the float64
    reference lives on the CPU"""

    def __init__(self):
        import torch
        from openroborl_amd import _lib
        self.dev = torch.device("cuda", 0)
        self.L = L = _lib.load()
        g = torch.Generator().manual_seed(77)
        rows = max(SIZES) + GUARD
        self.w0z = torch.randn(48, 512, generator=g) / math.sqrt(208.0)
        self.g0 = torch.randn(rows, 512, generator=g) * (torch.rand(rows, 512, generator=g) < 0.5)      # a masked gradient: half of it zeros
        self.z, self.tp = torch.randn(rows, 48, generator=g) * 2.0, torch.randn(rows, 48, generator=g) * 2.0
        w0zt = self.w0z.t().contiguous().to(self.dev)
        self.packed = torch.empty(int(L.orr_policy_packed_size(512, 48)), device=self.dev)
        assert L.orr_policy_pack(w0zt.data_ptr(), 512, 48, self.packed.data_ptr(), stream(self.dev)) == 0
        self.d = [x.to(self.dev) for x in (self.g0, self.z, self.tp)]
        torch.cuda.synchronize()

    def run(self, m, coef, null=False):
        """orr_latent_backward on the first m rows with the test's own outputs, GUARD sentinel rows behind each; the partials folded by
        orr_colsum_finish as two jobs.  -> g_z [m,48], gb [48], loss [1], partials"""
        import torch
        from openroborl_amd import _abi
        L, dev = self.L, self.dev
        rows = _abi.latent_backward_rows(m)
        g_z = torch.full((m + GUARD, 48), SENTINEL, device=dev)
        part = torch.full((49 * rows + 49 * GUARD,), SENTINEL, device=dev)
        g0, z, tp = self.d
        rc = L.orr_latent_backward(g0.data_ptr(), self.packed.data_ptr(), None if null else z.data_ptr(), None if null else tp.data_ptr(), m, coef,
                                   g_z.data_ptr(), part.data_ptr(), stream(dev))
        assert rc == 0, L.orr_last_error()
        gb, loss = torch.full((48 + GUARD,), SENTINEL, device=dev), torch.full((1 + GUARD,), SENTINEL, device=dev)
        jobs = (_abi.OrrColsumJob * 2)(_abi.OrrColsumJob(part.data_ptr(), gb.data_ptr(), rows, 48),
                                       _abi.OrrColsumJob(part.data_ptr() + 4 * 48 * rows, loss.data_ptr(), rows, 1))
        assert L.orr_colsum_finish(jobs, 2, stream(dev)) == 0, L.orr_last_error()
        torch.cuda.synchronize()
        for o, n in ((g_z, m), (part, 49 * rows), (gb, 48), (loss, 1)):
            assert bool((o[n:] == SENTINEL).all())                   # nothing behind the outputs is written
            assert bool(torch.isfinite(o[:n]).all()) and bool((o[:n] != SENTINEL).all())
        return g_z[:m].clone(), gb[:48].clone(), loss[:1].clone(), part[:49 * rows].clone()


@pytest.fixture(scope="module")
def lat():
    return Latent()


@pytest.mark.parametrize("coef", [0.0, 0.5])
@pytest.mark.parametrize("m", SIZES)
def test_latent_backward_matches_float64_within_the_dot_product_bound(lat, m, coef):
    import torch
    g_z, gb, loss, _ = lat.run(m, coef)
    g0, z, tp, w = lat.g0[:m].double(), lat.z[:m].double(), lat.tp[:m].double(), lat.w0z.double()
    term = coef * 2.0 * (z - tp) / m
    want = g0 @ w.t() + term
    bound = 520.0 * U * (g0.abs() @ w.abs().t() + term.abs())
    err = (g_z.cpu().double() - want).abs()
    print("m = %d, coefficient %g: largest error %.2e of its bound, largest |g_z| %.3f" % (m, coef, float((err / bound).max()), float(want.abs().max())))
    assert bool((err <= bound).all())
    assert float(want.abs().max()) > 1.0 and float(term.abs().max()) > (0.01 / m if coef else -1.0)
    # the column sums: m terms per column, whatever the order
    g64 = g_z.cpu().double()
    err_b = (gb.cpu().double() - g64.sum(dim=0)).abs()
    assert bool((err_b <= m * U * g64.abs().sum(dim=0)).all()), float((err_b / (m * U * g64.abs().sum(dim=0))).max())
    # the loss: (1 / m) sum_i sum_c (z - target)^2, or 0 without a coefficient (z and target_priv are not read then)
    l64 = float(((z - tp) ** 2).sum() / m) if coef else 0.0
    print("m = %d, coefficient %g: loss %.7f, float64 %.7f, bound %.2e" % (m, coef, loss.item(), l64, m * U * l64))
    assert abs(loss.item() - l64) <= m * U * l64
    assert (l64 > 10.0) == bool(coef)


@pytest.mark.parametrize("m", SIZES)
def test_latent_backward_bitwise_properties(lat, m):
    import torch
    for coef in (0.0, 0.5):
        a, b = lat.run(m, coef), lat.run(m, coef)                    # two runs: equal bits everywhere
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    g0_ = lat.run(m, 0.0)
    null = lat.run(m, 0.0, null=True)                                # coefficient 0: NULL z / target_priv give the bits of non-NULL ones
    for x, y in zip(g0_, null):
        assert torch.equal(x, y)
    assert float(g0_[2].item()) == 0.0
    big = lat.run(max(SIZES), 0.0)[0]                                # coefficient 0: a row is the same for every m that contains it
    assert torch.equal(big[:m], g0_[0])
    assert not torch.equal(lat.run(m, 0.5)[0], g0_[0])               # (and the coefficient does reach g_z)


def test_latent_backward_refusals_write_nothing(lat):
    import torch
    dev, L, m = lat.dev, lat.L, 5
    g0, z, tp = lat.d
    outs = [torch.full((m + 1, c), SENTINEL, device=dev) for c in (48, 49)]          # g_z, partials

    def call(g0_p=g0.data_ptr(), w_p=lat.packed.data_ptr(), z_p=z.data_ptr(), tp_p=tp.data_ptr(), count=m, coef=0.5, g_p=outs[0].data_ptr(),
             part_p=outs[1].data_ptr()):
        return L.orr_latent_backward(g0_p, w_p, z_p, tp_p, count, coef, g_p, part_p, stream(dev))
    for kw, text in ((dict(g0_p=None), b"bad argument"), (dict(w_p=None), b"bad argument"), (dict(z_p=None), b"bad argument"),
                     (dict(tp_p=None), b"bad argument"), (dict(g_p=None), b"bad argument"), (dict(part_p=None), b"bad argument"),
                     (dict(count=0), b"bad argument"), (dict(count=-3), b"bad argument"), (dict(w_p=lat.packed.data_ptr() + 4), b"16-byte aligned"),
                     (dict(w_p=lat.packed.data_ptr() + 8), b"16-byte aligned"), (dict(g0_p=g0.data_ptr() + 2), b"4-byte aligned"),
                     (dict(z_p=z.data_ptr() + 1), b"4-byte aligned"), (dict(tp_p=tp.data_ptr() + 3), b"4-byte aligned"),
                     (dict(g_p=outs[0].data_ptr() + 2), b"4-byte aligned"), (dict(part_p=outs[1].data_ptr() + 2), b"4-byte aligned")):
        rc = call(**kw)
        assert rc < 0 and text in L.orr_last_error() and b"orr_latent_backward" in L.orr_last_error(), (kw, rc, L.orr_last_error())
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == SENTINEL).all())
    assert call() == 0                                               # and the same call with everything in place
    torch.cuda.synchronize()
    assert bool((outs[0][:m] != SENTINEL).all()) and bool((outs[1].view(-1)[:49] != SENTINEL).all())
    assert bool((outs[0][m:] == SENTINEL).all()) and bool((outs[1].view(-1)[49:] == SENTINEL).all())


# ---- c. the learner -------------------------------------------------------------------------------------------------------------------
def history_batch(dev, B, seed, model, margin=0.0):
    """tests/test_gpu_teacher.py's synthetic PPO batch with a history.  margin > 0: only samples none of whose pre-activations on the way from
    the history to the actor's output (the encoder's hidden layer, the actor's two; float64) lies within `margin` of the ReLU's kink."""
    import torch
    g = torch.Generator().manual_seed(seed)
    obs, hist, priv = torch.randn(2 * B, 160, generator=g), torch.randn(2 * B, 512, generator=g), torch.randn(2 * B, 48, generator=g)
    if margin > 0.0:
        p = {k: v.detach().cpu().double() for k, v in model.p.items()}
        e0 = hist.double() @ p["model/enc_fc0/w:0"] + p["model/enc_fc0/b:0"]
        z = torch.relu(e0) @ p["model/enc_fc1/w:0"] + p["model/enc_fc1/b:0"]
        z0 = torch.cat((obs.double(), z), dim=1) @ p["model/pi_fc0/w:0"] + p["model/pi_fc0/b:0"]
        z1 = torch.relu(z0) @ p["model/pi_fc1/w:0"] + p["model/pi_fc1/b:0"]
        keep = (e0.abs().min(dim=1).values > margin) & (z0.abs().min(dim=1).values > margin) & (z1.abs().min(dim=1).values > margin)
        assert int(keep.sum()) >= B
        obs, hist, priv = obs[keep], hist[keep], priv[keep]
    obs, hist, priv = obs[:B].to(dev), hist[:B].to(dev), priv[:B].to(dev)
    with torch.no_grad():
        mu = model.mean(obs, hist=hist)
    act = mu + 0.125 * torch.randn(B, 12, generator=g).to(dev)
    shifted = mu + 0.04 * torch.randn(B, 12, generator=g).to(dev)
    old = (-0.5 * ((act - shifted) ** 2) / 0.125 ** 2 - 0.5 * math.log(2.0 * math.pi * 0.125 ** 2)).sum(dim=1)
    adv = torch.randn(B, generator=g).to(dev)
    adv[::97] = 0.0
    ret = torch.randn(B, generator=g).to(dev)
    return obs, hist, priv, act, old, adv, ret


def history_policy(dev, seed, **kw):
    from openroborl_amd import ppo
    return ppo.ActorCritic(dev, seed=seed, priv_dim=48, actor_priv_dim=48, history=16, **kw)


@pytest.mark.parametrize("graph,B,M", [(True, 512, 256), (False, 512, 256), (True, 8192, 4096)])
def test_fused_ppo_history_matches_the_torch_learner(graph, B, M):
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    lr, coef = 1e-4, (0.5 if graph else 0.0)                         # the eager case also takes the path without a latent loss
    ref_model, model = (history_policy(dev, 2) for _ in range(2))
    obs, hist, priv, act, old, adv, ret = history_batch(dev, B, 1, ref_model)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    ref = ppo.PPOHistory(ref_model, lr=lr, minibatch=M, latent_coef=coef)
    fused = learner_hip.FusedPPOHistory(model, lr=lr, minibatch=M, use_graph=graph, latent_coef=coef)
    assert isinstance(fused, learner_hip.FusedPPO) and set(fused.slots) == set(before) and len(before) == 16
    P = fused._plan(B, M)
    assert tuple(P["xv"].shape) == (M, 208) and tuple(P["xz"].shape) == (M, 208) and tuple(P["stats"].shape) == (B // M, 3)
    if M >= 4096:                                                    # 10 + 4 column-sum jobs in two launches
        assert P["n_jobs"] == 10 and P["jobs_s"][0][1] == 4 and tuple(P["part0"].shape) == (16, 512, 256)
    else:
        assert P["n_jobs"] == 6 and P["jobs_s"][0][1] == (3 if coef else 2)
    steps = 2 * 2 * (B // M)
    for it in range(2):
        g1, g2 = torch.Generator(device=dev), torch.Generator(device=dev)
        g1.manual_seed(10 + it); g2.manual_seed(10 + it)
        s_ref = ref.update(obs, hist, priv, act, adv, ret, old_logp=old, epochs=2, generator=g1)
        s_fused = fused.update(obs, hist, priv, act, adv, ret, old_logp=old, epochs=2, generator=g2)
        assert len(s_fused) == 3 and s_ref[2] > 1.0                  # the latent loss is reported whatever its coefficient
        np.testing.assert_allclose(s_fused, s_ref, rtol=2e-4, atol=2e-5)
    assert fused.steps_taken() == steps
    moved = 0.0
    for k in sorted(before):
        a, b = ref_model.p[k].detach(), model.p[k].detach()
        moved = max(moved, (a - before[k]).abs().max().item())
        assert (a - b).abs().max().item() < 0.02 * steps * lr, (k, (a - b).abs().max().item())
        assert (a - b).abs().mean().item() < 2e-3 * steps * lr, (k, (a - b).abs().mean().item())
    assert moved > 2 * lr
    for k in ENC:                                                    # the encoder trains, with or without the latent loss
        assert float((model.p[k].detach() - before[k]).abs().max()) > 0.5 * lr, k
    # without old_logp both learners compute it with the history; the fused forward pass sees the updated weights
    s_ref = ref.update(obs, hist, priv, act, adv, ret, generator=torch.Generator(device=dev).manual_seed(3))
    s_fused = fused.update(obs, hist, priv, act, adv, ret, generator=torch.Generator(device=dev).manual_seed(3))
    np.testing.assert_allclose(s_fused, s_ref, rtol=2e-4, atol=2e-5)
    model.enable_fused()
    with torch.no_grad():
        a_fused, _, v_fused = model.act(obs[:256], hist=hist[:256], critic_priv=priv[:256], deterministic=True)
        np.testing.assert_allclose(a_fused.cpu().numpy(), model.mean(obs[:256], hist=hist[:256]).clamp(-CLIP, CLIP).cpu().numpy(), atol=2e-5)
        np.testing.assert_allclose(v_fused.cpu().numpy(), model.value(obs[:256], priv[:256]).cpu().numpy(), atol=2e-5)


@pytest.mark.parametrize("B", [256, 4096])
def test_fused_history_gradients_match_float64_autograd(B):
    """The encoder's gradients and model/pi_fc0/w:0 of one minibatch against float64 autograd, with and without the latent loss; B = 4096:
    through the split weight gradients.  The batch is chosen by history_batch's margin rule from the float64 reference alone; no sample of it
    is left out of the comparison."""
    import torch
    from openroborl_amd import learner_hip
    dev = torch.device("cuda:0")
    model = history_policy(dev, 4)
    with torch.no_grad():
        model.p["model/pi/w:0"].mul_(30.0)
    obs, hist, priv, act, old, adv, ret = history_batch(dev, B, 0, model, margin=1e-4)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.p.items()}
    z64 = enc64(p64, hist.cpu())
    mu64 = mlp64(p64, "pi", torch.cat((obs.cpu().double(), z64), dim=1))
    logp = (-0.5 * ((act.cpu().double() - mu64) ** 2) / 0.125 ** 2 - 0.5 * math.log(2.0 * math.pi * 0.125 ** 2)).sum(dim=1)
    ratio = torch.exp(logp - old.cpu().double())
    surr64 = -torch.min(ratio * adv.cpu().double(), torch.clamp(ratio, 0.8, 1.2) * adv.cpu().double()).mean()
    lat64 = ((z64 - priv.cpu().double()) ** 2).sum(dim=1).mean()
    names = ("model/enc_fc0/w:0", "model/enc_fc1/w:0", "model/enc_fc1/b:0", "model/pi_fc0/w:0")
    for coef in (0.0, 0.5):
        want = torch.autograd.grad(surr64 + coef * lat64, [p64[k] for k in names], retain_graph=True)
        learner = learner_hip.FusedPPOHistory(model, lr=1e-4, minibatch=B, use_graph=False, latent_coef=coef)
        P = learner._plan(B, B)
        with torch.no_grad():
            P["obs"].copy_(obs)
            P["hist"].copy_(hist)
            P["priv"].copy_(priv)
            P["aux"][:, :12], P["aux"][:, 12], P["aux"][:, 13], P["aux"][:, 14] = act, old, adv, ret
            P["perm"].copy_(torch.arange(B, device=dev))
            learner._minibatch(P, 0)
        assert abs(P["stats"][0, 0].item() - surr64.item()) < 2e-4 * max(1.0, abs(surr64.item()))
        assert abs(P["stats"][0, 2].item() - lat64.item()) < 2e-4 * lat64.item()
        for k, g64 in zip(names, want):
            g32 = learner.g[k].detach().cpu().double()
            scale = g64.abs().max().item() + 1e-12
            cs = ((g32 * g64).sum() / (g32.norm() * g64.norm() + 1e-30)).item()
            print("B = %d, latent_coef %g, %s: gradient error %.2e of its scale, 1 - cosine %.2e" % (B, coef, k, (g32 - g64).abs().max().item() / scale, 1.0 - cs))
            assert (g32 - g64).abs().max().item() < 2e-3 * scale, (k, (g32 - g64).abs().max().item(), scale)
            assert cs > 0.99999, (k, cs)
            assert scale > 1e-6
    assert float(learner.g["model/pi_fc0/w:0"][160:].abs().max()) > 0.0


def test_eager_and_graph_replay_give_the_same_bits_and_a_learn_std_model_returns_six_stats():
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    B, M = 512, 256
    finals, stats = [], []
    for graph in (False, True):
        model = history_policy(dev, 6, learn_std=True)
        if not finals:
            data = history_batch(dev, B, 2, model)
        obs, hist, priv, act, old, adv, ret = data
        learner = learner_hip.FusedPPOHistory(model, lr=1e-4, minibatch=M, use_graph=graph, ent_coef=0.01, latent_coef=0.25)
        for it in range(2):
            s = learner.update(obs, hist, priv, act, adv, ret, old_logp=old, epochs=2, generator=torch.Generator(device=dev).manual_seed(it))
        assert len(s) == 6 and all(math.isfinite(float(x)) for x in s)
        finals.append(learner.flat_p.clone())
        stats.append(s)
    assert torch.equal(finals[0], finals[1]) and np.array_equal(stats[0], stats[1])
    # and the torch learner's six: ppo.STAT_NAMES' five and the latent loss
    ref_model = history_policy(dev, 6, learn_std=True)
    ref = ppo.PPOHistory(ref_model, lr=1e-4, minibatch=M, ent_coef=0.01, latent_coef=0.25)
    for it in range(2):
        s_ref = ref.update(obs, hist, priv, act, adv, ret, old_logp=old, epochs=2, generator=torch.Generator(device=dev).manual_seed(it))
    np.testing.assert_allclose(stats[1], s_ref, rtol=2e-4, atol=2e-5)
    # what a history policy is refused by stays refused; a plain model is refused here
    with pytest.raises(ValueError, match="FusedPPOHistory"):
        learner_hip.FusedPPO(history_policy(dev, 1))
    with pytest.raises(ValueError):
        learner_hip.FusedDistill(history_policy(dev, 1))
    with pytest.raises(ValueError, match="history encoder"):
        learner_hip.FusedPPOHistory(ppo.ActorCritic(dev, seed=1, priv_dim=48, actor_priv_dim=48))
    with pytest.raises(ValueError, match="latent_coef"):
        learner_hip.FusedPPOHistory(history_policy(dev, 1), latent_coef=-1.0)


# ---- d. the rollout -------------------------------------------------------------------------------------------------------------------
def test_graph_rollout_with_an_asymmetric_critic():
    """The eager first segment and the replayed ones equal collect_rollout(critic_priv=True) on a twin env with the same noise; vpred[k] is the
    teacher kernel's value on (obs[k], priv[k]); a third twin collected with critic_priv=False sees the same states (the actor is the same)
    and stores today's value, the history kernel's."""
    import torch
    from openroborl_amd import ppo, rollout
    dev = torch.device("cuda:0")
    n, T = 64, 4
    kw = dict(seed=11, auto_reset=True, contact_outputs=True, push=PUSH, push_outputs=True, config_overrides=short_episodes())
    envs = [mixed_env(n, **kw) for _ in range(3)]
    policies = [student_model(dev, 1).enable_fused() for _ in range(3)]
    collectors = [None, rollout.GraphRollout(envs[1], policies[1], T, critic_priv=True), rollout.GraphRollout(envs[2], policies[2], T, critic_priv=False)]
    assert collectors[1].critic_priv and not collectors[2].critic_priv and not rollout.GraphRollout(envs[2], policies[2], T).critic_priv
    obs = [e.reset() for e in envs]
    priv, hist = [None] * 3, [None] * 3
    gen = torch.Generator(device=dev).manual_seed(0)
    ended = 0
    for seg in range(3):                                             # eager, captured, replayed
        noise = torch.randn(T, n, 12, device=dev, generator=gen)
        a = rollout.collect_rollout(envs[0], policies[0], T, obs=obs[0], noise=noise, priv=priv[0], hist=hist[0], critic_priv=True)
        b = collectors[1].collect(obs[1], noise=noise, priv=priv[1], hist=hist[1])
        c = collectors[2].collect(obs[2], noise=noise, priv=priv[2], hist=hist[2])
        for k in ("obs", "actions", "rewards", "dones", "vpred", "last_obs", "priv", "last_priv", "hist", "last_hist"):
            assert torch.equal(a[k], b[k]), (seg, k)
            assert torch.equal(a[k], c[k]) == (k != "vpred"), (seg, k)
        for k in range(T):
            o, h, p = (b[x][k].contiguous() for x in ("obs", "hist", "priv"))
            assert torch.equal(raw_forward(policies[0].fused, "teacher", o, p, noise[k], n)[2][:, 0], b["vpred"][k]), (seg, k)
            _, s_raw, s_val = policies[0].act(o, hist=h, noise=noise[k])                  # today's forward pass: the estimate feeds the critic
            assert torch.equal(s_raw, c["actions"][k]) and torch.equal(s_val, c["vpred"][k]), (seg, k)
        ended += int(b["dones"].sum())
        obs = [x["last_obs"] for x in (a, b, c)]
        priv = [a["last_priv"].clone(), b["last_priv"], c["last_priv"]]
        hist = [a["last_hist"].clone(), b["last_hist"], c["last_hist"]]
        with torch.no_grad():                       # "the learner" moves the weights, encoder included
            for mdl in policies:
                for k2 in sorted(mdl.p):
                    mdl.p[k2].mul_(1.01)
                mdl.mark_updated()
    assert collectors[1].graph is not None and collectors[2].graph is not None and ended >= 1
    for e in envs[1:]:
        assert torch.equal(envs[0].state.view(torch.int32), e.state.view(torch.int32))
    # a policy without a history has no estimate to set the true row against
    teacher = ppo.ActorCritic(dev, seed=1, priv_dim=48, actor_priv_dim=48).enable_fused()
    with pytest.raises(ValueError, match="critic_priv"):
        rollout.GraphRollout(envs[0], teacher, T, critic_priv=True)
    with pytest.raises(ValueError, match="critic_priv"):
        rollout.collect_rollout(envs[0], teacher, 1, obs=obs[0], critic_priv=True)
    for e in envs:
        e.close()


# ---- e. train.py ----------------------------------------------------------------------------------------------------------------------
def test_train_history_ppo_from_scratch_and_from_its_own_zip_and_evaluate_it(tmp_path):
    from openroborl_amd import policy as pol
    first_zip, tuned_zip, log_path = str(tmp_path / "first.zip"), str(tmp_path / "tuned.zip"), str(tmp_path / "log.json")
    common = ["--history-ppo", "--num-robot", "64", "--horizon", "8", "--iters", "2", "--push", "0.05,0.2,0.5"]

    def run(*argv):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + list(argv), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        return r.stdout.decode()
    run("--save", first_zip, *common)
    first = pol.load_parameters(first_zip)
    assert first["model/pi_fc0/w:0"].shape == (208, 512) and first["model/vf_fc0/w:0"].shape == (208, 512)
    for k, shape in ENC.items():
        assert first[k].shape == shape, k
    run("--model-file", first_zip, "--latent-coef", "0.5", "--save", tuned_zip, "--log", log_path, *common)
    log = json.load(open(log_path))
    assert log and log[-1]["iter"] == 1
    for rec in log:
        assert math.isfinite(rec["latent_loss"]) and rec["latent_loss"] > 0.0 and math.isfinite(rec["surr"]) and math.isfinite(rec["vf"])
        assert math.isfinite(rec["mean_step_reward"])
    tuned = pol.load_parameters(tuned_zip)
    assert sorted(tuned) == sorted(first)
    for k in ("model/enc_fc0/w:0", "model/enc_fc1/w:0", "model/pi_fc0/w:0", "model/vf_fc0/w:0"):       # fine-tuning moves encoder, actor and critic
        assert tuned[k].tobytes() != first[k].tobytes(), k
    rec = json.loads(run("--eval", tuned_zip, "--num-robot", "16").strip().splitlines()[-1])
    assert rec["robots"] == 16 and math.isfinite(rec["return_mean"])
