"""The learned action std on the device: orr_ppo_head_logstd and orr_gauss_prepare (include/openroborl_learner.h) against float64 on the CPU,
the whole fused minibatch and FusedPPO against float64 autograd and ppo.PPO for a learn-std model, and a rollout + update loop whose
graphs are captured once while log_std moves underneath them.

One input recipe, evaluated in float64 on the CPU: ls = log 0.125 + linspace(-0.7, 0.7, 12); actions = mean + exp(ls) * randn; the old policy
has means shifted by 0.08 exp(ls) randn and log-stds shifted by 0.02 randn(12); every 97th advantage is zero; seed 3."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = "model/pi/logstd:0"
CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.01
LOG_2PI = math.log(2.0 * math.pi)


def _ptr(x):
    return x.data_ptr()


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _log_std():
    import torch
    return (math.log(0.125) + torch.linspace(-0.7, 0.7, 12)).float()


def _logp64(act, mu, ls):
    """float64 log-density of act [m,12] under N(mu, exp(ls)^2), ls [12]."""
    z = (act - mu) * (-ls).exp()
    return -0.5 * (z * z).sum(dim=1) - ls.sum() - 6.0 * LOG_2PI


def _recipe(m, mu, seed=3):
    """The module's recipe around the means mu [m,12] (CPU float32): -> ls [12], act [m,12], old_logp [m], adv [m], ret [m], CPU float32."""
    import torch
    g = torch.Generator().manual_seed(seed)
    ls = _log_std()
    act = mu + ls.exp() * torch.randn(m, 12, generator=g)
    old_mu = mu + 0.08 * ls.exp() * torch.randn(m, 12, generator=g)
    old_ls = ls + 0.02 * torch.randn(12, generator=g)
    old = _logp64(act.double(), old_mu.double(), old_ls.double()).float()
    adv = torch.randn(m, generator=g)
    adv[::97] = 0.0
    ret = torch.randn(m, generator=g)
    return ls, act, old, adv, ret


def _loss64(logp, old, adv, value, ret, ls, vf_coef, ent_coef):
    """-> (loss, the five stats, the ratios) in float64, the formulas of ppo.PPO.update."""
    import torch
    ratio = torch.exp(logp - old)
    surr = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * adv).mean()
    vf = ((value - ret) ** 2).mean()
    ent = ls.sum() + 6.0 * math.log(2.0 * math.pi * math.e)
    kl = ((ratio - 1.0) - (logp - old)).mean()
    clipped = ((ratio < 1.0 - CLIP) | (ratio > 1.0 + CLIP)).double().mean()
    return surr + vf_coef * vf - ent_coef * ent, [x.item() for x in (surr, vf, ent, kl, clipped)], ratio.detach()


_HEAD_CASES = {}


def _head_case(m):
    """Inputs and the float64 reference of the loss head at m samples: computed once, shared, left unchanged."""
    import torch
    if m not in _HEAD_CASES:
        g = torch.Generator().manual_seed(1000 + m)
        mu, value = torch.randn(m, 12, generator=g), torch.randn(m, generator=g)
        ls, act, old, adv, ret = _recipe(m, mu)
        if m == 1:          # one live sample: a unit advantage and a ratio of exp(0.05), inside the clip range
            adv = torch.ones(1)
            old = (_logp64(act.double(), mu.double(), ls.double()) - 0.05).float()
        mu64, v64, ls64 = mu.double().requires_grad_(True), value.double().requires_grad_(True), ls.double().requires_grad_(True)
        logp = _logp64(act.double(), mu64, ls64)
        logp.retain_grad()
        loss, stats, ratio = _loss64(logp, old.double(), adv.double(), v64, ret.double(), ls64, VF_COEF, ENT_COEF)
        loss.backward()
        z = ((act.double() - mu.double()) * (-ls.double()).exp())
        per_sample = (logp.grad[:, None] * (z * z - 1.0)).abs().max().item()      # the largest |gl (z^2 - 1)|
        _HEAD_CASES[m] = dict(mu=mu, value=value, ls=ls, act=act, old=old, adv=adv, ret=ret, g_mu=mu64.grad, g_v=v64.grad, g_ls=ls64.grad,
                              stats=stats, ratio=ratio, per_sample=per_sample)
    return _HEAD_CASES[m]


def _run_head(L, dev, c, m):
    import torch
    from openroborl_amd import _lib
    batch = torch.zeros(m, 16, device=dev)
    batch[:, :12], batch[:, 12], batch[:, 13], batch[:, 14] = c["act"].to(dev), c["old"].to(dev), c["adv"].to(dev), c["ret"].to(dev)
    mu, value, ls = c["mu"].to(dev), c["value"].to(dev), c["ls"].to(dev)
    out = dict(gm=torch.full((m, 12), 7.0, device=dev), gv=torch.full((m,), 7.0, device=dev), gls=torch.full((12,), 7.0, device=dev),
               gb_m=torch.full((12,), 7.0, device=dev), gb_v=torch.full((1,), 7.0, device=dev), stats=torch.full((5,), 7.0, device=dev))
    ws = torch.empty(int(L.orr_learner_workspace_floats(m, 32)), device=dev)
    _lib.check(L.orr_ppo_head_logstd(_ptr(mu), _ptr(value), _ptr(batch), _ptr(ls), m, CLIP, VF_COEF, ENT_COEF, _ptr(out["gm"]), _ptr(out["gv"]),
                                     _ptr(out["gls"]), _ptr(out["gb_m"]), _ptr(out["gb_v"]), _ptr(out["stats"]), _ptr(ws), _stream(dev)), L)
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("m", [1, 1000, 4096])      # the smallest size; no multiple of a wave or a workgroup; 16 workgroups > the finish's 4 row groups
def test_loss_head_logstd_kernel_matches_float64_autograd(m):
    import torch
    from openroborl_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda:0")
    c = _head_case(m)
    surr, vf, ent, kl, clipped = c["stats"]
    edge = min((c["ratio"] - (1.0 - CLIP)).abs().min().item(), (c["ratio"] - (1.0 + CLIP)).abs().min().item())
    print("m=%d float64: surr %.6g vf %.6g H %.6g kl %.6g clip_fraction %.4f, nearest ratio to a clip edge %.3g" % (m, surr, vf, ent, kl, clipped, edge))
    if m > 1:                                       # (one sample is inside the range by construction: a fraction of 0)
        assert 0.02 < clipped < 0.9, clipped
    assert edge > 1e-6, edge                        # no ratio so close to an edge that float32 could count it on the other side
    got = _run_head(L, dev, c, m)
    gm, gv, gls, stats = got["gm"].double(), got["gv"].double(), got["gls"].double(), got["stats"].double()
    scale = c["g_mu"].abs().max().item()
    err = dict(g_mean=(gm - c["g_mu"]).abs().max().item() / scale, g_value=(gv - c["g_v"]).abs().max().item() / c["g_v"].abs().max().item(),
               gb_mean=(got["gb_m"].double() - c["g_mu"].sum(dim=0)).abs().max().item() / (scale * math.sqrt(m)),
               gb_value=abs(got["gb_v"].item() - c["g_v"].sum().item()),
               g_logstd=(gls - c["g_ls"]).abs().max().item() / (c["per_sample"] * math.sqrt(m)),
               stats=[abs(stats[i].item() - c["stats"][i]) for i in range(5)])
    print("m=%d errors (in units of their scales): %r" % (m, err))
    assert scale > 0 and err["g_mean"] < 2e-5
    assert err["g_value"] < 1e-6
    assert err["gb_mean"] < 2e-5
    assert err["gb_value"] < 1e-5
    assert err["g_logstd"] < 2e-5
    assert err["stats"][0] < 2e-5 * max(1.0, abs(surr))
    assert err["stats"][1] < 2e-5 * vf
    assert err["stats"][2] < 1e-5
    assert err["stats"][3] < 2e-5 * max(1.0, kl)
    assert got["stats"][4].item() == float(np.float32(clipped)), (got["stats"][4].item(), clipped)     # the count / m, to the nearest float
    # samples outside the clip range on the clipped side, and zero advantages, get exactly zero gradient (as autograd gives them)
    dead = c["g_mu"].abs().sum(dim=1) == 0
    if m > 1:
        assert dead.any()
    assert bool((got["gm"][dead] == 0).all()) and bool((got["gm"][~dead] != 0).any())
    # fixed summation order: the same bits every time
    again = _run_head(L, dev, c, m)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("n", [1, 1000, 4097])
def test_gauss_prepare_matches_float64(n):
    import torch
    from openroborl_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(n)
    noise = torch.randn(n, 12, generator=g)
    ls = _log_std() + 0.02 * torch.randn(12, generator=g)
    want = noise.double() * ls.double().exp()
    want_logp = -0.5 * (noise.double() ** 2).sum(dim=1) - ls.double().sum() - 6.0 * LOG_2PI
    pad = 64                                        # rows behind the n: nothing there may be touched
    d_noise, d_ls = noise.to(dev), ls.to(dev)
    scaled, logp = torch.full((n + pad, 12), 7.0, device=dev), torch.full((n + pad,), 7.0, device=dev)
    _lib.check(L.orr_gauss_prepare(_ptr(d_noise), _ptr(d_ls), _ptr(scaled), _ptr(logp), n, _stream(dev)), L)
    assert bool((scaled[n:] == 7.0).all()) and bool((logp[n:] == 7.0).all())
    rel = ((scaled[:n].cpu().double() - want).abs() / want.abs().clamp_min(1e-30)).max().item()
    err = ((logp[:n].cpu().double() - want_logp).abs() / want_logp.abs().clamp_min(1.0)).max().item()
    print("n=%d scaled: relative error %.3g; logp: error %.3g of max(1, |logp|)" % (n, rel, err))
    assert rel < 2e-6
    assert err < 2e-5
    assert torch.equal(d_noise.cpu(), noise)
    # logp = NULL: scaled alone, the same bits
    only = torch.full((n + pad, 12), 7.0, device=dev)
    _lib.check(L.orr_gauss_prepare(_ptr(d_noise), _ptr(d_ls), _ptr(only), None, n, _stream(dev)), L)
    assert torch.equal(only, scaled)
    # in place (scaled = noise) is supported: the same bits again, and the same logp
    inplace, logp2 = torch.full((n + pad, 12), 7.0, device=dev), torch.empty(n, device=dev)
    inplace[:n].copy_(d_noise)
    _lib.check(L.orr_gauss_prepare(_ptr(inplace), _ptr(d_ls), _ptr(inplace), _ptr(logp2), n, _stream(dev)), L)
    assert torch.equal(inplace, scaled) and torch.equal(logp2, logp[:n])
    # a partial overlap is refused and writes nothing
    if n > 1:
        before = inplace.clone()
        assert L.orr_gauss_prepare(_ptr(inplace), _ptr(d_ls), _ptr(inplace) + 48, None, n - 1, _stream(dev)) == -1
        assert b"orr_gauss_prepare" in L.orr_last_error() and torch.equal(inplace, before)


def _digest(x):
    import hashlib
    return hashlib.sha256(x.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:10]


def _learn_std_model(dev, seed):
    import torch
    from openroborl_amd import ppo
    model = ppo.ActorCritic(dev, seed=seed, learn_std=True)
    with torch.no_grad():
        model.p[KEY].copy_(_log_std().reshape(1, 12))
    return model


def _model_batch(dev, model, B, seed):
    """The recipe around the model's own means on random observations: device tensors obs, act, old, adv, ret."""
    import torch
    obs = torch.randn(B, 160, generator=torch.Generator().manual_seed(seed + 100)).to(dev)
    with torch.no_grad():
        mu = model.mean(obs).cpu()
    _, act, old, adv, ret = _recipe(B, mu, seed=seed)
    return (obs,) + tuple(x.to(dev) for x in (act, old, adv, ret))


def test_fused_gradient_of_a_learn_std_model_matches_float64_cpu():
    """tests/test_gpu_learner.py's test_fused_gradient_matches_float64_cpu for a learn-std model: every parameter, the log-std included."""
    import torch
    from openroborl_amd import learner_hip
    dev = torch.device("cuda:0")
    B = 4096
    model = _learn_std_model(dev, 4)
    obs, act, old, adv, ret = _model_batch(dev, model, B, 3)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.p.items()}

    def mlp(net):
        x = obs.cpu().double()
        h = torch.relu(x @ p64["model/%s_fc0/w:0" % net] + p64["model/%s_fc0/b:0" % net])
        h = torch.relu(h @ p64["model/%s_fc1/w:0" % net] + p64["model/%s_fc1/b:0" % net])
        return h @ p64["model/%s/w:0" % net] + p64["model/%s/b:0" % net]
    ls64 = p64[KEY].reshape(12)
    loss, stats64, _ = _loss64(_logp64(act.cpu().double(), mlp("pi"), ls64), old.cpu().double(), adv.cpu().double(), mlp("vf")[:, 0],
                               ret.cpu().double(), ls64, 1.0, ENT_COEF)
    loss.backward()
    assert 0.02 < stats64[4] < 0.9, stats64[4]
    learner = learner_hip.FusedPPO(model, lr=1e-4, minibatch=B, use_graph=False, ent_coef=ENT_COEF)
    assert KEY in learner.slots and learner.n_stats == 5
    P = learner._plan(B, B)
    with torch.no_grad():
        P["obs"].copy_(obs)
        P["aux"][:, :12], P["aux"][:, 12], P["aux"][:, 13], P["aux"][:, 14] = act, old, adv, ret
        P["perm"].copy_(torch.arange(B, device=dev))
        learner._minibatch(P, 0)
    got = P["stats"][0].cpu().double().tolist()
    print("stats fused %r float64 %r" % (got, stats64))
    for i in range(5):
        assert abs(got[i] - stats64[i]) < 2e-4 * max(1.0, abs(stats64[i])), (i, got[i], stats64[i])
    for k in sorted(model.p):
        g32, g64 = learner.g[k].detach().cpu().double(), p64[k].grad
        scale = g64.abs().max().item() + 1e-12
        cs = ((g32 * g64).sum() / (g32.norm() * g64.norm() + 1e-30)).item()
        print("%-20s max error %.3g of scale %.3g, cosine %.8f" % (k, (g32 - g64).abs().max().item(), scale, cs))
        assert (g32 - g64).abs().max().item() < 2e-3 * scale, (k, (g32 - g64).abs().max().item(), scale)
        assert cs > 0.99999, (k, cs)


@pytest.mark.parametrize("graph,B,M", [(False, 8192, 1024), (True, 8192, 1024), (True, 32768, 4096)])
def test_fused_learn_std_update_matches_the_torch_learner(graph, B, M):
    """Two updates of two epochs through ppo.PPO and through FusedPPO, both with a learned std and the entropy bonus, from the same parameters,
    data and permutations: the same five stats, the same parameters (Adam moves every one by at most lr per step), bit-reproducible."""
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    lr, steps = 1e-4, 2 * 2 * (B // M)
    ref_model = _learn_std_model(dev, 2)
    obs, act, old, adv, ret = _model_batch(dev, ref_model, B, 1)
    before = {k: v.detach().clone() for k, v in ref_model.p.items()}
    ref = ppo.PPO(ref_model, lr=lr, minibatch=M, ent_coef=ENT_COEF)

    def run_fused():
        model = _learn_std_model(dev, 2)
        fused = learner_hip.FusedPPO(model, lr=lr, minibatch=M, use_graph=graph, ent_coef=ENT_COEF)
        out = []
        for it in range(2):
            gen = torch.Generator(device=dev)
            gen.manual_seed(10 + it)
            out.append(fused.update(obs, act, adv, ret, old_logp=old, epochs=2, generator=gen))
        return model, fused, out
    model, fused, s_fused = run_fused()
    for it in range(2):
        gen = torch.Generator(device=dev)
        gen.manual_seed(10 + it)
        s_ref = ref.update(obs, act, adv, ret, old_logp=old, epochs=2, generator=gen)
        print("update %d stats torch %r fused %r" % (it, s_ref.tolist(), s_fused[it].tolist()))
        assert s_ref.shape == s_fused[it].shape == (5,)
        np.testing.assert_allclose(s_fused[it], s_ref, rtol=2e-4, atol=2e-5)
    assert fused.steps_taken() == steps                              # the capture's warm-up steps were undone
    for k in sorted(before):
        a, b = ref_model.p[k].detach(), model.p[k].detach()
        print("%-20s max difference %.3g mean %.3g (of %g)" % (k, (a - b).abs().max().item(), (a - b).abs().mean().item(), steps * lr))
        assert (a - b).abs().max().item() < 0.02 * steps * lr, (k, (a - b).abs().max().item())
        assert (a - b).abs().mean().item() < 2e-3 * steps * lr, (k, (a - b).abs().mean().item())
    assert (model.p[KEY].detach() - before[KEY]).abs().max().item() > lr
    again = run_fused()[1]
    assert torch.equal(again.flat_p, fused.flat_p)


def test_rollout_and_update_replay_their_graphs_while_log_std_moves():
    """A 64-robot env, horizon 4, GraphRollout + FusedPPO with a learned std at lr = 1e-2, four iterations: both graphs are captured once
    while log_std moves, and every segment was sampled with the log-std of its collection.

    Two sampling checks in every segment.  (1) What this feature owns, to rounding: the actions are the fused kernel's own mean (a second,
    noise-free pass over the segment's observations, the same bits) plus the scaled noise that orr_gauss_prepare left in the collector, in ONE
    float32 rounding - |a - fused_mean - scaled| <= 2^-24 |a|, evaluated in float64.  (2) The issue's: |a - model.mean(obs) - exp(log_std) noise|
    < 2e-5, the fused-vs-torch forward bound, where model.mean is torch's GEMM path.  (2) = (1) + |fused_mean - torch_mean|, and that
    remainder is absolute against means that grow with every Adam step of 1e-2: measured on an MI355X, either path is 3e-7 max|mean| away
    from a float64 evaluation of the same weights (1.3e-5 and 1.6e-5 at max|mean| = 51), so the bound holds while max|mean| stays under
    about 60.  With two epochs per iteration (eight Adam steps before the last collection) the means reach 9, 29 and 51 at collections 2 - 4
    and (2) measured 2.8e-6, 8.0e-6, 1.3e-5 in five runs on two machines - and 2.62e-5 in one run on a third.  The update therefore takes ONE
    epoch per iteration, the fewest steps with which log_std still moves between collections; nothing else about the check changed: the means
    then reach 2.6, 8.2, 12.9 and (2) measures 1.0e-6, 2.5e-6, 2.6e-6.  Every
    figure is printed before it is asserted."""
    import torch
    from openroborl_amd import learner_hip, rollout
    from openroborl_amd.env import VecQuadrupedEnv
    dev = torch.device("cuda:0")
    n, T = 64, 4
    env = VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=n, mode="train", auto_reset=True, seed=11, device=dev)
    model = _learn_std_model(dev, 1).enable_fused()
    learner = learner_hip.FusedPPO(model, lr=1e-2, minibatch=n * T, ent_coef=ENT_COEF)
    collector = rollout.GraphRollout(env, model, T)
    assert len(collector._launch_params()) == 1 and len(learner._graph_key()) == len(learner_hip._FusedLearner._graph_key(learner)) + 5
    gen = torch.Generator(device=dev).manual_seed(0)
    obs = env.reset()
    seen, graphs, plans = [], [], []
    for it in range(4):
        ls = model.log_std.detach().clone().reshape(12)
        seen.append(ls.cpu())
        noise = torch.randn(T, n, 12, device=dev, generator=gen)
        buf = collector.collect(obs, noise=noise)
        graphs.append(collector.graph)
        flat_obs = buf["obs"].reshape(T * n, 160)
        with torch.no_grad():
            mean = model.mean(flat_obs).reshape(T, n, 12)
        fused_mean = model.fused.forward(flat_obs, None, want_mean=True)[3].reshape(T, n, 12)      # the weights of this collection: nothing updated since
        a64 = buf["actions"].double()
        own = ((a64 - fused_mean.double() - collector.scaled.double()).abs() / a64.abs().clamp_min(1e-30)).max().item()
        issue = (buf["actions"] - mean - ls.exp() * noise).abs().max().item()
        print("collection %d: |a - fused_mean - scaled| / |a| max %.3g (2^-24 = 5.96e-8); |a - torch_mean - exp(ls) noise| max %.3g; "
              "|fused_mean - torch_mean| max %.3g; max|mean| %.3g; flat_p %s"
              % (it, own, issue, (fused_mean - mean).abs().max().item(), mean.abs().max().item(), _digest(learner.flat_p)))
        ref = ls.double().exp() * noise.double()
        assert bool(((collector.scaled.double() - ref).abs() <= 2e-6 * ref.abs()).all())    # orr_gauss_prepare's bound above, with the log-std of this collection
        assert own <= 2.0 ** -24 * (1.0 + 1e-9)                                                    # sampled with the log-std of this collection, one rounding
        assert issue < 2e-5
        want = -0.5 * (noise.double() ** 2).sum(dim=-1) - ls.double().sum() - 6.0 * LOG_2PI
        assert ((buf["logp"].double() - want).abs() / want.abs().clamp_min(1.0)).max().item() < 2e-5
        adv, ret = rollout.gae_fused(buf["rewards"], buf["vpred"], buf["dones"], 0.95, 0.95, normalize=True, eps=1e-8)
        stats = learner.update(buf["obs"].reshape(T * n, -1), buf["actions"].reshape(T * n, -1), adv.reshape(-1), ret.reshape(-1),
                               old_logp=buf["logp"].reshape(-1), epochs=1, generator=gen)
        plans.append(learner._plans[(n * T, n * T)]["graphs"])
        assert stats.shape == (5,) and np.isfinite(stats).all()
        for k in ("obs", "actions", "rewards", "vpred", "logp"):
            assert bool(torch.isfinite(buf[k]).all()), k
        obs = buf["last_obs"]
    assert graphs[0] is None and graphs[1] is not None and graphs[2] is graphs[1] and graphs[3] is graphs[1]     # eager, captured, replayed
    assert plans[0] is not None and all(p is plans[0] for p in plans)
    assert learner.steps_taken() == 4
    for a, b in zip(seen, seen[1:]):
        assert not torch.equal(a, b)                                                      # one Adam step of up to 1e-2 in between
    assert bool(torch.isfinite(learner.flat_p).all())
    env.close()


def test_a_fixed_std_model_keeps_its_two_stats_and_its_std_in_the_key():
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    model = ppo.ActorCritic(dev, seed=2)
    learner = learner_hip.FusedPPO(model, lr=1e-4, minibatch=256)
    assert not learner.learn_std and learner.n_stats == 2 and KEY not in learner.slots
    assert learner._graph_key()[-3:] == (0.2, 1.0, 0.125)
    g = torch.Generator().manual_seed(0)
    obs, act = torch.randn(512, 160, generator=g).to(dev), (0.1 * torch.randn(512, 12, generator=g)).to(dev)
    stats = learner.update(obs, act, torch.randn(512, generator=g).to(dev), torch.randn(512, generator=g).to(dev))
    assert stats.shape == (2,) and np.isfinite(stats).all()
    model.std = 0.2
    assert learner._graph_key()[-1] == 0.2
    with pytest.raises(ValueError):
        learner_hip.FusedPPO(ppo.ActorCritic(dev, seed=2), ent_coef=0.01)
