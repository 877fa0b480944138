"""orr_policy_forward_recurrent, a recurrent policy's step in one launch with an optional asymmetric critic, against the recurrence and the two
MLPs spelled out in float64; its host path (FusedActorCritic, the rollout), the torch learner ppo.PPORecurrent and train.py --recurrent-ppo."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_gpu_recurrent import H, SENTINEL, Z, _guarded, _pads_untouched, _reference

pytestmark = pytest.mark.gpu

STD, CLIP = 0.01, 0.1
OUTS = {"hid": H, "latent": Z, "mean": 12, "raw": 12, "action": 12, "value": None}


@functools.lru_cache(maxsize=None)
def _model(fused=True, seed=3):
    import torch
    from openroborl_amd import ppo
    model = ppo.ActorCritic(torch.device("cuda:0"), priv_dim=48, actor_priv_dim=48, recurrent=256, seed=seed)      # the project's initial scale
    return model.enable_fused() if fused else model


def _inputs(n):
    """Robot 0's observation is 20 x the others': its action clips.  Robots 1, 4, .. start, inside every workgroup."""
    rng = np.random.default_rng(40 + n)
    f = lambda *shape: rng.normal(0, 1, shape).astype(np.float32)   # noqa: E731
    ins = {"obs": f(n, 160), "start": (np.arange(n) % 3 == 1).astype(np.uint8), "h0": rng.uniform(-0.9, 0.9, (n, H)).astype(np.float32),
           "priv": f(n, Z), "noise": f(n, 12)}
    ins["obs"][0] *= 20.0
    return ins


def _step_reference(ins, with_priv, with_h0, dtype):
    """The recurrence of test_gpu_recurrent._reference (T = 1), then the two ReLU MLPs: the actor on obs | z, the critic on obs | priv or obs | z."""
    P = {k: v.detach().cpu().numpy().astype(dtype) for k, v in _model().p.items()}
    g = _reference({k: v for k, v in P.items() if k.startswith("model/gru_")}, ins["obs"][None], ins["start"][None], ins["h0"] if with_h0 else None, dtype)
    out = {"hid": g["hid"][0], "latent": g["latent"][0]}
    def mlp(net, x):
        for layer in ("model/%s_fc0" % net, "model/%s_fc1" % net):
            x = np.maximum(x @ P[layer + "/w:0"] + P[layer + "/b:0"], 0)
        return x @ P["model/%s/w:0" % net] + P["model/%s/b:0" % net]
    obs = ins["obs"].astype(dtype)
    out["mean"] = mlp("pi", np.concatenate((obs, out["latent"]), axis=1))
    out["raw"] = out["mean"] + dtype(STD) * ins["noise"].astype(dtype)
    out["action"] = np.clip(out["raw"], -CLIP, CLIP)
    out["value"] = mlp("vf", np.concatenate((obs, ins["priv"].astype(dtype) if with_priv else out["latent"]), axis=1))[:, 0]
    return out


@functools.lru_cache(maxsize=None)
def _tolerance():
    """8 x the largest difference of the float32 numpy evaluation from the float64 one at n = 33 (test_gpu_recurrent._tolerance's rule)."""
    ins = _inputs(33)
    a, b = _step_reference(ins, True, True, np.float32), _step_reference(ins, True, True, np.float64)
    assert (np.abs(b["raw"][0]) > CLIP).any() and (np.abs(b["raw"][1:]) < CLIP).any()
    return 8.0 * max(np.abs(a[k].astype(np.float64) - b[k]).max() for k in OUTS)


def _call(ins, with_priv=True, with_h0=True, outs=tuple(OUTS), change=None, expect=0):
    """One raw call.  change: {argument: None (a null pointer) | +bytes | another argument's name (its address)}.  -> the outputs as numpy."""
    import torch
    from openroborl_amd import _lib
    dev, fused, n, L = torch.device("cuda:0"), _model().fused, len(ins["obs"]), _lib.load()
    dins = {k: torch.from_numpy(v).to(dev) for k, v in ins.items()}
    bufs = {k: _guarded((n,) if w is None else (n, w), dev) for k, w in OUTS.items()}
    p = {k: v.data_ptr() for k, v in dins.items()}
    p.update({k: (bufs[k][1].data_ptr() if k in outs else None) for k in OUTS})
    p.update(net=C.addressof(fused.net), enc=C.addressof(fused.gru.enc), n=n)
    p.update({k: None for k, on in (("priv", with_priv), ("h0", with_h0)) if not on})
    for k, v in (change or {}).items():
        p[k] = v if (v is None or k == "n") else (p[v] if isinstance(v, str) else p[k] + v)
    rc = L.orr_policy_forward_recurrent(C.cast(p["net"], C.POINTER(type(fused.net))), C.cast(p["enc"], C.POINTER(type(fused.gru.enc))), p["obs"], p["start"],
                                        p["h0"], p["priv"], p["n"], p["noise"], STD, CLIP, p["action"], p["raw"], p["value"], p["mean"], p["hid"],
                                        p["latent"], None)
    torch.cuda.synchronize()
    assert (rc == 0) if expect == 0 else (rc < 0 and L.orr_last_error()), rc
    assert all(_pads_untouched(full) for full, _ in bufs.values())
    if expect:
        assert all(bool((full == SENTINEL).all()) for full, _ in bufs.values())
    return {k: bufs[k][1].cpu().numpy() for k in outs}


@pytest.mark.parametrize("with_h0", [True, False])
@pytest.mark.parametrize("with_priv", [True, False])
@pytest.mark.parametrize("n", [1, 16, 17, 33])
def test_step_matches_float64(n, with_priv, with_h0):
    got, want, tol = _call(_inputs(n), with_priv, with_h0), _step_reference(_inputs(n), with_priv, with_h0, np.float64), _tolerance()
    for k in OUTS:
        err = np.abs(got[k].astype(np.float64) - want[k]).max()
        print("n=%d priv=%s h0=%s %s: error %.3e, tolerance %.3e" % (n, with_priv, with_h0, k, err, tol))
        assert err < tol, (k, err, tol)


def test_asymmetric_critic_and_inert_optional_outputs():
    ins, tol, (asym, sym) = _inputs(33), _tolerance(), (_call(_inputs(33), True), _call(_inputs(33), False))
    assert np.abs(asym["value"] - sym["value"]).max() > tol
    assert np.abs(asym["value"] - _step_reference(ins, True, True, np.float64)["value"]).max() < tol
    bare = _call(ins, True, outs=("hid", "action"))
    for k in ("action", "raw", "mean", "hid", "latent"):
        assert np.array_equal(asym[k], sym[k]) and (k not in bare or np.array_equal(asym[k], bare[k])), k


def test_chained_in_place_steps_are_the_gru_kernels_bits():
    """Four steps with hid aliasing h0 against orr_gru_forward(T = 4): the same accumulation order, hence the same bits."""
    import torch
    dev, n, T = torch.device("cuda:0"), 33, 4
    steps = [_inputs(n) for _ in range(T)]
    for t, s in enumerate(steps):
        s["obs"] = np.random.default_rng(t).normal(0, 1, (n, 160)).astype(np.float32)
        s["start"] = (np.arange(n) % 4 == t).astype(np.uint8)
    whole_latent = torch.empty((T, n, Z), device=dev)
    whole = _model().fused.gru.forward(torch.from_numpy(np.stack([s["obs"] for s in steps])).to(dev), torch.from_numpy(np.stack([s["start"] for s in steps])).to(dev),
                                       torch.from_numpy(steps[0]["h0"]).to(dev), latent=whole_latent)
    h, z, act = torch.from_numpy(steps[0]["h0"]).to(dev), torch.empty((n, Z), device=dev), torch.empty((2, n, 12), device=dev)
    for t, s in enumerate(steps):
        d = {k: torch.from_numpy(s[k]).to(dev) for k in ("obs", "start", "noise")}
        for rep in range(2 if t == 0 else 1):             # step 0 twice from the same state: the same bits
            h_in = h.clone() if t == 0 else h
            _model().fused.forward(d["obs"], d["noise"], hidden=h_in, start=d["start"], out_hidden=h_in, out_latent=z, out_action=act[rep], want_value=False)
            assert torch.equal(h_in, whole[t]) and torch.equal(z, whole_latent[t]), t
        if t == 0:
            h = h_in
            assert torch.equal(act[0], act[1])


@pytest.mark.parametrize("change", [{"net": None}, {"enc": None}, {"obs": None}, {"hid": None}, {"action": None}, {"n": 0}, {"hid": +4}, {"hid": "h0", "h0": +64},
                                    {"latent": "hid"}, {"value": "obs"}], ids=str)
def test_step_refuses(change):
    _call(_inputs(17), change=change, expect=-1)


def test_host_path_matches_torch_and_bf16_refuses_priv():
    import torch
    from openroborl_amd import policy_hip
    dev, ins, tol = torch.device("cuda:0"), _inputs(33), _tolerance()
    d = {k: torch.from_numpy(v).to(dev) for k, v in ins.items()}
    for priv in (d["priv"], None):
        kw = dict(hidden=d["h0"], start=d["start"], noise=d["noise"], **({} if priv is None else {"priv": priv}))
        got, want = _model().act(d["obs"], **kw), _model(fused=False).act(d["obs"], **kw)
        for a, b in zip(got, want):
            assert (a - b).abs().max().item() < tol
    bf16 = policy_hip.FusedActorCritic(_model().p, dev, std=0.125, bf16_gru=True)
    bf16.forward(d["obs"], d["noise"], hidden=d["h0"], start=d["start"])
    with pytest.raises(ValueError):
        bf16.forward(d["obs"], d["noise"], hidden=d["h0"], start=d["start"], priv=d["priv"])


def test_graph_rollout_records_priv_and_values_of_the_true_row():
    import torch
    from openroborl_amd import rollout
    from tests import gpu_kit
    T, n = 3, 32
    env = gpu_kit.mixed_env(n, seed=11, auto_reset=True, contact_outputs=True, config_overrides=gpu_kit.short_episodes())
    collector = rollout.GraphRollout(env, _model(), T, critic_priv=True)
    obs, state = env.reset(), {}
    for _ in range(3):                                       # eager, capture, replay
        buf = collector.collect(obs, generator=torch.Generator(device=env.device).manual_seed(1), **state)
        assert buf["priv"].shape == (T, n, Z) and buf["hid"].shape == (T, n, H) and torch.equal(buf["starts"][1:], buf["dones"][:-1])
        want = _model(fused=False).value(buf["obs"].reshape(T * n, 160), buf["priv"].reshape(T * n, Z)).view(T, n)
        assert (buf["vpred"] - want).abs().max().item() < _tolerance()
        obs, state = buf["last_obs"].clone(), {"hidden": buf["last_hidden"].clone(), "start": buf["dones"][-1].clone(), "priv": buf["last_priv"].clone()}


def test_learner_gradient_is_autograd_of_the_stated_loss():
    """On the CPU in float64, one minibatch of all robots: PPORecurrent's step direction against the loss written out by hand."""
    import torch
    from openroborl_amd import history, ppo
    T, N, g = 3, 4, torch.Generator().manual_seed(0)
    model = ppo.ActorCritic("cpu", priv_dim=48, actor_priv_dim=48, recurrent=256, seed=5)
    model.p = {k: v.detach().double().requires_grad_(True) for k, v in model.p.items()}
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    obs, starts, h0, priv, act, adv, ret = r(T, N, 160), torch.rand(T, N, generator=g) < 0.3, 0.3 * r(N, H), r(T, N, Z), 0.1 * r(T, N, 12), r(T, N), r(T, N)
    with torch.no_grad():
        old = model.log_prob(obs.reshape(-1, 160), act.reshape(-1, 12), priv=history.encode_seq(model.p, obs, starts, h0)[1].reshape(-1, Z)) + 0.3 * r(T * N)
    _, z = history.encode_seq(model.p, obs, starts, h0)
    ratio = torch.exp(model.log_prob(obs.reshape(-1, 160), act.reshape(-1, 12), priv=z.reshape(-1, Z)) - old)
    loss = (-torch.min(ratio * adv.reshape(-1), ratio.clamp(0.8, 1.2) * adv.reshape(-1)).mean()
            + ((model.value(obs.reshape(-1, 160), priv.reshape(-1, Z)) - ret.reshape(-1)) ** 2).mean() + 0.5 * ((z - priv) ** 2).sum(-1).mean())
    want = dict(zip(sorted(model.p), torch.autograd.grad(loss, [model.p[k] for k in sorted(model.p)])))
    learner = ppo.PPORecurrent(model, minibatch=T * N, latent_coef=0.5)
    learner._step = lambda kl=None: None                     # keep the gradients, take no step
    stats = learner.update(obs, starts, h0, priv, act, adv.reshape(-1), ret.reshape(-1), old_logp=old, generator=g)
    assert len(stats) == 3 and abs(stats[2] - ((z - priv) ** 2).sum(-1).mean().item()) < 1e-9
    for k in sorted(want):
        assert torch.allclose(model.p[k].grad, want[k], rtol=1e-9, atol=1e-12) and want[k].abs().max() > 0, k


def test_train_recurrent_ppo(tmp_path):
    import json
    from tests import gpu_kit
    path = str(tmp_path / "recurrent.zip")
    out = gpu_kit.run_train("--recurrent-ppo", "--iters", "2", "--num-robot", "64", "--horizon", "8", "--latent-coef", "0.1", "--save", path)
    assert "fused learner is not built yet" in out and np.isfinite(json.loads(out.strip().splitlines()[-1])["latent_loss"])
    rec = json.loads(gpu_kit.run_train("--eval", path, "--num-robot", "16").strip().splitlines()[-1])
    assert rec["robots"] == 16 and np.isfinite(rec["return_mean"])


@pytest.mark.parametrize("flag", [["--history", "--distill", "x.zip"], ["--history-ppo"], ["--distill", "x.zip"], ["--hip-forward"], ["--hip-backward"],
                                  ["--bf16-gemm"], ["--obs-norm"]], ids=lambda f: f[0])
def test_train_refuses_recurrent_ppo_with(flag):
    from tests import gpu_kit
    gpu_kit.train_refuses(["--recurrent-ppo", "--num-robot", "64", "--iters", "1"] + flag, "--recurrent-ppo is a mode of its own")
