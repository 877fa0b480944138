"""The privileged critic on the device (run with -m gpu on an MI355X):

  1. orr_privileged_obs: every word of the row against numpy float64 built from the records and the bound buffers, read back; the
     unbound cases; the refusals;
  2. orr_policy_forward_priv: the actor bit for bit orr_policy_forward's, the value against the float64 MLP on cat(obs, priv), the tile's
     edges, the guard bands;
  3. rollout.GraphRollout with a privileged critic against rollout.collect_rollout and against a twin env;
  4. learner_hip.FusedPPO with `priv` against ppo.PPO with `priv` and against float64;
  5. train.py --privileged-critic in a child process.

Bounds of (1).  Copied words and the 0/1 words: exact.  Scaled words: the host forms each divisor in float32 (half an ulp), the device
divides or multiplies once or twice (half an ulp each): at most 1.5 ulps of the result, bound 2.  Rotated words: a float32
quaternion product, the quaternion-to-matrix formula and a three-term dot product are about ten roundings of 6e-8 relative to
max(1, |v|): bound 1e-5 max(1, |v|), a tenfold margin."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from openroborl_amd import _abi
from openroborl_amd import env as envmod
from tests.gpu_kit import mixed_env, short_episodes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.25
PAD = 5
PUSH = dict(prob=1.0, lin_vel=(0.1, 0.4), lin_vel_z=0.1, ang_vel=0.3)
F = envmod.PRIV_FIELDS


# ---- 1. the row --------------------------------------------------------------------------------------------------------------------
def priv_ref(env, done, contact=True, push=True):
    """The rows in float64 from what the device holds: env.state, env.contact_out, env.push_out (read back) and `done` (uint8 [N] or
    None), by the table of include/openroborl_hip.h"""
    lay, n = env.layout, env.num_robot
    st = env.state.detach().cpu().numpy()
    sti = st.view(np.int32)
    f = lambda name: st[:, lay.sl(name)].astype(np.float64)   # noqa: E731
    out = np.zeros((n, envmod.PRIV_DIM))
    iq = np.array([np.asarray(env.models[int(t)]["init_quat"], dtype=np.float32) for t in env.robot_type]).astype(np.float64)
    qi = np.concatenate([-iq[:, :3], iq[:, 3:]], axis=1) / (iq * iq).sum(axis=1, keepdims=True)
    x1, y1, z1, w1 = f("QUAT").T
    x0, y0, z0, w0 = qi.T
    x = x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0
    y = -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0
    z = x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0
    w = -x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)      # [N, 3, 3]
    down = np.tile(np.array([0.0, 0.0, -1.0]), (n, 1))
    for name, v in (("base_lin_vel", f("LINVEL")), ("base_ang_vel", f("ANGVEL")), ("gravity", down)):
        out[:, F[name]] = np.einsum("nji,nj->ni", R, v)             # R^T v
    out[:, 9] = f("POS")[:, 2]
    out[:, F["motor_strength"]] = f("STRENGTH")
    sim_dt = float(np.float32(env.cfg.sim_dt))
    out[:, 22] = f("LATENCY")[:, 0] / ((_abi.RING_DEPTH - 2) * sim_dt)
    out[:, 23] = f("FOOT_MU")[:, 0]
    out[:, F["knee_friction"]] = f("KNEE_FRICTION") * 20.0
    out[:, F["mass_ratio"]] = f("MASS_RATIO")
    out[:, F["inertia_ratio"]] = f("INERTIA_RATIO")
    live = np.zeros(n, dtype=bool) if done is None else (np.asarray(done) == 0)
    if contact and env.contact_out is not None:
        nsum = env.contact_out.cpu().numpy().reshape(n, 4, 4)[:, :, 0].astype(np.float64)
        out[:, F["foot_contact"]] = (nsum > 0) * live[:, None]
        out[:, F["foot_force"]] = nsum / (env.cfg.action_repeat * sim_dt) / 100.0 * live[:, None]
    if push and env.push_out is not None:
        out[:, F["push"]] = env.push_out.cpu().numpy()[:, :6].astype(np.float64) * live[:, None]
    ep, mx = sti[:, lay.sl("EP_STEP")][:, 0].astype(np.float64), sti[:, lay.sl("MAX_EP_STEPS")][:, 0].astype(np.float64)
    out[:, 46] = ep / np.maximum(mx, 1.0)
    return out


COPIED = list(range(10, 22)) + [23] + list(range(28, 32)) + list(range(40, 46))
FLAGS = list(range(32, 36))
SCALED = [9, 22] + list(range(24, 28)) + list(range(36, 40)) + [46]        # (word 9 is a copy too: 0 ulps is within 2)
ROTATED = list(range(0, 9))


def check_rows(got, want, done):
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got[:, COPIED], want[:, COPIED].astype(np.float32))
    assert np.array_equal(got[:, FLAGS], want[:, FLAGS].astype(np.float32))
    assert not got[:, 47].any()
    ended = np.ones(len(got), dtype=bool) if done is None else (np.asarray(done) != 0)
    assert not got[ended][:, 32:46].any()
    ulp = np.spacing(np.abs(want[:, SCALED]).astype(np.float32)).astype(np.float64)
    err = np.abs(got[:, SCALED].astype(np.float64) - want[:, SCALED])
    print("scaled words: largest error %.2f ulps" % float((err / ulp).max()))
    assert (err <= 2.0 * ulp).all(), (err / ulp).max()
    for a in (0, 3, 6):
        v = np.linalg.norm(want[:, a:a + 3], axis=1, keepdims=True)
        e = np.abs(got[:, a:a + 3].astype(np.float64) - want[:, a:a + 3])
        print("rotated words %d..%d: largest error %.2e of max(1, |v|)" % (a, a + 2, float((e / np.maximum(1.0, v)).max())))
        assert (e <= 1e-5 * np.maximum(1.0, v)).all(), (a, e.max())


@pytest.mark.parametrize("n", [5, 64 + 3])
def test_privileged_row_matches_float64(n):
    import torch
    env = mixed_env(n, seed=3, auto_reset=True, contact_outputs=True, push=PUSH, push_outputs=True, config_overrides=short_episodes())
    assert len(set(env.robot_type.tolist())) == 2
    buf = torch.full((n + PAD, envmod.PRIV_DIM), SENTINEL, device=env.device)
    rng = np.random.RandomState(n)
    env.reset()
    got = env.privileged_obs(out=buf[:n], done=None)
    assert got.data_ptr() == buf.data_ptr()
    check_rows(buf[:n].cpu().numpy(), priv_ref(env, None), None)
    seen_done = seen_live = seen_contact = seen_push = 0
    for k in range(40):
        act = torch.from_numpy(rng.uniform(-0.1, 0.1, (n, 12)).astype(np.float32)).to(env.device)
        _, _, done, _ = env.step(act)
        env.privileged_obs(out=buf[:n], done=done)
        d = done.cpu().numpy()
        rows = buf[:n].cpu().numpy()
        check_rows(rows, priv_ref(env, d), d)
        seen_done += int((d != 0).sum()); seen_live += int((d == 0).sum())
        seen_contact += int((rows[:, 32:36] == 1.0).sum()); seen_push += int((rows[:, 40:46] != 0.0).sum())
    # episodes ended (and restarted: the row is the new episode's), and the live rows carried contacts and pushes
    assert seen_done >= 1 and seen_live >= 1 and seen_contact >= 1 and seen_push >= 1, (seen_done, seen_live, seen_contact, seen_push)
    assert bool((buf[n:] == SENTINEL).all())                         # rows beyond N are not written
    # a fresh output tensor; the argument checks of step_into
    fresh = env.privileged_obs(done=done)
    assert torch.equal(fresh, buf[:n])
    for bad in (dict(out=buf[:n].double()), dict(out=buf[:n + 1]), dict(out=buf[:n, :47]), dict(out=buf[:n].t().contiguous().t()),
                dict(done=done.bool()), dict(done=done[:n - 1]), dict(out=buf[:n].cpu())):
        with pytest.raises(ValueError):
            env.privileged_obs(**bad)
    env.close()


def test_privileged_row_unbound_cases():
    n = 9
    env = mixed_env(n, seed=4, auto_reset=True, config_overrides=short_episodes())
    import torch
    rng = np.random.RandomState(0)
    env.reset()
    for k in range(3):
        _, _, done, _ = env.step(torch.from_numpy(rng.uniform(-0.1, 0.1, (n, 12)).astype(np.float32)).to(env.device))
    d = done.cpu().numpy()
    assert not d.any()
    rows = env.privileged_obs(done=done).cpu().numpy()               # nothing bound: zeros in both groups
    assert not rows[:, 32:46].any()
    check_rows(rows, priv_ref(env, d), d)
    env.bind_contact_outputs(True)                                   # contacts only
    _, _, done, _ = env.step(torch.zeros(n, 12, device=env.device))
    rows = env.privileged_obs(done=done).cpu().numpy()
    assert rows[:, 32:36].any() and rows[:, 36:40].any() and not rows[:, 40:46].any()
    check_rows(rows, priv_ref(env, done.cpu().numpy()), done.cpu().numpy())
    rows = env.privileged_obs(done=None).cpu().numpy()               # done == NULL: zeros whatever is bound
    assert not rows[:, 32:46].any()
    check_rows(rows, priv_ref(env, None), None)
    env.bind_contact_outputs(False)
    env.bind_push_outputs(True)                                      # push outputs only (prob 0: the rows hold what a step wrote)
    env.set_push(PUSH)
    _, _, done, _ = env.step(torch.zeros(n, 12, device=env.device))
    rows = env.privileged_obs(done=done).cpu().numpy()
    assert rows[:, 40:46].any() and not rows[:, 32:40].any()
    check_rows(rows, priv_ref(env, done.cpu().numpy()), done.cpu().numpy())
    env.close()


def test_privileged_obs_refusals_write_nothing():
    import torch
    n = 6
    env = mixed_env(n, seed=4)
    env.reset()
    L = env.L
    buf = torch.full((n + 1, envmod.PRIV_DIM), SENTINEL, device=env.device)
    done = torch.zeros(n, dtype=torch.uint8, device=env.device)
    st = env._stream()
    assert L.orr_privileged_obs(None, done.data_ptr(), buf.data_ptr(), st) != 0 and b"null handle" in L.orr_last_error()
    assert L.orr_privileged_obs(env.h, done.data_ptr(), None, st) != 0 and b"null buffer" in L.orr_last_error()
    assert L.orr_privileged_obs(env.h, done.data_ptr(), buf.data_ptr() + 4, st) != 0 and b"16-byte aligned" in L.orr_last_error()
    h = C.c_void_p()
    assert L.orr_create(C.byref(env.cfg), C.byref(h)) == 0           # a handle with no state bound
    assert L.orr_privileged_obs(h, done.data_ptr(), buf.data_ptr(), st) != 0 and b"not bound" in L.orr_last_error()
    L.orr_destroy(h)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert L.orr_privileged_obs(env.h, done.data_ptr(), buf.data_ptr(), st) == 0       # and the same call with everything in place
    torch.cuda.synchronize()
    assert bool((buf[:n] != SENTINEL).all()) and bool((buf[n:] == SENTINEL).all())
    env.close()


# ---- 2. the forward pass -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    """A privileged model with random weights and biases, its fused copy, and the plain model with the same actor and the first 160
    rows of the critic's layer 0"""
    import torch
    from openroborl_amd import policy_hip, ppo
    dev = torch.device("cuda", 0)
    model = ppo.ActorCritic(dev, seed=3, priv_dim=48)
    with torch.no_grad():
        for k, v in model.p.items():
            if k.endswith("/b:0"):
                v.copy_(torch.randn(v.shape, generator=torch.Generator().manual_seed(len(k))).to(dev) * 0.1)
        model.p["model/pi/w:0"].mul_(30.0)
    plain = {k: v.detach().clone() for k, v in model.p.items()}
    plain["model/vf_fc0/w:0"] = model.p["model/vf_fc0/w:0"].detach()[:160].clone()
    return model, policy_hip.FusedActorCritic(model.p, dev, std=0.125), policy_hip.FusedActorCritic(plain, dev, std=0.125)


def value64(p, obs, priv):
    import torch
    x = torch.cat((obs, priv), dim=1).double()
    h = torch.relu(x @ p["model/vf_fc0/w:0"].double() + p["model/vf_fc0/b:0"].double())
    h = torch.relu(h @ p["model/vf_fc1/w:0"].double() + p["model/vf_fc1/b:0"].double())
    return (h @ p["model/vf/w:0"].double() + p["model/vf/b:0"].double())[:, 0]


def raw_forward(fused, obs, priv, noise, n, guard=16):
    """The C entry point with the test's own output buffers: n rows + a guard band in each"""
    import torch
    dev = obs.device
    outs = [torch.full((n + guard, c), SENTINEL, device=dev) for c in (12, 12, 1, 12)]      # action, raw, value, mean
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if priv is None:
        rc = fused.L.orr_policy_forward(C.byref(fused.net), obs.data_ptr(), n, noise.data_ptr(), 0.125, 2.0 * math.pi, outs[0].data_ptr(),
                                        outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), st)
    else:
        rc = fused.L.orr_policy_forward_priv(C.byref(fused.net), obs.data_ptr(), priv.data_ptr(), n, noise.data_ptr(), 0.125, 2.0 * math.pi,
                                             outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), st)
    assert rc == 0, fused.L.orr_last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o[n:] == SENTINEL).all())                      # rows beyond n are not written
    return [o[:n] for o in outs]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_forward_priv(nets, n):
    import torch
    model, fused, fused_plain = nets
    assert fused.priv_dim == 48 and fused_plain.priv_dim == 0
    dev = model.device
    g = torch.Generator(device=dev).manual_seed(100 + n)
    obs = torch.randn(n, 160, generator=g, device=dev) * 2.0
    priv = torch.randn(n, 48, generator=g, device=dev) * 2.0
    noise = torch.randn(n, 12, generator=g, device=dev)
    act, raw, val, mean = raw_forward(fused, obs, priv, noise, n)
    act0, raw0, val0, mean0 = raw_forward(fused_plain, obs, None, noise, n)
    # the actor: the same code on the same inputs
    assert torch.equal(act, act0) and torch.equal(raw, raw0) and torch.equal(mean, mean0)
    v64 = value64(model.p, obs, priv).detach()
    err = float((val[:, 0].double() - v64).abs().max())
    print("n = %d: value error %.2e of the bound %.2e" % (n, err, 2e-5 * max(1.0, float(v64.abs().max()))))
    assert err < 2e-5 * max(1.0, float(v64.abs().max()))
    # through the Python layer: the same numbers, and the vector is required
    a2, r2, v2, m2 = fused.forward(obs, noise, want_mean=True, priv=priv)
    assert torch.equal(a2, act) and torch.equal(r2, raw) and torch.equal(v2, val[:, 0]) and torch.equal(m2, mean)
    with pytest.raises(ValueError):
        fused.forward(obs, noise)
    with pytest.raises(ValueError):
        fused_plain.forward(obs, noise, priv=priv)
    with pytest.raises(ValueError):
        fused.forward(obs, noise, priv=priv[:, :47].contiguous())
    # obs zeroed and ONE privileged column set: the value moves as the float64 MLP says (a transposed or shifted tile would not)
    zero = torch.zeros_like(obs)
    for col in (0, 17, 47):
        one = torch.zeros_like(priv)
        one[:, col] = torch.linspace(-2.0, 2.0, n, device=dev) if n > 1 else 1.5
        v = raw_forward(fused, zero, one, noise, n)[2][:, 0]
        w64 = value64(model.p, zero, one)
        assert float((v.double() - w64).abs().max()) < 2e-5 * max(1.0, float(w64.abs().max())), col
        base = value64(model.p, zero, torch.zeros_like(priv))
        assert n == 1 or float((w64 - base).abs().max()) > 1e-3                  # the column matters


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_forward_priv_with_zero_privileged_rows_is_the_plain_value(nets, n):
    import torch
    from openroborl_amd import policy_hip
    model, _, fused_plain = nets
    dev = model.device
    p = {k: v.detach().clone() for k, v in model.p.items()}
    p["model/vf_fc0/w:0"][160:] = 0.0
    fused0 = policy_hip.FusedActorCritic(p, dev, std=0.125)
    g = torch.Generator(device=dev).manual_seed(200 + n)
    obs = torch.randn(n, 160, generator=g, device=dev) * 2.0
    priv = torch.randn(n, 48, generator=g, device=dev) * 2.0
    noise = torch.randn(n, 12, generator=g, device=dev)
    val = raw_forward(fused0, obs, priv, noise, n)[2]
    val0 = raw_forward(fused_plain, obs, None, noise, n)[2]
    assert bool((val == val0).all())                                # ==: a signed zero does not matter


# ---- 3. the rollout ------------------------------------------------------------------------------------------------------------------
def test_graph_rollout_with_a_privileged_critic():
    """The eager first segment and the replayed second one equal collect_rollout on a twin env with the same noise; priv[k + 1] is
    env.privileged_obs(done=dones[k]) of a third twin stepped with the same actions."""
    import torch
    from openroborl_amd import ppo, rollout
    dev = torch.device("cuda:0")
    n, T = 64, 4
    kw = dict(seed=11, auto_reset=True, contact_outputs=True, push=PUSH, push_outputs=True, config_overrides=short_episodes())
    envs = [mixed_env(n, **kw) for _ in range(3)]
    models = [ppo.ActorCritic(dev, seed=1, priv_dim=48).enable_fused() for _ in range(2)]
    collector = rollout.GraphRollout(envs[1], models[1], T)
    obs = [e.reset() for e in envs]
    priv = [None, None]
    gen = torch.Generator(device=dev).manual_seed(0)
    ended = 0
    for seg in range(3):
        noise = torch.randn(T, n, 12, device=dev, generator=gen)
        a = rollout.collect_rollout(envs[0], models[0], T, obs=obs[0], noise=noise, priv=priv[0])
        b = collector.collect(obs[1], noise=noise, priv=priv[1])
        for k in ("obs", "actions", "rewards", "dones", "vpred", "last_obs", "priv", "last_priv"):
            assert torch.equal(a[k], b[k]), (seg, k)
        np.testing.assert_allclose(b["logp"].cpu().numpy(), a["logp"].cpu().numpy(), rtol=1e-6, atol=1e-5)
        assert tuple(b["priv"].shape) == (T, n, 48) and tuple(b["last_priv"].shape) == (n, 48)
        # the third twin: the same clipped actions, the row recomputed after every step
        assert torch.equal(envs[2].privileged_obs(done=None) if seg == 0 else b["priv"][0], b["priv"][0])
        for k in range(T):
            _, _, done, _ = envs[2].step(b["actions"][k].clamp(-2.0 * math.pi, 2.0 * math.pi).contiguous())
            want = envs[2].privileged_obs(done=done)
            assert torch.equal(want, b["priv"][k + 1] if k + 1 < T else b["last_priv"]), (seg, k)
        ended += int(b["dones"].sum())
        obs = [a["last_obs"], b["last_obs"]]
        priv = [a["last_priv"].clone(), b["last_priv"]]
        with torch.no_grad():                       # "the learner" moves the weights; both policies are told so
            for m in models:
                for k2 in sorted(m.p):
                    m.p[k2].mul_(1.01)
                m.mark_updated()
    assert collector.graph is not None and ended >= 1
    assert torch.equal(envs[0].state.view(torch.int32), envs[1].state.view(torch.int32))
    for e in envs:
        e.close()


# ---- 4. the learner ------------------------------------------------------------------------------------------------------------------
def batch(dev, B, seed, model, margin=0.0):
    """tests/test_gpu_learner.py's synthetic batch + privileged observations.  margin > 0: only samples none of whose critic
    pre-activations (float64) lies within `margin` of the ReLU's kink - what a comparison of gradients across precisions presumes (a
    unit on the kink has derivative 0 in one precision and 1 in the other, and its whole column of the weight gradient differs by that
    sample's share)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    obs, priv = torch.randn(2 * B, 160, generator=g), torch.randn(2 * B, 48, generator=g)
    if margin > 0.0:
        p = {k: v.detach().cpu().double() for k, v in model.p.items()}
        z0 = torch.cat((obs, priv), dim=1).double() @ p["model/vf_fc0/w:0"] + p["model/vf_fc0/b:0"]
        z1 = torch.relu(z0) @ p["model/vf_fc1/w:0"] + p["model/vf_fc1/b:0"]
        keep = (z0.abs().min(dim=1).values > margin) & (z1.abs().min(dim=1).values > margin)
        assert int(keep.sum()) >= B
        obs, priv = obs[keep], priv[keep]
    obs, priv = obs[:B].to(dev), priv[:B].to(dev)
    with torch.no_grad():
        mu = model.mean(obs)
    act = mu + 0.125 * torch.randn(B, 12, generator=g).to(dev)
    shifted = mu + 0.04 * torch.randn(B, 12, generator=g).to(dev)
    old = (-0.5 * ((act - shifted) ** 2) / 0.125 ** 2 - 0.5 * math.log(2.0 * math.pi * 0.125 ** 2)).sum(dim=1)
    adv = torch.randn(B, generator=g).to(dev)
    adv[::97] = 0.0
    ret = torch.randn(B, generator=g).to(dev)
    return obs, priv, act, old, adv, ret


@pytest.mark.parametrize("graph,B,M", [(True, 512, 256), (False, 512, 256), (True, 8192, 4096)])
def test_fused_update_with_priv_matches_the_torch_learner(graph, B, M):
    """tests/test_gpu_learner.py::test_fused_update_matches_the_torch_learner with a privileged critic, at its tolerances.  M = 4096:
    the split weight gradients, part0_vf [16, 208, 512]."""
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    lr = 1e-4
    ref_model, model = ppo.ActorCritic(dev, seed=2, priv_dim=48), ppo.ActorCritic(dev, seed=2, priv_dim=48)
    obs, priv, act, old, adv, ret = batch(dev, B, 1, ref_model)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    ref = ppo.PPO(ref_model, lr=lr, minibatch=M)
    fused = learner_hip.FusedPPO(model, lr=lr, minibatch=M, use_graph=graph)
    P = fused._plan(B, M)
    assert tuple(P["priv"].shape) == (B, 48) and tuple(P["xv"].shape) == (M, 208)
    if M >= 4096:
        assert tuple(P["part0_vf"].shape) == (16, 208, 512) and tuple(P["part0_pi"].shape) == (16, 160, 512)
        assert P["n_jobs"] == 10 and P["jobs"][9].cols == 208 * 512 and P["jobs"][7].cols == 160 * 512
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
    assert float((model.p["model/vf_fc0/w:0"].detach()[160:] - before["model/vf_fc0/w:0"][160:]).abs().max()) > 0.5 * lr   # the privileged rows train
    with pytest.raises(ValueError):
        fused.update(obs, act, adv, ret, old_logp=old)
    # the rollout's fused forward pass sees the updated weights (views of the flat buffer)
    model.enable_fused()
    with torch.no_grad():
        _, _, v_fused = model.act(obs[:256], priv[:256], deterministic=True)
        np.testing.assert_allclose(v_fused.cpu().numpy(), model.value(obs[:256], priv[:256]).cpu().numpy(), atol=2e-5)


@pytest.mark.parametrize("B", [256, 4096])
def test_fused_gradient_with_priv_matches_float64_cpu(B):
    """The gradient of model/vf_fc0/w:0 (208 rows) from the hand-written backward against float64 autograd; B = 4096: through part0_vf."""
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    model = ppo.ActorCritic(dev, seed=4, priv_dim=48)
    obs, priv, act, old, adv, ret = batch(dev, B, 0, model, margin=1e-4)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.p.items()}
    vf64 = ((value64(p64, obs.cpu(), priv.cpu()) - ret.cpu().double()) ** 2).mean()
    vf64.backward()
    learner = learner_hip.FusedPPO(model, lr=1e-4, minibatch=B, use_graph=False)
    P = learner._plan(B, B)
    with torch.no_grad():
        P["obs"].copy_(obs)
        P["priv"].copy_(priv)
        P["aux"][:, :12], P["aux"][:, 12], P["aux"][:, 13], P["aux"][:, 14] = act, old, adv, ret
        P["perm"].copy_(torch.arange(B, device=dev))
        learner._minibatch(P, 0)
    assert abs(P["stats"][0, 1].item() - vf64.item()) < 2e-4 * max(1.0, abs(vf64.item()))
    for k in ("model/vf_fc0/w:0", "model/vf_fc0/b:0", "model/vf_fc1/w:0", "model/vf/w:0"):
        g32, g64 = learner.g[k].detach().cpu().double(), p64[k].grad
        scale = g64.abs().max().item() + 1e-12
        print("%s: gradient error %.2e of its scale" % (k, (g32 - g64).abs().max().item() / scale))
        assert (g32 - g64).abs().max().item() < 2e-3 * scale, (k, (g32 - g64).abs().max().item(), scale)
        cs = (g32 * g64).sum() / (g32.norm() * g64.norm() + 1e-30)
        assert cs.item() > 0.99999, (k, cs.item())
    assert float(p64["model/vf_fc0/w:0"].grad[160:].abs().max()) > 0.0


def test_fused_update_with_priv_is_reproducible_bit_for_bit():
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    B, M = 8192, 4096
    outs = []
    for _ in range(2):
        model = ppo.ActorCritic(dev, seed=3, priv_dim=48)
        obs, priv, act, old, adv, ret = batch(dev, B, 5, model)
        fused = learner_hip.FusedPPO(model, lr=1e-4, minibatch=M)
        gen = torch.Generator(device=dev); gen.manual_seed(0)
        fused.update(obs, act, adv, ret, old_logp=old, epochs=2, generator=gen, priv=priv)
        outs.append(fused.flat_p.clone())
    assert torch.equal(outs[0], outs[1])


# ---- 5. train.py ---------------------------------------------------------------------------------------------------------------------
def test_train_with_a_privileged_critic_runs_saves_and_evaluates(tmp_path):
    import json
    zip_path, log_path = str(tmp_path / "priv.zip"), str(tmp_path / "log.json")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--privileged-critic", "--num-robot", "64", "--horizon", "4", "--iters", "3",
           "--push", "0.05,0.2,0.5", "--save", zip_path, "--log", log_path]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    log = json.load(open(log_path))
    assert log and log[-1]["iter"] == 2
    for rec in log:
        assert math.isfinite(rec["surr"]) and math.isfinite(rec["vf"]) and math.isfinite(rec["mean_step_reward"])
    from openroborl_amd import policy as pol
    w = pol.load_parameters(zip_path)
    assert w["model/vf_fc0/w:0"].shape == (208, 512) and w["model/pi_fc0/w:0"].shape == (160, 512)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--eval", zip_path, "--num-robot", "16"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    rec = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert rec["robots"] == 16 and math.isfinite(rec["return_mean"])
