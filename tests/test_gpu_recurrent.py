"""The recurrent history student on the GPU, against the recurrence spelled out in float64 on the CPU; its learner, rollout, refusals, train.py."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, G, Z, F = 256, 768, 48, 32
CASES = [(1, 1), (1, 17), (3, 16), (6, 33)]
SENTINEL, PAD = -7.25, 64


def _weights(seed=11):
    """Scaled so that the pre-activations span roughly +-3: saturated gates alone would hide errors."""
    rng = np.random.default_rng(seed)
    return {"model/gru_x/w:0": rng.normal(0, 0.2, (F, G)), "model/gru_x/b:0": rng.normal(0, 0.3, G), "model/gru_h/w:0": rng.normal(0, 0.1, (H, G)),
            "model/gru_h/b:0": rng.normal(0, 0.3, G), "model/gru_out/w:0": rng.normal(0, 0.1, (H, Z)), "model/gru_out/b:0": rng.normal(0, 0.1, Z)}


def _inputs(T, n, seed=3):
    """obs, h0 and a starts pattern: robots 0, 3, .. start at t = 0, robots 1, 4, .. mid-sequence, the rest never."""
    rng = np.random.default_rng(seed + 100 * T + n)
    starts = np.zeros((T, n), dtype=np.uint8)
    starts[0, 0::3] = 1
    starts[T // 2, 1::3] = 1
    return rng.normal(0, 1, (T, n, 160)).astype(np.float32), starts, rng.uniform(-0.9, 0.9, (n, H)).astype(np.float32)


def _frame(obs):
    return np.concatenate((obs[..., 0:4], obs[..., 12:24], obs[..., 48:60], np.zeros(obs.shape[:-1] + (4,), obs.dtype)), axis=-1)


def _reference(W, obs, starts, h0, dtype):
    w = {k.split("/")[1][4:] + k[-3]: v.astype(dtype) for k, v in W.items()}       # xw, xb, hw, hb, outw, outb
    sig = lambda a: 1 / (1 + np.exp(-a))   # noqa: E731
    T, n = starts.shape
    h = np.zeros((n, H), dtype) if h0 is None else h0.astype(dtype)
    out = {k: [] for k in ("hid", "latent", "frames", "hprev", "saved")}
    for t in range(T):
        x = _frame(obs[t]).astype(dtype)
        hp = np.where(starts[t][:, None] != 0, dtype(0), h)
        gx, gh = x @ w["xw"] + w["xb"], hp @ w["hw"] + w["hb"]
        r, u, q = sig(gx[:, :H] + gh[:, :H]), sig(gx[:, H:2 * H] + gh[:, H:2 * H]), gh[:, 2 * H:]
        c = np.tanh(gx[:, 2 * H:] + r * q)
        h = (1 - u) * c + u * hp
        for k, v in (("hid", h), ("latent", h @ w["outw"] + w["outb"]), ("frames", x), ("hprev", hp), ("saved", np.stack((r, u, c, q), axis=1))):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _tolerance():
    """8 x the largest difference of the float32 numpy evaluation from the float64 one at the (6, 33) case."""
    obs, starts, h0 = _inputs(6, 33)
    a, b = _reference(_weights(), obs, starts, h0, np.float32), _reference(_weights(), obs, starts, h0, np.float64)
    return 8.0 * max(np.abs(a[k].astype(np.float64) - b[k]).max() for k in ("hid", "latent", "saved"))


def _guarded(shape, dev):
    """An output buffer between two pads of sentinels -> (the whole allocation, the view the kernel writes)."""
    import torch
    size = int(np.prod(shape))
    full = torch.full((2 * PAD + size,), SENTINEL, dtype=torch.float32, device=dev)
    return full, full[PAD:PAD + size].view(shape)


_pads_untouched = lambda full: bool((full[:PAD] == SENTINEL).all()) and bool((full[-PAD:] == SENTINEL).all())   # noqa: E731


def _encoder(dev, W=None):
    import torch
    from openroborl_amd import policy_hip
    return policy_hip.GruEncoder({k: torch.from_numpy(v.astype(np.float32)).to(dev) for k, v in (W or _weights()).items()}, dev)


def _forward(enc, dev, obs, starts, h0, names=("latent", "frames", "hprev", "saved")):
    import torch
    T, n = starts.shape
    shapes = {"hid": (T, n, H), "latent": (T, n, Z), "frames": (T, n, F), "hprev": (T, n, H), "saved": (T, n, 4, H)}
    bufs = {k: _guarded(shapes[k], dev) for k in ("hid",) + tuple(names)}
    enc.forward(torch.from_numpy(obs).to(dev), torch.from_numpy(starts).to(dev), None if h0 is None else torch.from_numpy(h0).to(dev),
                **{k: v[1] for k, v in bufs.items()})
    torch.cuda.synchronize()
    assert all(_pads_untouched(full) for full, _ in bufs.values())
    return {k: v[1].cpu().numpy() for k, v in bufs.items()}


@pytest.mark.parametrize("with_h0", [True, False])
@pytest.mark.parametrize("T,n", CASES)
def test_forward_matches_float64(T, n, with_h0):
    import torch
    dev = torch.device("cuda:0")
    obs, starts, h0 = _inputs(T, n)
    h0 = h0 if with_h0 else None
    got, want = _forward(_encoder(dev), dev, obs, starts, h0), _reference(_weights(), obs, starts, h0, np.float64)
    tol = _tolerance()
    for k in ("hid", "latent", "saved"):
        err = np.abs(got[k].astype(np.float64) - want[k]).max()
        print("T=%d n=%d h0=%s %s: error %.3e, tolerance %.3e" % (T, n, with_h0, k, err, tol))
        assert err < tol, (k, err, tol)
    assert np.array_equal(got["frames"], _frame(obs))                                   # exact copies
    assert np.array_equal(got["hprev"][0], np.where(starts[0][:, None] != 0, np.float32(0), np.zeros((n, H), np.float32) if h0 is None else h0))
    assert np.array_equal(got["hprev"][1:], np.where(starts[1:][:, :, None] != 0, np.float32(0), got["hid"][:-1]))


def test_chaining_determinism_and_optional_outputs():
    import torch
    dev = torch.device("cuda:0")
    T, n = 6, 33
    obs, starts, h0 = _inputs(T, n)
    enc = _encoder(dev)
    whole = _forward(enc, dev, obs, starts, h0)
    again = _forward(enc, dev, obs, starts, h0)
    assert all(np.array_equal(whole[k], again[k]) for k in whole)
    bare = _forward(enc, dev, obs, starts, h0, names=())
    only_latent = _forward(enc, dev, obs, starts, h0, names=("latent",))
    assert np.array_equal(bare["hid"], whole["hid"]) and all(np.array_equal(only_latent[k], whole[k]) for k in only_latent)
    h = torch.from_numpy(h0).to(dev)                                                     # six steps in place: hid is h0
    o, s = torch.from_numpy(obs).to(dev), torch.from_numpy(starts).to(dev)
    z = torch.empty((1, n, Z), device=dev)
    for t in range(T):
        enc.forward(o[t:t + 1], s[t:t + 1], h, hid=h.view(1, n, H), latent=z)
        assert np.array_equal(h.cpu().numpy(), whole["hid"][t]) and np.array_equal(z[0].cpu().numpy(), whole["latent"][t])


def _backward(dev, W, fwd, starts, g_latent):
    import torch
    from openroborl_amd import _abi, _lib
    L = _lib.load()
    T, n = starts.shape
    packed = []
    for w in (W["model/gru_h/w:0"].T, W["model/gru_out/w:0"].T):
        src = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(dev)
        packed.append(torch.empty(int(L.orr_policy_packed_size(*src.shape)), device=dev))
        _lib.check(L.orr_policy_pack(src.data_ptr(), src.shape[0], src.shape[1], packed[-1].data_ptr(), None), L)
    encT = _abi.OrrGruTransposed(packed[0].data_ptr(), packed[1].data_ptr())
    rows = _abi.gru_backward_rows(n)
    bufs = {"g_x": _guarded((T, n, G), dev), "g_h": _guarded((T, n, G), dev), "partials": _guarded((2, rows, G), dev)}
    ins = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (g_latent, fwd["saved"], fwd["hprev"], starts)]
    _lib.check(L.orr_gru_backward(C.byref(encT), *(x.data_ptr() for x in ins), T, n, *(bufs[k][1].data_ptr() for k in ("g_x", "g_h", "partials")), None), L)
    torch.cuda.synchronize()
    assert all(_pads_untouched(full) for full, _ in bufs.values())
    return {k: v[1].cpu().numpy() for k, v in bufs.items()}


def _close(got, want, name):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    scale = np.abs(want).max() + 1e-12
    assert np.abs(got - want).max() < 2e-3 * scale, (name, np.abs(got - want).max(), scale)
    assert got @ want / (np.linalg.norm(got) * np.linalg.norm(want) + 1e-30) > 0.99999, name


@pytest.mark.parametrize("T,n", [(3, 16), (6, 33)])
def test_backward_matches_float64_autograd(T, n):
    import torch
    dev = torch.device("cuda:0")
    W = _weights()
    obs, starts, h0 = _inputs(T, n)
    fwd = _forward(_encoder(dev), dev, obs, starts, h0)
    g_latent = np.random.default_rng(5).normal(0, 1, (T, n, Z)).astype(np.float32)
    got = _backward(dev, W, fwd, starts, g_latent)
    w = {k: torch.from_numpy(v) for k, v in W.items()}
    h, px, ph, loss = torch.from_numpy(h0).double(), [], [], 0.0
    for t in range(T):
        hp = torch.where(torch.from_numpy(starts[t] != 0)[:, None], torch.zeros_like(h), h)
        gx = (torch.from_numpy(_frame(obs[t])).double() @ w["model/gru_x/w:0"] + w["model/gru_x/b:0"]).requires_grad_(True)
        gh = hp @ w["model/gru_h/w:0"] + w["model/gru_h/b:0"]
        gh.requires_grad_(True).retain_grad()
        r, u = torch.sigmoid(gx[:, :H] + gh[:, :H]), torch.sigmoid(gx[:, H:2 * H] + gh[:, H:2 * H])
        h = (1 - u) * torch.tanh(gx[:, 2 * H:] + r * gh[:, 2 * H:]) + u * hp
        loss = loss + ((h @ w["model/gru_out/w:0"] + w["model/gru_out/b:0"]) * torch.from_numpy(g_latent[t]).double()).sum()
        px.append(gx), ph.append(gh)
    loss.backward()
    g_x, g_h = torch.stack([x.grad for x in px]).numpy(), torch.stack([x.grad for x in ph]).numpy()
    _close(got["g_x"], g_x, "g_x"), _close(got["g_h"], g_h, "g_h")
    _close(got["partials"][0].astype(np.float64).sum(0), g_x.sum((0, 1)), "d bx"), _close(got["partials"][1].astype(np.float64).sum(0), g_h.sum((0, 1)), "d bh")
    changed = g_latent.copy()                                # robots 1, 4, .. start at T // 2: nothing flows into the earlier steps
    changed[T // 2:, 1::3] += 1.0
    other = _backward(dev, W, fwd, starts, changed)
    assert np.array_equal(other["g_x"][:T // 2, 1::3], got["g_x"][:T // 2, 1::3]) and not np.array_equal(other["g_x"][T // 2:, 1::3], got["g_x"][T // 2:, 1::3])


def _student(dev, seed):
    from openroborl_amd import ppo
    return ppo.ActorCritic(dev, priv_dim=48, actor_priv_dim=48, recurrent=256, seed=seed)


def _segment(dev, T, N, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    starts = torch.rand((T, N), generator=g) < 0.15
    starts[0, ::2] = True
    return (torch.randn((T, N, 160), generator=g).to(dev), starts.to(dev), (torch.rand((N, H), generator=g) - 0.5).to(dev),
            torch.randn((T, N, Z), generator=g).to(dev))


def test_learner_gradient_matches_float64_cpu():
    import torch
    from openroborl_amd import history, learner_hip
    dev = torch.device("cuda:0")
    T, N = 4, 33
    model = _student(dev, 4)
    obs, starts, h0, target = _segment(dev, T, N, 0)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.p.items() if k.startswith("model/gru_")}
    _, z = history.encode_seq(p64, obs.cpu().double(), starts.cpu(), h0.cpu().double())
    loss64 = ((z - target.cpu().double()) ** 2).sum(dim=-1).mean()
    loss64.backward()
    learner = learner_hip.FusedDistillRecurrent(model, lr=1e-4, minibatch=T * N, use_graph=False)
    learner.T, learner.minibatch = T, N
    P = learner._plan(N, N)
    with torch.no_grad():
        P["obs"].copy_(obs), P["starts"].copy_(starts.view(torch.uint8)), P["h0"].copy_(h0), P["target"].copy_(target)
        P["perm"].copy_(torch.arange(N, device=dev))
        learner._minibatch(P, 0)
    assert abs(P["stats"][0, 0].item() - loss64.item()) < 2e-4 * max(1.0, abs(loss64.item()))
    for k in sorted(p64):
        _close(learner.g[k].detach().cpu().numpy(), p64[k].grad.numpy(), k)


@pytest.mark.parametrize("graph", [False, True])
def test_learner_matches_the_torch_learner(graph):
    """test_fused_update_matches_the_torch_learner's construction: same parameters, data and robot permutations."""
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    T, N, M, lr = 8, 256, 1024, 1e-4
    ref_model, model = _student(dev, 2), _student(dev, 2)
    obs, starts, h0, target = _segment(dev, T, N, 1)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    ref = ppo.DistillRecurrent(ref_model, lr=lr, minibatch=M)
    fused = learner_hip.FusedDistillRecurrent(model, lr=lr, minibatch=M, use_graph=graph)
    for it in range(2):
        g1, g2 = torch.Generator(device=dev), torch.Generator(device=dev)
        g1.manual_seed(10 + it), g2.manual_seed(10 + it)
        s_ref = ref.update(obs, starts, h0, target, epochs=2, generator=g1)
        s_fused = fused.update(obs, starts, h0, target, epochs=2, generator=g2)
        np.testing.assert_allclose(s_fused, s_ref, rtol=2e-4, atol=2e-5)
    steps = 2 * 2 * (N * T // M)
    assert fused.steps_taken() == steps
    for k in sorted(before):
        a, b = ref_model.p[k].detach(), model.p[k].detach()
        if k.startswith("model/gru_"):
            assert (a - before[k]).abs().max().item() > 2 * lr and (a - b).abs().max().item() < steps * lr, (k, (a - b).abs().max().item())
        else:
            assert torch.equal(b, before[k])             # the teacher's nets are frozen


def test_rollout_carries_the_hidden_state():
    """Graph and eager collectors agree bit for bit; an ended episode's next state is what a zero state gives."""
    import torch
    from openroborl_amd import rollout
    from tests import gpu_kit
    dev = torch.device("cuda:0")
    T, n, runs = 6, 64, []
    for graph in (True, False):
        env = gpu_kit.mixed_env(n, seed=11, auto_reset=True, contact_outputs=True, config_overrides=gpu_kit.short_episodes())
        policy = _student(dev, 7).enable_fused()
        gen = torch.Generator(device=dev).manual_seed(1)
        collector = rollout.GraphRollout(env, policy, T) if graph else None
        obs, hidden, start, segs = env.reset(), None, None, []
        for _ in range(3):                                   # eager, capture, replay
            noise = torch.randn((T, n, 12), device=dev, generator=gen)
            buf = collector.collect(obs, noise=noise, hidden=hidden, start=start) if graph else rollout.collect_rollout(env, policy, T, obs=obs, noise=noise,
                                                                                                                       hidden=hidden, start=start)
            segs.append({k: buf[k].clone() for k in ("actions", "hidden", "last_hidden", "starts", "dones", "hid", "obs")})
            obs, hidden, start = buf["last_obs"].clone(), segs[-1]["last_hidden"], segs[-1]["dones"][-1]
        runs.append(segs)
    ended = 0
    for a, b in zip(*runs):
        assert all(torch.equal(a[k], b[k]) for k in ("actions", "hidden", "last_hidden", "starts"))
        assert torch.equal(a["starts"][1:], a["dones"][:-1])
        for k in range(T - 1):
            rows = a["dones"][k].nonzero().flatten()
            if len(rows):
                zero = policy.fused.gru.forward(a["obs"][k + 1][rows].contiguous().view(1, -1, 160))
                assert torch.equal(zero[0], a["hid"][k + 1][rows])
                ended += len(rows)
    assert ended > 0


def _raw_args(dev):
    import torch
    from openroborl_amd import _abi, _lib
    L = _lib.load()
    T, n = 2, 17
    enc = _encoder(dev)
    f = lambda *shape: _guarded(shape, dev)   # noqa: E731
    wt = torch.zeros(int(L.orr_policy_packed_size(G, H)), device=dev)
    keep = {"enc": enc, "wt": wt, "encT": _abi.OrrGruTransposed(wt.data_ptr(), wt.data_ptr()),
            "bufs": {k: f(*s) for k, s in (("obs", (T, n, 160)), ("h0", (n, H)), ("hid", (T, n, H)), ("latent", (T, n, Z)), ("frames", (T, n, F)),
                                           ("hprev", (T, n, H)), ("saved", (T, n, 4, H)), ("g_latent", (T, n, Z)), ("g_x", (T, n, G)), ("g_h", (T, n, G)),
                                           ("partials", (2, _abi.gru_backward_rows(n), G)))},
            "starts": torch.zeros((T, n), dtype=torch.uint8, device=dev)}
    p = {k: v[1].data_ptr() for k, v in keep["bufs"].items()}
    p.update(starts=keep["starts"].data_ptr(), T=T, n=n)
    return L, keep, p


REFUSALS = [("forward", {"obs": None}), ("forward", {"hid": None}), ("forward", {"T": 0}), ("forward", {"n": 0}), ("forward", {"starts": None}),
            ("forward", {"hid": +4}), ("forward", {"saved": +4}), ("forward", {"latent": +2}), ("forward", {"hprev": "hid"}), ("forward", {"h0": "hid"}),
            ("forward", {"frames": "obs"}), ("backward", {"g_x": None}), ("backward", {"starts": None}), ("backward", {"T": 0}), ("backward", {"n": -1}),
            ("backward", {"g_x": +4}), ("backward", {"partials": +2}), ("backward", {"g_h": "g_x"}), ("backward", {"g_x": "saved"})]


@pytest.mark.parametrize("entry,change", REFUSALS)
def test_entry_points_refuse(entry, change):
    """None: a null pointer; an integer on a pointer: that many bytes off; a name: the other buffer's address (an overlap)."""
    import torch
    dev = torch.device("cuda:0")
    L, keep, p = _raw_args(dev)
    for k, v in change.items():
        p[k] = v if (v is None or k in ("T", "n")) else (p[v] if isinstance(v, str) else p[k] + v)
    if entry == "forward":
        rc = L.orr_gru_forward(C.byref(keep["enc"].enc), p["obs"], p["starts"], p["h0"], p["T"], p["n"], p["hid"], p["latent"], p["frames"], p["hprev"],
                               p["saved"], None)
    else:
        rc = L.orr_gru_backward(C.byref(keep["encT"]), p["g_latent"], p["saved"], p["hprev"], p["starts"], p["T"], p["n"], p["g_x"], p["g_h"],
                                p["partials"], None)
    torch.cuda.synchronize()
    assert rc < 0 and L.orr_last_error()
    assert all(bool((full == SENTINEL).all()) for full, _ in keep["bufs"].values())


def test_model_and_train_refuse():
    import torch
    from openroborl_amd import ppo
    from tests import gpu_kit
    dev = torch.device("cuda:0")
    for kw in ({"actor_priv_dim": 48, "history": 16}, {}, {"actor_priv_dim": 48, "obs_norm": True}):
        with pytest.raises(ValueError):
            ppo.ActorCritic(dev, priv_dim=48, recurrent=256, **kw)
    gpu_kit.train_refuses(["--recurrent", "--num-robot", "64", "--iters", "1"], "--recurrent belongs to --distill")


def test_train_distills_a_recurrent_student(tmp_path):
    import json
    from tests import gpu_kit
    teacher, student, log_path = str(tmp_path / "teacher.zip"), str(tmp_path / "student.zip"), str(tmp_path / "log.json")
    common = ["--num-robot", "64", "--horizon", "8", "--push", "0.05,0.2,0.5"]
    gpu_kit.run_train("--privileged-actor", "--iters", "1", "--save", teacher, *common)
    gpu_kit.run_train("--distill", teacher, "--recurrent", "--iters", "3", "--save", student, "--log", log_path, *common)
    log = json.load(open(log_path))
    assert log[-1]["iter"] == 2 and all(np.isfinite(rec["latent_loss"]) and rec["latent_loss"] > 0.0 for rec in log)
    rec = json.loads(gpu_kit.run_train("--eval", student, "--num-robot", "16").strip().splitlines()[-1])
    assert rec["robots"] == 16 and np.isfinite(rec["return_mean"])
