"""The forward layers of the fused learners on the matrix cores (csrc/orr_learner_forward.hip: orr_dense_forward) against float64 numpy on
the float32 inputs, against the rollout's forward kernels bit for bit, its refusals, and through the learners (hip_forward=True).
The float64 bound per element is (k + 2) U (|in| . |W| + |b|), U = 2^-24: k fused multiply-adds and one addition in any rounding pass a
term through at most k + 1 roundings, gamma_{k+1} <= (k + 2) U since (k + 1)^2 U < 1 for k <= 512; ReLU is 1-Lipschitz and exact."""
import numpy as np
import pytest

from tests import learner_refs as lr
from tests.gpu_kit import EPS as U
from tests.test_gpu_learner_gemm import SENT, _kit, _same_parameters

pytestmark = pytest.mark.gpu
SHAPES = [(160, 0, 512, 1), (160, 48, 512, 1), (512, 0, 256, 1), (256, 0, 48, 0), (256, 0, 12, 0), (256, 0, 1, 0)]


def _dense(L, st, xa, xb, w, b, relu, y, ra=None, rb=None, x_out=None, m=None):
    """orr_dense_forward on torch tensors (None: a NULL pointer); returns the code"""
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    return L.orr_dense_forward(ptr(xa), xa.shape[1], ptr(ra), ptr(xb), 0 if xb is None else xb.shape[1], ptr(rb), y.shape[0] if m is None else m,
                               ptr(w), ptr(b), w.shape[1], relu, ptr(y), ptr(x_out), st)


@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("m", [1, 17, 1000])
@pytest.mark.parametrize("ka,kb,n,relu", SHAPES)
def test_dense_forward_matches_float64(ka, kb, n, relu, m, tables):
    """m: one row; one row past a 16-row fragment; no multiple of any tile.  tables: indices with repeats into sources taller than m."""
    torch, _abi, L, dev, st = _kit()
    rng = np.random.RandomState(1000 * (ka + kb) + n + m)
    k, tall = ka + kb, m + 9 if tables else m
    xa, xb, w, b = lr.mixed(rng, tall, ka), (lr.mixed(rng, tall, kb) if kb else None), lr.mixed(rng, k, n), lr.mixed(rng, n)
    ra, rb = (rng.randint(0, tall, m).astype(np.int64), rng.randint(0, tall, m).astype(np.int64)) if tables else (np.arange(m), np.arange(m))
    if tables:
        ra[-1], rb[-1] = ra[0], rb[0]                                   # a repeat for every m > 1
    xin = np.concatenate([xa[ra]] + ([xb[rb]] if kb else []), axis=1)
    d = {name: (None if a is None else torch.from_numpy(a).to(dev)) for name, a in (("xa", xa), ("xb", xb), ("w", w), ("b", b))}
    tabs = dict(ra=torch.from_numpy(ra).to(dev), rb=torch.from_numpy(rb).to(dev) if kb else None) if tables else {}
    runs = []
    for _ in range(2):
        y, x_out = torch.full((m + 2, n), SENT, device=dev), torch.full((m + 2, k), SENT, device=dev)      # sentinel rows behind both
        assert _dense(L, st, d["xa"], d["xb"], d["w"], d["b"], relu, y, x_out=x_out, m=m, **tabs) == 0, L.orr_last_error()
        runs.append((y.cpu().numpy(), x_out.cpu().numpy()))
    y, x_out = runs[0]
    assert (y[m:] == SENT).all() and (x_out[m:] == SENT).all()
    assert np.array_equal(lr.bits(x_out[:m]), lr.bits(xin))
    assert all(np.array_equal(lr.bits(a), lr.bits(c)) for a, c in zip(runs[0], runs[1]))
    x64, w64, b64 = xin.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    ref = x64 @ w64 + b64
    ratio = lr.ratio_of(y[:m], np.maximum(ref, 0.0) if relu else ref, (k + 2) * U * (np.abs(x64) @ np.abs(w64) + np.abs(b64)))
    print("ka %d kb %d n %d m %d tables %d: error / bound %.3f" % (ka, kb, n, m, tables, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("kind", ["plain", "teacher", "history"])
def test_dense_forward_chain_gives_the_rollouts_bits(kind):
    """33 rows: two full workgroups of the forward kernel and one row.  The chain of orr_dense_forward calls on the unpacked weights against
    orr_policy_forward / _teacher / _history: mean, value and (history) latent, bit for bit."""
    torch, _abi, L, dev, st = _kit()
    from openroborl_amd import ppo
    n = 33
    model = ppo.ActorCritic(dev, seed=3, **{"plain": {}, "teacher": dict(priv_dim=48, actor_priv_dim=48),
                                           "history": dict(priv_dim=48, actor_priv_dim=48, history=16)}[kind])
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for key in sorted(model.p):
            if key.endswith("/b:0"):
                model.p[key].add_(0.1 * torch.randn(model.p[key].shape, generator=g).to(dev))
    obs, priv, hist = (torch.randn(n, c, generator=g).to(dev) for c in (160, 48, 512))
    p = {key: v.detach() for key, v in model.p.items()}

    def chain(names, xa, xb, widths):
        for i, (name, width) in enumerate(zip(names, widths)):
            y = torch.empty(n, width, device=dev)
            last = i == len(names) - 1
            assert _dense(L, st, xa, xb, p["model/%s/w:0" % name], p["model/%s/b:0" % name], 0 if last else 1, y) == 0, L.orr_last_error()
            xa, xb = y, None
        return xa

    model.enable_fused()
    latent = torch.empty(n, 48, device=dev)
    more = {"plain": {}, "teacher": dict(priv=priv), "history": dict(hist=hist, out_latent=latent)}[kind]
    _, _, value, mean = model.fused.forward(obs, want_mean=True, **more)
    xb = {"plain": None, "teacher": priv, "history": None}[kind]
    if kind == "history":
        xb = chain(("enc_fc0", "enc_fc1"), hist, None, (256, 48))
        assert torch.equal(xb.view(torch.int32), latent.view(torch.int32))
    assert torch.equal(chain(("pi_fc0", "pi_fc1", "pi"), obs, xb, (512, 256, 12)).view(torch.int32), mean.view(torch.int32))
    assert torch.equal(chain(("vf_fc0", "vf_fc1", "vf"), obs, xb, (512, 256, 1)).view(torch.int32), value.view(n, 1).view(torch.int32))


@pytest.mark.parametrize("bad", ["null", "m", "ka", "kb", "n", "align", "xb without kb", "kb without xb", "y on w", "x_out on xa", "x_out on y"])
def test_refused_calls_write_nothing(bad):
    torch, _abi, L, dev, st = _kit()
    m, ka, kb, n = 32, 32, 16, 32
    xa, xb, w, b = torch.zeros(m, ka, device=dev), torch.zeros(m, kb, device=dev), torch.zeros(ka + kb, n, device=dev), torch.zeros(n, device=dev)
    y, x_out = torch.full((m, n), SENT, device=dev), torch.full((m, ka + kb), SENT, device=dev)
    a = dict(xa=xa.data_ptr(), ka=ka, ra=None, xb=xb.data_ptr(), kb=kb, rb=None, m=m, w=w.data_ptr(), b=b.data_ptr(), n=n, relu=1, y=y.data_ptr(),
             x_out=x_out.data_ptr())
    a.update({"null": dict(w=None), "m": dict(m=0), "ka": dict(ka=24), "kb": dict(kb=8), "n": dict(n=40), "align": dict(xa=a["xa"] + 4),
              "xb without kb": dict(kb=0), "kb without xb": dict(xb=None), "y on w": dict(y=a["w"]), "x_out on xa": dict(x_out=a["xa"]),
              "x_out on y": dict(x_out=a["y"])}[bad])
    assert L.orr_dense_forward(*(list(a.values()) + [st])) < 0 and b"orr_dense_forward" in L.orr_last_error()
    torch.cuda.synchronize()
    assert bool((y == SENT).all()) and bool((x_out == SENT).all()) and not bool(xa.any()) and not bool(w.any())


def test_fused_gradient_with_hip_forward_matches_float64_cpu():
    """test_fused_gradient_matches_float64_cpu's construction and thresholds at B = M = 1000 (no multiple of a tile), hip_forward=True."""
    import torch
    from openroborl_amd import learner_hip, ppo
    from tests.test_gpu_learner import _loss64, _synthetic_batch
    dev, B = torch.device("cuda:0"), 1000
    model = ppo.ActorCritic(dev, seed=4)
    obs, _, act, old, adv, ret = _synthetic_batch(dev, B, seed=0, model=model)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.p.items()}
    loss64, surr64, vf64 = _loss64(p64, obs.cpu().double(), act.cpu().double(), adv.cpu().double(), ret.cpu().double(), old.cpu().double())
    loss64.backward()
    learner = learner_hip.FusedPPO(model, lr=1e-4, minibatch=B, hip_forward=True, use_graph=False)
    P = learner._plan(B, B)
    with torch.no_grad():
        P["obs"].copy_(obs)
        P["aux"][:, :12], P["aux"][:, 12], P["aux"][:, 13], P["aux"][:, 14] = act, old, adv, ret
        P["perm"].copy_(torch.arange(B, device=dev))
        learner._minibatch(P, 0)
    assert torch.equal(P["x"], obs)                                     # layer 0 left the gathered input for the weight gradient
    assert abs(P["stats"][0, 0].item() - surr64.item()) < 2e-4 * max(1.0, abs(surr64.item()))
    assert abs(P["stats"][0, 1].item() - vf64.item()) < 2e-4 * max(1.0, abs(vf64.item()))
    for k in sorted(model.p):
        g32, g64 = learner.g[k].detach().cpu().double(), p64[k].grad
        scale = g64.abs().max().item() + 1e-12
        assert (g32 - g64).abs().max().item() < 2e-3 * scale, (k, (g32 - g64).abs().max().item(), scale)
        assert ((g32 * g64).sum() / (g32.norm() * g64.norm() + 1e-30)).item() > 0.99999, k


def test_fused_update_with_both_flags_matches_the_torch_learner():
    """A privileged critic (two sources, two row tables), hip_forward and hip_backward, a captured epoch with no library GEMM replayed several
    times, B = 2048, M = 512, against ppo.PPO at test_fused_update_matches_the_torch_learner's tolerances."""
    import torch
    from openroborl_amd import learner_hip, ppo
    from tests.test_gpu_privileged import batch
    dev, B, M, lr_ = torch.device("cuda:0"), 2048, 512, 1e-4
    ref_model, model = ppo.ActorCritic(dev, seed=2, priv_dim=48), ppo.ActorCritic(dev, seed=2, priv_dim=48)
    obs, priv, act, old, adv, ret = batch(dev, B, 1, ref_model)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    ref = ppo.PPO(ref_model, lr=lr_, minibatch=M)
    fused = learner_hip.FusedPPO(model, lr=lr_, minibatch=M, use_graph=True, hip_forward=True, hip_backward=True)
    for it in range(2):
        g1, g2 = torch.Generator(device=dev), torch.Generator(device=dev)
        g1.manual_seed(10 + it); g2.manual_seed(10 + it)
        s_ref = ref.update(obs, act, adv, ret, old_logp=old, epochs=2, generator=g1, priv=priv)
        s_fused = fused.update(obs, act, adv, ret, old_logp=old, epochs=2, generator=g2, priv=priv)
        np.testing.assert_allclose(s_fused, s_ref, rtol=2e-4, atol=2e-5)
    assert fused.steps_taken() == 2 * 2 * (B // M)
    _same_parameters(ref_model, model, before, 2 * 2 * (B // M), lr_)


def test_fused_distill_history_with_hip_forward_matches_the_torch_learner():
    """The encoder chain (the gather of hist, 512 -> 256 -> 48): test_fused_distill_history_matches_the_torch_learner at B = 512, M = 256 and
    its tolerances, hip_forward=True, a captured epoch."""
    import torch
    from openroborl_amd import learner_hip, ppo
    from tests.test_gpu_history import regress_data, student_model
    dev, B, M, lr_ = torch.device("cuda:0"), 512, 256, 1e-4
    hist, target = regress_data(dev, B)
    ref_model, model = student_model(dev, 2), student_model(dev, 2)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    ref, fused = ppo.DistillHistory(ref_model, lr=lr_, minibatch=M), learner_hip.FusedDistillHistory(model, lr=lr_, minibatch=M, hip_forward=True)
    for it in range(2):
        g1, g2 = torch.Generator(device=dev), torch.Generator(device=dev)
        g1.manual_seed(10 + it); g2.manual_seed(10 + it)
        np.testing.assert_allclose(fused.update(hist, target, epochs=2, generator=g2), ref.update(hist, target, epochs=2, generator=g1), rtol=2e-4, atol=2e-5)
    _same_parameters(ref_model, model, before, 2 * 2 * (B // M), lr_, prefix="model/enc_")
