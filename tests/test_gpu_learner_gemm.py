"""The backward GEMMs of the fused learners on the matrix cores (csrc/orr_learner_gemm.hip: orr_wgrad, orr_dgrad_relu) against float64
numpy on the float32 inputs, and through the learners (hip_backward=True).  The bounds are learner_refs' "short" rule, U = 2^-24: a sum
of t terms in ANY order passes every term through at most t - 1 additions, + 1 for the rounding of the product or of the stored value."""
import ctypes as C

import numpy as np
import pytest

from tests import learner_refs as lr
from tests.gpu_kit import EPS as U

pytestmark = pytest.mark.gpu
SENT = 12345.0
WGRAD_SHAPES = [(160, 512), (208, 512), (512, 256), (256, 48)]
DGRAD_SHAPES = [(256, 512), (48, 256)]


def _kit():
    import torch
    from openroborl_amd import _abi, _lib
    dev = torch.device("cuda:0")
    return torch, _abi, _lib.load(), dev, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _finish(torch, _abi, L, st, dev, partials, rows, cols):
    """one orr_colsum_finish job over partials [rows][cols] -> float32 numpy [cols]"""
    out = torch.full((cols,), SENT, device=dev)
    job = (_abi.OrrColsumJob * 1)(_abi.OrrColsumJob(partials.data_ptr(), out.data_ptr(), rows, cols))
    assert L.orr_colsum_finish(job, 1, st) == 0, L.orr_last_error()
    return out.cpu().numpy()


@pytest.mark.parametrize("k,n", WGRAD_SHAPES)
@pytest.mark.parametrize("m", [1, 17, 1000, 4112])
def test_wgrad_matches_float64(m, k, n):
    """m: one row; one past a 16-row fragment; no multiple of any chunk; tall with a short last slice (4112 rows make 16 slices of 288 rows
    for every shape here: fourteen full, one of 80, one empty - not an even split)."""
    torch, _abi, L, dev, st = _kit()
    rng = np.random.RandomState(1000 * k + n + m)
    x, g = lr.mixed(rng, m, k), lr.mixed(rng, m, n)
    S = L.orr_wgrad_slices(m, k, n)
    assert 1 <= S == L.orr_wgrad_slices(m, k, n)
    xd, gd = torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev)
    runs = []
    for _ in range(2):
        part = torch.full((S + 1, k, n), SENT, device=dev)              # a sentinel row behind the last slice
        assert L.orr_wgrad(xd.data_ptr(), k, gd.data_ptr(), n, m, part.data_ptr(), st) == 0, L.orr_last_error()
        gw = _finish(torch, _abi, L, st, dev, part, S, k * n).reshape(k, n)
        runs.append((part.cpu().numpy(), gw))
    part, gw = runs[0]
    assert (part[S] == SENT).all() and (part[:S] != SENT).all()         # exactly S slices, all of them written
    assert np.array_equal(lr.bits(part), lr.bits(runs[1][0])) and np.array_equal(lr.bits(gw), lr.bits(runs[1][1]))
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    ratio = lr.ratio_of(gw, x64.T @ g64, (m + 1) * U * (np.abs(x64).T @ np.abs(g64)))
    print("m %d k %d n %d: S %d, error / bound %.3f" % (m, k, n, S, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("n,k", DGRAD_SHAPES)
@pytest.mark.parametrize("m", [1, 17, 1000])
def test_dgrad_relu_matches_float64(m, n, k):
    torch, _abi, L, dev, st = _kit()
    rng = np.random.RandomState(1000 * k + n + m)
    gz, w = lr.mixed(rng, m, n), lr.mixed(rng, k, n)
    h = lr.relu_data(m, k)[1]                                           # about half exact zeros
    h[rng.uniform(size=h.shape) < 0.2] = -1.5                           # and negatives
    keep = h > 0
    rows = L.orr_dgrad_partial_rows(m)
    d = [torch.from_numpy(a).to(dev) for a in (gz, w, h)]
    runs = []
    for _ in range(2):
        gh, ws = torch.full((m + 2, k), SENT, device=dev), torch.full((rows + 1, k), SENT, device=dev)
        assert L.orr_dgrad_relu(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), m, n, k, gh.data_ptr(), ws.data_ptr(), st) == 0, L.orr_last_error()
        gb = _finish(torch, _abi, L, st, dev, ws, rows, k)
        runs.append((gh.cpu().numpy(), ws.cpu().numpy(), gb))
    gh, ws, gb = runs[0]
    assert (gh[m:] == SENT).all() and (ws[rows] == SENT).all()          # rows >= m and the row behind the partials: untouched
    assert all(np.array_equal(lr.bits(a), lr.bits(b)) for a, b in zip(runs[0], runs[1]))
    assert (lr.bits(gh[:m][~keep]) == 0).all()                          # +0.0 where h <= 0
    gz64, w64 = gz.astype(np.float64), w.astype(np.float64)
    ref = np.where(keep, gz64 @ w64.T, 0.0)
    b_gh = np.where(keep, (n + 1) * U * (np.abs(gz64) @ np.abs(w64).T), 0.0)
    r_gh = lr.ratio_of(gh[:m], ref, b_gh)
    r_gb = lr.ratio_of(gb, ref.sum(axis=0), (m + 1) * U * np.abs(ref).sum(axis=0) + b_gh.sum(axis=0))
    print("m %d n %d k %d: gh error / bound %.3f, gb %.3f" % (m, n, k, r_gh, r_gb))
    assert r_gh <= 1.0 and r_gb <= 1.0


@pytest.mark.parametrize("bad", ["k", "n", "m", "align"])
def test_refused_calls_write_nothing(bad):
    torch, _abi, L, dev, st = _kit()
    m, k, n = (0 if bad == "m" else 32), (24 if bad == "k" else 32), (40 if bad == "n" else 32)
    a = torch.zeros(64 * 64 + 4, device=dev)
    out, ws = torch.full((16 * 64 * 64,), SENT, device=dev), torch.full((64 * 64,), SENT, device=dev)
    p = a.data_ptr() + (4 if bad == "align" else 0)
    assert L.orr_wgrad(p, k, a.data_ptr(), n, m, out.data_ptr(), st) < 0 and b"orr_wgrad" in L.orr_last_error()
    assert L.orr_dgrad_relu(p, a.data_ptr(), a.data_ptr(), m, n, k, out.data_ptr(), ws.data_ptr(), st) < 0 and b"orr_dgrad_relu" in L.orr_last_error()
    if bad != "align":
        assert L.orr_wgrad_slices(m, k, n) == -1
    assert L.orr_dgrad_partial_rows(0) == -1
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((ws == SENT).all())


def _same_parameters(ref_model, model, before, steps, lr_, prefix="model/"):
    """the tolerances of test_fused_update_matches_the_torch_learner / test_fused_distill_history_matches_the_torch_learner"""
    for key in sorted(k for k in before if k.startswith(prefix)):
        a, b = ref_model.p[key].detach(), model.p[key].detach()
        assert (a - b).abs().max().item() < 0.02 * steps * lr_, (key, (a - b).abs().max().item())
        assert (a - b).abs().mean().item() < 2e-3 * steps * lr_, (key, (a - b).abs().mean().item())
        assert (b - before[key]).abs().max().item() > 0.0, key


def test_fused_gradient_with_hip_backward_matches_float64_cpu():
    """test_fused_gradient_matches_float64_cpu's construction and thresholds at B = M = 4112 (a short and an empty slice), hip_backward=True."""
    import torch
    from openroborl_amd import learner_hip, ppo
    from tests.test_gpu_learner import _loss64, _synthetic_batch
    dev, B = torch.device("cuda:0"), 4112
    model = ppo.ActorCritic(dev, seed=4)
    obs, _, act, old, adv, ret = _synthetic_batch(dev, B, seed=0, model=model)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.p.items()}
    loss64, surr64, vf64 = _loss64(p64, obs.cpu().double(), act.cpu().double(), adv.cpu().double(), ret.cpu().double(), old.cpu().double())
    loss64.backward()
    learner = learner_hip.FusedPPO(model, lr=1e-4, minibatch=learner_hip.FusedPPO.fit_minibatch(B, B), hip_backward=True, use_graph=False)
    P = learner._plan(B, B)
    assert P["part0_pi"].shape[0] == learner.L.orr_wgrad_slices(B, 160, 512) and P["n_jobs"] == 10
    with torch.no_grad():
        P["obs"].copy_(obs)
        P["aux"][:, :12], P["aux"][:, 12], P["aux"][:, 13], P["aux"][:, 14] = act, old, adv, ret
        P["perm"].copy_(torch.arange(B, device=dev))
        learner._minibatch(P, 0)
    assert abs(P["stats"][0, 0].item() - surr64.item()) < 2e-4 * max(1.0, abs(surr64.item()))
    assert abs(P["stats"][0, 1].item() - vf64.item()) < 2e-4 * max(1.0, abs(vf64.item()))
    for k in sorted(model.p):
        g32, g64 = learner.g[k].detach().cpu().double(), p64[k].grad
        scale = g64.abs().max().item() + 1e-12
        assert (g32 - g64).abs().max().item() < 2e-3 * scale, (k, (g32 - g64).abs().max().item(), scale)
        assert ((g32 * g64).sum() / (g32.norm() * g64.norm() + 1e-30)).item() > 0.99999, k


def test_fused_update_with_hip_backward_matches_the_torch_learner():
    """(graph=True, B=8192, M=1024) of test_fused_update_matches_the_torch_learner, its tolerances, hip_backward=True: several replays of the
    captured epoch against ppo.PPO."""
    import torch
    from openroborl_amd import learner_hip, ppo
    from tests.test_gpu_learner import _synthetic_batch
    dev, B, M, lr_ = torch.device("cuda:0"), 8192, 1024, 1e-4
    ref_model, model = ppo.ActorCritic(dev, seed=2), ppo.ActorCritic(dev, seed=2)
    obs, _, act, old, adv, ret = _synthetic_batch(dev, B, seed=1, model=ref_model)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    ref, fused = ppo.PPO(ref_model, lr=lr_, minibatch=M), learner_hip.FusedPPO(model, lr=lr_, minibatch=M, use_graph=True, hip_backward=True)
    for it in range(2):
        g1, g2 = torch.Generator(device=dev), torch.Generator(device=dev)
        g1.manual_seed(10 + it); g2.manual_seed(10 + it)
        s_ref = ref.update(obs, act, adv, ret, old_logp=old, epochs=2, generator=g1)
        s_fused = fused.update(obs, act, adv, ret, old_logp=old, epochs=2, generator=g2)
        np.testing.assert_allclose(s_fused, s_ref, rtol=2e-4, atol=2e-5)
    assert fused.steps_taken() == 2 * 2 * (B // M)
    _same_parameters(ref_model, model, before, 32, lr_)


def test_fused_distill_history_with_hip_backward_matches_the_torch_learner():
    """The encoder chain (orr_wgrad at 256 x 48 and 512 x 256, orr_dgrad_relu at n = 48): test_fused_distill_history_matches_the_torch_learner's
    (graph=False, B=512, M=256) case and tolerances, hip_backward=True."""
    import torch
    from openroborl_amd import learner_hip, ppo
    from tests.test_gpu_history import regress_data, student_model
    dev, B, M, lr_ = torch.device("cuda:0"), 512, 256, 1e-4
    hist, target = regress_data(dev, B)
    ref_model, model = student_model(dev, 2), student_model(dev, 2)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    ref, fused = ppo.DistillHistory(ref_model, lr=lr_, minibatch=M), learner_hip.FusedDistillHistory(model, lr=lr_, minibatch=M, use_graph=False, hip_backward=True)
    assert fused._plan(B, M)["n_jobs"] == 3                             # enc_fc0's bias and both weight gradients
    for it in range(2):
        g1, g2 = torch.Generator(device=dev), torch.Generator(device=dev)
        g1.manual_seed(10 + it); g2.manual_seed(10 + it)
        np.testing.assert_allclose(fused.update(hist, target, epochs=2, generator=g2), ref.update(hist, target, epochs=2, generator=g1), rtol=2e-4, atol=2e-5)
    _same_parameters(ref_model, model, before, 2 * 2 * (B // M), lr_, prefix="model/enc_")
