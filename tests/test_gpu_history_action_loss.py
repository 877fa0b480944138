"""The history student's action loss on the device (run with -m gpu on an MI355X):

  a. orr_history_student_head against float64 autograd: the mean, both losses, d loss / d z;
  b. its bitwise properties: the teacher kernel's mean, mean = NULL, two calls, the folded column sums, orr_regress_head, the guard rows;
  c. its refusals;
  d. learner_hip.FusedDistillHistory(action_coef, latent_coef) against ppo.DistillHistory, eager against graph replay, the default coefficients;
  e. that it learns;
  f. train.py --distill --history --distill-action-coef in a child process, and --eval of what it saved.

Tolerances: those of tests/test_gpu_history.py and tests/test_gpu_teacher.py (forward pass: 2e-5 max(1, max|.|); loss head: 2e-5 of the gradient's
scale, x sqrt(m) for a sum over m, and a cosine above 0.99999; losses rtol 2e-4; learners: losses rtol 2e-4 / atol 2e-5, parameters 0.02 steps lr
at most and 2e-3 steps lr on average)."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_history import regress_data, stream, student_model
from tests.test_gpu_teacher import CLIP, SENTINEL, mlp64
from tests.test_history_action_loss_cpu import _data as cpu_data, _student as cpu_student

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 5
SIZES = [1, 15, 16, 17, 33]           # one row; a workgroup's edge on both sides; a third workgroup
COEFS = [(1.0, 0.0), (0.0, 1.0), (0.7, 0.3)]


# ---- the kernel's inputs ----------------------------------------------------------------------------------------------------------------
class Head(object):
    """A history student, its packed actor (policy_hip.FusedActorCritic: what orr_policy_forward_teacher reads) and the three packed transposes"""

    def __init__(self, seed):
        import torch
        from openroborl_amd import policy_hip
        self.dev = torch.device("cuda", 0)
        self.model = student_model(self.dev, seed)
        self.fused = policy_hip.FusedActorCritic(self.model.p, self.dev, std=0.125)
        self.L = L = self.fused.L
        p = {k: v.detach() for k, v in self.model.p.items()}
        w2t = torch.zeros(16, 256, device=self.dev)
        w2t[:12] = p["model/pi/w:0"].t()
        self.t = []
        for w in (w2t, p["model/pi_fc1/w:0"].t().contiguous(), p["model/pi_fc0/w:0"][160:].t().contiguous()):
            out = torch.empty(int(L.orr_policy_packed_size(w.shape[0], w.shape[1])), device=self.dev)
            assert L.orr_policy_pack(w.data_ptr(), w.shape[0], w.shape[1], out.data_ptr(), stream(self.dev)) == 0
            self.t.append(out)
        torch.cuda.synchronize()
        self.p64 = {k: v.cpu().double() for k, v in p.items()}       # the float64 reference lives on the CPU

    def run(self, obs, z, tm, tp, m, a, b, mean=True, net=None):
        """orr_history_student_head on the first m rows with the test's own outputs: GUARD sentinel rows behind each; the partials folded by
        orr_colsum_finish.  -> g_z [m,48], mean [m,12] or None, gb [48], stats [2], partials"""
        import torch
        from openroborl_amd import _abi
        L, dev = self.L, self.dev
        rows = _abi.student_head_rows(m)
        g_z, mu = torch.full((m + GUARD, 48), SENTINEL, device=dev), torch.full((m + GUARD, 12), SENTINEL, device=dev)
        part = torch.full((50 * rows + 50 * GUARD,), SENTINEL, device=dev)
        rc = L.orr_history_student_head(C.byref(self.fused.net) if net is None else net, self.t[0].data_ptr(), self.t[1].data_ptr(), self.t[2].data_ptr(),
                                        obs.data_ptr(), z.data_ptr(), tm.data_ptr(), tp.data_ptr(), m, a, b, g_z.data_ptr(), mu.data_ptr() if mean else None,
                                        part.data_ptr(), stream(dev))
        assert rc == 0, L.orr_last_error()
        gb, stats = torch.full((48 + GUARD,), SENTINEL, device=dev), torch.full((2 + GUARD,), SENTINEL, device=dev)
        jobs = (_abi.OrrColsumJob * 2)(_abi.OrrColsumJob(part.data_ptr(), gb.data_ptr(), rows, 48),
                                       _abi.OrrColsumJob(part.data_ptr() + 4 * 48 * rows, stats.data_ptr(), rows, 2))
        assert L.orr_colsum_finish(jobs, 2, stream(dev)) == 0, L.orr_last_error()
        torch.cuda.synchronize()
        for o, n in ((g_z, m), (part, 50 * rows), (gb, 48), (stats, 2)) + (((mu, m),) if mean else ()):
            assert bool((o[n:] == SENTINEL).all())                   # nothing behind the outputs is written
            assert bool(torch.isfinite(o[:n]).all()) and bool((o[:n] != SENTINEL).all())
        if not mean:
            assert bool((mu == SENTINEL).all())
        return g_z[:m].clone(), mu[:m].clone() if mean else None, gb[:48].clone(), stats[:2].clone(), part[:50 * rows].clone()


@pytest.fixture(scope="module")
def head():
    return Head(3)


def ref64(p, obs, z, tm, tp, a, b):
    """float64 on the CPU: mean, both losses, d (a L_act + b L_lat) / d z by autograd, and the 768 hidden pre-activations of every sample"""
    import torch
    z64 = z.double().requires_grad_(True)
    pre0 = torch.cat((obs.double(), z64), dim=1) @ p["model/pi_fc0/w:0"] + p["model/pi_fc0/b:0"]
    pre1 = torch.relu(pre0) @ p["model/pi_fc1/w:0"] + p["model/pi_fc1/b:0"]
    mu = torch.relu(pre1) @ p["model/pi/w:0"] + p["model/pi/b:0"]
    l_act, l_lat = ((mu - tm.double()) ** 2).sum(dim=1).mean(), ((z64 - tp.double()) ** 2).sum(dim=1).mean()
    g, = torch.autograd.grad(a * l_act + b * l_lat, z64)
    return mu.detach(), l_act.item(), l_lat.item(), g, torch.cat((pre0, pre1), dim=1).detach()


_CASES = {}


def case(head, m):
    """Inputs of m samples + GUARD rows, on the CPU, and which samples stay in the g_z comparison: those none of whose 768 float64 hidden
    pre-activations is smaller in magnitude than 1e-4 max(1, max |pre|) (a float32 pre-activation within rounding of zero can take the other
    side of the ReLU and move the gradient by a whole term).  The seed is the first, counted from 100 m, at which at most a quarter of the
    samples is left out and one remains - decided here, from the float64 reference alone."""
    import torch
    if m not in _CASES:
        for seed in range(100 * m, 100 * m + 50):
            g = torch.Generator().manual_seed(seed)
            obs, z = torch.randn(m + GUARD, 160, generator=g) * 2.0, torch.randn(m + GUARD, 48, generator=g) * 2.0
            tm, tp = torch.randn(m + GUARD, 12, generator=g), torch.randn(m + GUARD, 48, generator=g) * 2.0
            pre = ref64(head.p64, obs[:m], z[:m], tm[:m], tp[:m], 1.0, 1.0)[4]
            keep = pre.abs().min(dim=1).values >= 1e-4 * max(1.0, float(pre.abs().max()))
            if int((~keep).sum()) <= m // 4 and int(keep.sum()) >= 1:
                break
        else:
            raise AssertionError("no seed for m = %d" % m)
        _CASES[m] = (seed, obs, z, tm, tp, keep)
    return _CASES[m]


# ---- a. against float64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", SIZES)
def test_student_head_matches_float64_autograd(head, m):
    """Measured on an MI355X over the five sizes and the three coefficient pairs: g_z off by at most 5.9e-7 of its scale on the retained
    samples (the bound: 2e-5; torch float32 on the CPU against the same float64: at most 5.8e-7), 1 - cosine at most 1.1e-13, the mean off by
    at most 1.1e-6; 0 to 3 samples left out per case."""
    import torch
    seed, obs, z, tm, tp, keep = case(head, m)
    left_out = int((~keep).sum())
    print("m = %d: seed %d, %d of %d samples left out of the g_z comparison" % (m, seed, left_out, m))
    assert left_out <= m // 4 and int(keep.sum()) >= 1
    dev = head.dev
    d = [x.to(dev) for x in (obs, z, tm, tp)]
    for a, b in COEFS:
        g_z, mu, gb, stats, _ = head.run(d[0], d[1], d[2], d[3], m, a, b)
        mu64, act64, lat64, g64, _ = ref64(head.p64, obs[:m], z[:m], tm[:m], tp[:m], a, b)
        assert float((mu64 - mlp64(head.p64, "pi", torch.cat((obs[:m], z[:m]), dim=1))).abs().max()) < 1e-12      # the project's float64 actor
        g32 = g_z.cpu().double()
        scale = float(g64.abs().max())
        err = float((g32 - g64)[keep].abs().max())
        cs = float((g32[keep] * g64[keep]).sum() / (g32[keep].norm() * g64[keep].norm() + 1e-300))
        err_m = float((mu.cpu().double() - mu64).abs().max())
        print("m = %d, coefficients (%g, %g): g_z error %.2e of its scale (bound 2e-5), 1 - cosine %.2e, mean error %.2e of the bound %.2e, "
              "losses %.6f / %.6f against %.6f / %.6f" % (m, a, b, err / scale, 1.0 - cs, err_m, 2e-5 * max(1.0, float(mu64.abs().max())),
                                                          stats[0].item(), stats[1].item(), act64, lat64))
        assert torch.isfinite(g_z).all()
        assert err_m < 2e-5 * max(1.0, float(mu64.abs().max()))
        assert err < 2e-5 * scale
        assert cs > 0.99999
        np.testing.assert_allclose([stats[0].item(), stats[1].item()], [act64, lat64], rtol=2e-4)
        assert scale > 1e-3 / m and float(mu64.abs().max()) > 0.1
    # the action loss's own gradient is there to be got wrong: per sample it is O(0.1)
    assert float(ref64(head.p64, obs[:m], z[:m], tm[:m], tp[:m], 1.0, 0.0)[3].abs().max()) * m > 0.1


# ---- b. bitwise properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", SIZES)
def test_student_head_bitwise_properties(head, m):
    import torch
    from openroborl_amd import _lib
    dev, L = head.dev, head.L
    _, obs, z, tm, tp, _ = case(head, m)
    obs, z, tm, tp = (x.to(dev) for x in (obs, z, tm, tp))
    a, b = 0.7, 0.3
    g_z, mu, gb, stats, part = head.run(obs, z, tm, tp, m, a, b)
    # the mean is the teacher kernel's on priv = z (noise = NULL, value = NULL)
    outs = [torch.full((m + GUARD, c), SENTINEL, device=dev) for c in (12, 12, 12)]
    rc = L.orr_policy_forward_teacher(C.byref(head.fused.net), obs.data_ptr(), z.data_ptr(), m, None, 0.125, CLIP, outs[0].data_ptr(), outs[1].data_ptr(), None,
                                      outs[2].data_ptr(), stream(dev))
    assert rc == 0, L.orr_last_error()
    torch.cuda.synchronize()
    assert torch.equal(mu, outs[2][:m])
    # mean = NULL: no other output bit changes; a second call: the same bits everywhere
    g1, _, gb1, st1, part1 = head.run(obs, z, tm, tp, m, a, b, mean=False)
    assert torch.equal(g1, g_z) and torch.equal(gb1, gb) and torch.equal(st1, stats) and torch.equal(part1, part)
    g2, mu2, gb2, st2, part2 = head.run(obs, z, tm, tp, m, a, b)
    assert torch.equal(g2, g_z) and torch.equal(mu2, mu) and torch.equal(gb2, gb) and torch.equal(st2, stats) and torch.equal(part2, part)
    # the critic's members are not read
    from openroborl_amd import _abi
    actor_only = _abi.OrrPolicyNet()
    for f in ("w0_pi", "b0_pi", "w1_pi", "b1_pi", "w2_pi", "b2_pi"):
        setattr(actor_only, f, getattr(head.fused.net, f))
    g3, mu3, _, _, _ = head.run(obs, z, tm, tp, m, a, b, net=C.byref(actor_only))
    assert torch.equal(g3, g_z) and torch.equal(mu3, mu)
    # the folded column sums
    scale = float(g_z.abs().max())
    err = float((gb.double() - g_z.double().sum(dim=0)).abs().max())
    print("m = %d: folded column sums off by %.2e of the gradient's scale x sqrt(m) (bound 2e-5)" % (m, err / (scale * math.sqrt(m))))
    assert err < 2e-5 * scale * math.sqrt(m)
    # action_coef = 0: orr_regress_head's numbers
    g0, _, gb0, st0, _ = head.run(obs, z, tm, tp, m, 0.0, 1.0)
    zc, tc = z[:m].contiguous(), tp[:m].contiguous()
    gr, gbr, sr = torch.empty(m, 48, device=dev), torch.empty(48, device=dev), torch.empty(1, device=dev)
    ws = torch.empty(int(L.orr_learner_workspace_floats(m, 64)), device=dev)
    _lib.check(L.orr_regress_head(zc.data_ptr(), tc.data_ptr(), m, 48, gr.data_ptr(), gbr.data_ptr(), sr.data_ptr(), ws.data_ptr(), stream(dev)), L)
    torch.cuda.synchronize()
    scale = float(gr.abs().max())
    assert float((g0 - gr).abs().max()) < 2e-5 * scale
    assert float((gb0 - gbr).abs().max()) < 2e-5 * scale * math.sqrt(m)
    assert abs(st0[1].item() - sr[0].item()) < 2e-5 * max(1.0, abs(sr[0].item()))


# ---- c. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_student_head_refusals_write_nothing(head):
    import torch
    from openroborl_amd import _abi
    dev, L, m = head.dev, head.L, 5
    _, obs, z, tm, tp, _ = case(head, 17)
    obs, z, tm, tp = (x.to(dev) for x in (obs, z, tm, tp))
    outs = [torch.full((m + 1, c), SENTINEL, device=dev) for c in (48, 12, 50)]      # g_z, mean, partials

    def call(net=None, w2t=head.t[0].data_ptr(), w1t=head.t[1].data_ptr(), w0zt=head.t[2].data_ptr(), obs_p=obs.data_ptr(), z_p=z.data_ptr(),
             tm_p=tm.data_ptr(), tp_p=tp.data_ptr(), count=m, g_p=outs[0].data_ptr(), mean_p=outs[1].data_ptr(), part_p=outs[2].data_ptr()):
        return L.orr_history_student_head(C.byref(head.fused.net) if net is None else net, w2t, w1t, w0zt, obs_p, z_p, tm_p, tp_p, count, 1.0, 0.5, g_p,
                                          mean_p, part_p, stream(dev))
    no_member, odd, odd_bias = _abi.OrrPolicyNet(), _abi.OrrPolicyNet(), _abi.OrrPolicyNet()
    for dst in (no_member, odd, odd_bias):
        C.memmove(C.byref(dst), C.byref(head.fused.net), C.sizeof(dst))
    no_member.b1_pi = None
    odd.w1_pi = head.fused.net.w1_pi + 4
    odd_bias.b2_pi = head.fused.net.b2_pi + 2
    for kw, text in ((dict(net=C.POINTER(_abi.OrrPolicyNet)()), b"bad argument"), (dict(w2t=None), b"bad argument"), (dict(w1t=None), b"bad argument"),
                     (dict(w0zt=None), b"bad argument"), (dict(obs_p=None), b"bad argument"), (dict(z_p=None), b"bad argument"),
                     (dict(tm_p=None), b"bad argument"), (dict(tp_p=None), b"bad argument"), (dict(g_p=None), b"bad argument"),
                     (dict(part_p=None), b"bad argument"), (dict(count=0), b"bad argument"), (dict(count=-3), b"bad argument"),
                     (dict(net=C.byref(no_member)), b"null pointer"), (dict(net=C.byref(odd)), b"16-byte aligned"),
                     (dict(net=C.byref(odd_bias)), b"4-byte aligned"), (dict(w2t=head.t[0].data_ptr() + 4), b"16-byte aligned"),
                     (dict(w1t=head.t[1].data_ptr() + 8), b"16-byte aligned"), (dict(w0zt=head.t[2].data_ptr() + 12), b"16-byte aligned"),
                     (dict(obs_p=obs.data_ptr() + 2), b"4-byte aligned"), (dict(z_p=z.data_ptr() + 1), b"4-byte aligned"),
                     (dict(tm_p=tm.data_ptr() + 2), b"4-byte aligned"), (dict(tp_p=tp.data_ptr() + 3), b"4-byte aligned"),
                     (dict(g_p=outs[0].data_ptr() + 2), b"4-byte aligned"), (dict(mean_p=outs[1].data_ptr() + 1), b"4-byte aligned"),
                     (dict(part_p=outs[2].data_ptr() + 2), b"4-byte aligned")):
        rc = call(**kw)
        assert rc < 0 and text in L.orr_last_error() and b"orr_history_student_head" in L.orr_last_error(), (kw, rc, L.orr_last_error())
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == SENTINEL).all())
    assert call() == 0                                               # and the same call with everything in place
    torch.cuda.synchronize()
    assert bool((outs[0][:m] != SENTINEL).all()) and bool((outs[1][:m] != SENTINEL).all()) and bool((outs[2].view(-1)[:50] != SENTINEL).all())
    assert bool((outs[0][m:] == SENTINEL).all()) and bool((outs[1][m:] == SENTINEL).all()) and bool((outs[2].view(-1)[50:] == SENTINEL).all())


# ---- d. the learner ---------------------------------------------------------------------------------------------------------------------------
_ACT = {}


def action_data(dev, B):
    """regress_data's hist and latent targets + observations and teacher means of O(1); computed once per B"""
    import torch
    if B not in _ACT:
        g = torch.Generator().manual_seed(B + 1)
        _ACT[B] = regress_data(dev, B) + (torch.randn(B, 160, generator=g).to(dev), torch.randn(B, 12, generator=g).to(dev))
    return _ACT[B]


_FINALS = {}


@pytest.mark.parametrize("graph,B,M", [(True, 512, 256), (False, 512, 256), (True, 8192, 4096)])
def test_fused_learner_with_an_action_loss_matches_the_torch_learner(graph, B, M):
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    lr, a, b = 1e-4, 1.0, 0.5
    hist, target, obs, tmean = action_data(dev, B)
    ref_model, model = student_model(dev, 2), student_model(dev, 2)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    ref = ppo.DistillHistory(ref_model, lr=lr, minibatch=M, action_coef=a, latent_coef=b)
    fused = learner_hip.FusedDistillHistory(model, lr=lr, minibatch=M, use_graph=graph, action_coef=a, latent_coef=b)
    P = fused._plan(B, M)
    assert P["n_jobs"] + 2 <= 12 and len(P["jobs_s"]) == B // M       # within ORR_COLSUM_MAX_JOBS
    steps = 2 * 2 * (B // M)
    for it in range(2):
        g1, g2 = torch.Generator(device=dev), torch.Generator(device=dev)
        g1.manual_seed(10 + it); g2.manual_seed(10 + it)
        s_ref = ref.update(hist, target, 2, g1, obs=obs, target_mean=tmean)
        s_fused = fused.update(hist, target, 2, g2, obs=obs, target_mean=tmean)
        print("losses: fused %.7f (action %.7f, latent %.7f) torch %.7f (%.7f, %.7f)"
              % (s_fused, fused.last_action_loss, fused.last_latent_loss, s_ref, ref.last_action_loss, ref.last_latent_loss))
        np.testing.assert_allclose([s_fused, fused.last_action_loss, fused.last_latent_loss], [s_ref, ref.last_action_loss, ref.last_latent_loss],
                                   rtol=2e-4, atol=2e-5)
    assert fused.steps_taken() == steps                              # the capture's warm-up steps were undone
    moved = 0.0
    for k in sorted(before):
        x, y = ref_model.p[k].detach(), model.p[k].detach()
        if not k.startswith("model/enc_"):                           # the actor and the critic: untouched by both, bit for bit
            assert torch.equal(y, before[k]) and torch.equal(x, before[k]), k
            continue
        moved = max(moved, (y - before[k]).abs().max().item())
        print("%s: largest difference %.3f steps of lr, mean %.5f" % (k, (x - y).abs().max().item() / (steps * lr), (x - y).abs().mean().item() / (steps * lr)))
        assert (x - y).abs().max().item() < 0.02 * steps * lr, (k, (x - y).abs().max().item())
        assert (x - y).abs().mean().item() < 2e-3 * steps * lr, (k, (x - y).abs().mean().item())
    assert moved > 2 * lr
    with pytest.raises(ValueError):
        fused.update(hist, target, 1, None)                          # action_coef > 0 without obs / target_mean
    with pytest.raises(ValueError):
        fused.update(hist, target, 1, None, obs=obs[:, :100], target_mean=tmean)
    # eager and graph replay: the same bits
    _FINALS[(graph, B, M)] = fused.flat_p.clone()
    if (True, B, M) in _FINALS and (False, B, M) in _FINALS:
        assert torch.equal(_FINALS[(True, B, M)], _FINALS[(False, B, M)])


def test_eager_and_graph_replay_give_the_same_bits_and_a_changed_actor_is_packed_again():
    import torch
    from openroborl_amd import learner_hip
    dev = torch.device("cuda:0")
    B, M = 512, 256
    hist, target, obs, tmean = action_data(dev, B)
    finals = []
    for graph in (True, False):
        model = student_model(dev, 2)
        fused = learner_hip.FusedDistillHistory(model, lr=1e-4, minibatch=M, use_graph=graph, action_coef=1.0, latent_coef=0.5)
        g = torch.Generator(device=dev).manual_seed(3)
        fused.update(hist, target, 2, g, obs=obs, target_mean=tmean)
        with torch.no_grad():                                        # somebody loads another actor: the next update sees it
            model.p["model/pi_fc1/w:0"].mul_(1.05)
            model.mark_updated()
        fused.update(hist, target, 1, g, obs=obs, target_mean=tmean)
        finals.append((fused.flat_p.clone(), fused.last_action_loss))
        if graph:
            stale = student_model(dev, 2)                            # the same two updates WITHOUT the change: another action loss
            f2 = learner_hip.FusedDistillHistory(stale, lr=1e-4, minibatch=M, use_graph=True, action_coef=1.0, latent_coef=0.5)
            g = torch.Generator(device=dev).manual_seed(3)
            f2.update(hist, target, 2, g, obs=obs, target_mean=tmean)
            f2.update(hist, target, 1, g, obs=obs, target_mean=tmean)
            assert abs(f2.last_action_loss - fused.last_action_loss) > 1e-3 * fused.last_action_loss
    assert torch.equal(finals[0][0], finals[1][0]) and finals[0][1] == finals[1][1]


def test_default_coefficients_take_the_path_without_them_bit_for_bit():
    import torch
    from openroborl_amd import learner_hip
    dev = torch.device("cuda:0")
    B, M = 512, 256
    hist, target, obs, tmean = action_data(dev, B)
    finals = []
    for kw in (dict(), dict(action_coef=0.0, latent_coef=1.0)):
        fused = learner_hip.FusedDistillHistory(student_model(dev, 2), lr=1e-4, minibatch=M, **kw)
        assert not fused.head
        losses = [fused.update(hist, target, 1, torch.Generator(device=dev).manual_seed(i)) for i in range(2)]
        assert "jobs_s" not in fused._plan(B, M) and fused._actor is None       # orr_regress_head: no head buffers, no packed actor
        finals.append((fused.flat_p.clone(), losses))
    assert torch.equal(finals[0][0], finals[1][0]) and finals[0][1] == finals[1][1]


# ---- e. it learns -----------------------------------------------------------------------------------------------------------------------------
def test_the_action_loss_falls_on_a_fixed_batch():
    """tests/test_history_action_loss_cpu.py's student and batch (there ppo.DistillHistory alone is shown to bring the loss down), here on the device"""
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = torch.device("cuda:0")
    hist, priv, obs, mean = (x.to(dev) for x in cpu_data(7))
    model = ppo.ActorCritic(dev, params=cpu_student(5).state_dict())
    assert model.history == 16
    fused = learner_hip.FusedDistillHistory(model, lr=1e-3, minibatch=16, action_coef=1.0, latent_coef=0.0)
    losses = [fused.update(hist, priv, 1, torch.Generator(device=dev).manual_seed(i), obs=obs, target_mean=mean) for i in range(20)]
    print("action loss: %.5f -> %.5f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
    assert fused.last_action_loss == pytest.approx(losses[-1]) and fused.last_latent_loss > 0.0


# ---- f. train.py ------------------------------------------------------------------------------------------------------------------------------
def test_train_a_history_student_with_the_action_loss_and_evaluate_it(tmp_path):
    teacher_zip, student_zip, log_path = str(tmp_path / "T.zip"), str(tmp_path / "s.zip"), str(tmp_path / "log.json")
    common = ["--num-robot", "64", "--horizon", "8", "--iters", "2", "--push", "0.05,0.2,0.5"]

    def run(*argv):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + list(argv), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        return r.stdout.decode()
    run("--privileged-actor", "--save", teacher_zip, *common)
    run("--distill", teacher_zip, "--history", "--distill-action-coef", "1", "--save", student_zip, "--log", log_path, *common)
    log = json.load(open(log_path))
    assert log and log[-1]["iter"] == 1
    for rec in log:
        assert math.isfinite(rec["action_loss"]) and rec["action_loss"] > 0.0 and math.isfinite(rec["latent_loss"]) and rec["latent_loss"] > 0.0
        assert rec["total_loss"] == pytest.approx(rec["action_loss"] + rec["latent_loss"], rel=1e-4, abs=1e-5)
    rec = json.loads(run("--eval", student_zip, "--num-robot", "16").strip().splitlines()[-1])
    assert rec["robots"] == 16 and math.isfinite(rec["return_mean"])
