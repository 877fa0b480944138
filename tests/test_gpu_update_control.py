"""The update controls on the device (include/openroborl_learner.h: orr_update_control, orr_adam_step_ctl; learner_hip's control path):
a. the two entry points alone, against float64 and a host restatement of the rules;
b. the fused learners under them against the torch yardsticks (ppo._UpdateControl) from the same parameters, data and permutations."""
import ctypes as C
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests.gpu_kit import EPS
from tests.test_gpu_learner import _ptr, _stream, _synthetic_batch
from tests.test_update_control_cpu import kl_rule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
WORDS = None      # _abi.UPDATE_CTL_WORDS, set by lib()


def lib():
    global WORDS
    import torch
    from openroborl_amd import _abi, _lib
    WORDS = _abi.UPDATE_CTL_WORDS
    return _lib, _lib.load(), torch.device("cuda:0")


def new_ctl(dev, **words):
    """An orr_update_ctl on the device as its owner initialises it: the three factors 1, everything else 0; `words` override."""
    import torch
    host = np.zeros(len(WORDS), dtype=np.int32)
    host.view(F32)[:3] = 1.0
    for k, v in words.items():
        i = WORDS.index(k)
        if isinstance(v, float):
            host.view(F32)[i] = v
        else:
            host[i] = v
    return torch.from_numpy(host).to(dev)


def read_ctl(ctl):
    raw = ctl.cpu().numpy()
    return {k: (float(raw.view(F32)[i]) if k in ("lr_mult", "kl_lr_mult", "grad_scale", "grad_norm", "grad_norm_max", "grad_norm_sum") else int(raw[i]))
            for i, k in enumerate(WORDS)}


def control(_lib, L, dev, g, n, partials, ctl, pre_scale=1.0, max_norm=0.0, kl=None, kl_stop=0.0, kl_target=0.0, lo=0.5, hi=2.0):
    _lib.check(L.orr_update_control(_ptr(g), n, pre_scale, max_norm, None if kl is None else _ptr(kl), kl_stop, kl_target, lo, hi, _ptr(partials),
                                    _ptr(ctl), _stream(dev)), L)
    return read_ctl(ctl)


def fold_like_the_kernel(partials):
    """orr_update_control's second launch on the host, in float32: lane l adds partials[l], partials[l + 64], ... one after the other, then
    the wave's shuffle tree (offsets 32 .. 1); lane 0's value."""
    x = np.zeros(64, dtype=F32)
    for b in range(0, len(partials), 64):
        chunk = partials[b:b + 64]
        x[:len(chunk)] = x[:len(chunk)] + chunk
    for o in (32, 16, 8, 4, 2, 1):
        x[:o] = x[:o] + x[o:2 * o]
    return x[0]


# ---- a. the kernels alone -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [434701, 4099, 8, 3])     # the real size; a workgroup's tail; two vectors; fewer floats than one vector
def test_update_control_norm_scale_and_guard(n):
    import torch
    _lib, L, dev = lib()
    gen = torch.Generator(device=dev).manual_seed(n)
    pad = (n + 3) // 4 * 4 + 1024
    g = torch.randn(pad, device=dev, generator=gen) * (10.0 ** -(torch.arange(pad, device=dev) % 4).float())
    g[n:] = 1e30                                           # nothing at or beyond n is read
    P = int(L.orr_update_control_partials(n))
    assert P == (n + 1023) // 1024
    partials, ctl = torch.zeros(P, device=dev), new_ctl(dev)
    c = control(_lib, L, dev, g, n, partials, ctl)
    # the sum of squares against float64 within the kernel's own bound (csrc/orr_learner.hip): (17 + ceil(P / 64)) roundings of 2^-24
    s64 = float((g[:n].double() ** 2).sum())
    bound = (17 + (P + 63) // 64) * EPS
    assert bound <= 1e-5
    s32 = fold_like_the_kernel(partials.cpu().numpy())
    print("n %d: sum of squares rel err %.3g (bound %.3g)" % (n, abs(float(s32) - s64) / s64, bound))
    assert abs(float(s32) - s64) <= bound * s64
    norm = F32(c["grad_norm"])
    assert abs(float(norm) - math.sqrt(float(s32))) <= 2.0 * EPS * float(norm)       # the record's norm is sqrt of that sum
    assert c["grad_scale"] == 1.0 and c["skip"] == 0 and c["n_calls"] == 1 and c["n_clipped"] == 0 and c["grad_norm_max"] == c["grad_norm"]
    first = (partials.clone(), ctl.clone())
    # the same inputs give the same bits; the padding changes nothing
    partials2, ctl2 = torch.zeros(P, device=dev), new_ctl(dev)
    control(_lib, L, dev, g, n, partials2, ctl2)
    assert torch.equal(partials2, first[0]) and torch.equal(ctl2, first[1])
    g0 = g.clone()
    g0[n:] = 0.0
    partials2, ctl2 = torch.zeros(P, device=dev), new_ctl(dev)
    control(_lib, L, dev, g0, n, partials2, ctl2)
    assert torch.equal(partials2, first[0]) and torch.equal(ctl2, first[1])
    # the clip coefficient: max_norm below, at and above the norm, and off
    clipped = 0
    for mn in (0.5 * float(norm), float(norm), 2.0 * float(norm), 0.0, -1.0):
        c = control(_lib, L, dev, g, n, partials, ctl, max_norm=mn)
        want = min(F32(1.0), F32(mn) / (norm + F32(1e-6))) if mn > 0.0 else F32(1.0)
        assert abs(c["grad_scale"] - float(want)) <= EPS * float(want), (mn, c["grad_scale"], want)
        clipped += int(c["grad_scale"] < 1.0)
        assert c["n_clipped"] == clipped and c["grad_norm"] == float(norm)
    assert clipped >= 1 and c["n_calls"] == 6 and abs(c["grad_norm_sum"] - 6.0 * float(norm)) <= 8.0 * EPS * 6.0 * float(norm)
    # pre_scale scales the norm (a power of two: exactly)
    c = control(_lib, L, dev, g, n, partials, ctl, pre_scale=0.25)
    assert c["grad_norm"] == 0.25 * float(norm) and c["grad_norm_max"] == float(norm)
    # the guard: a NaN in the first element, the last, a middle workgroup; an Inf; a square beyond float32
    bad = 0
    for idx, val in ((0, float("nan")), (n - 1, float("nan")), ((P // 2) * 1024 % n, float("nan")), (n // 2, float("inf")), (n // 3, 1e20)):
        gb = g.clone()
        gb[idx] = val
        c = control(_lib, L, dev, gb, n, partials, ctl, max_norm=1.0)
        bad += 1
        assert c["skip"] == 1 and c["grad_scale"] == 0.0 and c["n_nonfinite"] == bad and not math.isfinite(c["grad_norm"]), (idx, val, c)
        assert math.isfinite(c["grad_norm_max"]) and math.isfinite(c["grad_norm_sum"]) and c["n_calls"] == 7
        c = control(_lib, L, dev, g, n, partials, ctl)     # the next clean call clears bit 0
        assert c["skip"] == 0 and c["grad_scale"] == 1.0 and c["n_nonfinite"] == bad and c["grad_norm"] == float(norm)
        ctl[WORDS.index("n_calls")] = 7


def host_control(c, kl, kl_stop, kl_target, lo, hi):
    """The host restatement of orr_update_control's KL rules on a record `c` (a finite gradient, no clip)."""
    c = dict(c)
    bad = not math.isfinite(kl)
    skip = (c["skip"] & 2) | int(bad)
    if not bad and kl_stop > 0.0 and F32(kl) > F32(kl_stop):
        skip |= 2
    if skip == 0 and kl_target > 0.0:
        c["kl_lr_mult"] = kl_rule(c["kl_lr_mult"], kl, kl_target, lo, hi)
    c["grad_scale"] = 0.0 if bad else 1.0
    c["n_nonfinite"] += int(bad)
    c["n_calls"] += int(not bad)
    c["n_kl_skipped"] += int(bool(skip & 2))
    c["skip"] = skip
    return c


def test_update_control_kl_rules_follow_the_host_restatement():
    import torch
    _lib, L, dev = lib()
    n, t, lo, hi = 8, 0.01, 0.4, 2.0
    g = torch.full((n,), 0.5, device=dev)
    partials, ctl, kl = torch.zeros(1, device=dev), new_ctl(dev), torch.zeros(1, device=dev)
    want = read_ctl(ctl)
    nan = float("nan")
    # (kl, kl_stop): the adaptive rule through both clamps and the dead band, a NaN; then the stop: trips, holds through small KLs and a NaN
    seq = [(x * t, 0.0) for x in (0.0, 0.4, 0.4, 0.4, 0.6, 1.9, 2.1, 2.1, 2.1, 2.1, 2.1)] + [(nan, 0.0), (0.4 * t, 0.0)]
    seq += [(1.9 * t, 2.0 * t), (2.1 * t, 2.0 * t), (0.4 * t, 2.0 * t), (nan, 2.0 * t), (0.4 * t, 2.0 * t), (0.4 * t, 0.0)]
    mults, skips = [], []
    for x, stop in seq:
        kl.fill_(x)
        got = control(_lib, L, dev, g, n, partials, ctl, kl=kl, kl_stop=stop, kl_target=t, lo=lo, hi=hi)
        want = host_control(want, float(F32(x)), stop, t, lo, hi)
        for k in ("kl_lr_mult", "skip", "grad_scale", "n_nonfinite", "n_kl_skipped", "n_calls"):
            assert got[k] == want[k], (x, stop, k, got, want)
        mults.append(got["kl_lr_mult"]); skips.append(got["skip"])
    assert max(mults) == hi and min(mults) == float(F32(lo)) and mults[0] == 1.0                 # both clamps were met
    assert skips[-6:] == [0, 2, 2, 3, 2, 2] and got["n_kl_skipped"] == 5 and got["n_nonfinite"] == 2
    before = got["kl_lr_mult"]
    ctl[WORDS.index("skip")] = 0                             # the host clears the gate: the next step is taken and the rule runs again
    got = control(_lib, L, dev, g, n, partials, ctl, kl=kl, kl_stop=2.0 * t, kl_target=t, lo=lo, hi=hi)
    assert got["skip"] == 0 and got["kl_lr_mult"] == kl_rule(before, 0.4 * t, t, lo, hi) != before and got["n_kl_skipped"] == 5
    # kl == NULL with the thresholds off: no rule, no refusal
    got = control(_lib, L, dev, g, n, partials, ctl)
    assert got["skip"] == 0 and abs(got["grad_norm"] - math.sqrt(8 * 0.25)) <= 2.0 * EPS * math.sqrt(2.0)


def adam64(p, m, v, g, t, lr, flags, b1=0.9, b2=0.999, eps=1e-5):
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    if flags:       # ORR_ADAM_MPI_EPSILON
        p = p - lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (v.sqrt() + eps)
    else:
        p = p - lr / (1 - b1 ** t) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    return p, m, v


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("n", [434701, 8, 3])
def test_adam_step_ctl(n, flags):
    import torch
    _lib, L, dev = lib()
    gen = torch.Generator(device=dev).manual_seed(n)
    pad = (n + 3) // 4 * 4
    p0 = torch.randn(pad, device=dev, generator=gen)
    grads = [torch.randn(pad, device=dev, generator=gen) * (10.0 ** -(i % 4)) for i in range(6)]
    z = lambda: torch.zeros(pad, device=dev)                # noqa: E731
    zs = lambda: torch.zeros(2, dtype=torch.int32, device=dev)   # noqa: E731

    def plain(bufs, g):
        _lib.check(L.orr_adam_step(_ptr(bufs[0]), _ptr(g), _ptr(bufs[1]), _ptr(bufs[2]), n, 1e-3, 0.9, 0.999, 1e-5, 0.5, flags, _ptr(bufs[3]),
                                   _stream(dev)), L)

    def under(bufs, g, ctl):
        _lib.check(L.orr_adam_step_ctl(_ptr(bufs[0]), _ptr(g), _ptr(bufs[1]), _ptr(bufs[2]), n, 1e-3, 0.9, 0.999, 1e-5, 0.5, flags, _ptr(bufs[3]),
                                       _ptr(ctl), _stream(dev)), L)

    # the neutral record: orr_adam_step's bits, six steps
    a, b, ctl = [p0.clone(), z(), z(), zs()], [p0.clone(), z(), z(), zs()], new_ctl(dev)
    for g in grads:
        plain(a, g)
        under(b, g, ctl)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert b[3].tolist() == [6, 0]
    if pad > n:                                             # nothing beyond n is touched
        assert torch.equal(b[0][n:], p0[n:]) and bool((b[1][n:] == 0).all()) and bool((b[2][n:] == 0).all())
    # the factors: float64 Adam with lr and gradient scaled accordingly
    ctl = new_ctl(dev, lr_mult=0.5, kl_lr_mult=1.5, grad_scale=0.25)
    b = [p0.clone(), z(), z(), zs()]
    p64, m64, v64 = p0.double(), z().double(), z().double()
    for t, g in enumerate(grads, 1):
        under(b, g, ctl)
        p64, m64, v64 = adam64(p64, m64, v64, g.double() * 0.5 * 0.25, t, 1e-3 * 0.5 * 1.5, flags)
        assert (b[0][:n].double() - p64[:n]).abs().max().item() < 2e-6
    # a set skip word: nothing changes, and the step count does not advance - the next step is the one a run without the skipped call takes
    a, b = [p0.clone(), z(), z(), zs()], [p0.clone(), z(), z(), zs()]
    ctl = new_ctl(dev)
    for i, g in enumerate(grads[:3]):
        plain(a, g)
        under(b, g, ctl)
        held = [x.clone() for x in b]
        ctl[WORDS.index("skip")] = i + 1                    # 1, 2, 3
        under(b, grads[5], ctl)
        assert all(torch.equal(x, y) for x, y in zip(b, held)), i
        ctl[WORDS.index("skip")] = 0
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and b[3].tolist() == [3, 0]


# ---- b. the learners --------------------------------------------------------------------------------------------------------------------

SHAPES = [(8192, 1024), (32768, 4096)]      # both weight-gradient forms (plain GEMMs; the 16-way split over the batch)
LR = 1e-4


def heavy_rows(B):
    """A dozen rows whose advantage and return are far out: the minibatches' gradient norms then differ by how many of them each drew."""
    import torch
    return torch.arange(12) * (B // 12) + 5


def setup(kind, dev, B, seed=2):
    """-> (reference model, fused model, update() arguments, keywords, reference class, fused class, constructor keywords)"""
    import torch
    from openroborl_amd import learner_hip, ppo
    if kind == "history":
        from tests.test_gpu_history_ppo import history_batch, history_policy
        ref_model, model = history_policy(dev, seed), history_policy(dev, seed)
        obs, hist, priv, act, old, adv, ret = history_batch(dev, B, 1, ref_model)
        adv[heavy_rows(B)], ret[heavy_rows(B)] = 60.0, 40.0
        return ref_model, model, (obs, hist, priv, act, adv, ret), {"old_logp": old}, ppo.PPOHistory, learner_hip.FusedPPOHistory, {"latent_coef": 0.5}
    if kind == "distill":
        from tests.test_gpu_teacher import distill_data
        ref_model, model = ppo.ActorCritic(dev, seed=seed), ppo.ActorCritic(dev, seed=seed)
        obs, target = distill_data(dev, B)
        target = target.clone()
        target[heavy_rows(B)] += 30.0
        return ref_model, model, (obs, target), {}, ppo.Distill, learner_hip.FusedDistill, {}
    kw = {"learn_std": True} if kind == "learn_std" else {}
    ref_model, model = ppo.ActorCritic(dev, seed=seed, **kw), ppo.ActorCritic(dev, seed=seed, **kw)
    obs, _, act, old, adv, ret = _synthetic_batch(dev, B, seed=1, model=ref_model)
    adv[heavy_rows(B)], ret[heavy_rows(B)] = 60.0, 40.0
    return ref_model, model, (obs, act, adv, ret), {"old_logp": old}, ppo.PPO, learner_hip.FusedPPO, ({"ent_coef": 0.01} if kw else {})


def gen(dev, seed):
    import torch
    return torch.Generator(device=dev).manual_seed(seed)


def same_parameters(ref_model, model, steps, lr=LR, names=None):
    """test_fused_update_matches_the_torch_learner's bounds: Adam moves a weight by at most lr per step."""
    for k in sorted(names or model.p):
        a, b = ref_model.p[k].detach(), model.p[k].detach()
        assert (a - b).abs().max().item() < 0.02 * steps * lr, (k, (a - b).abs().max().item())
        assert (a - b).abs().mean().item() < 2e-3 * steps * lr, (k, (a - b).abs().mean().item())


@pytest.mark.parametrize("kind,graph,B,M", [("ppo", True, 8192, 1024), ("ppo", False, 8192, 1024), ("ppo", True, 32768, 4096), ("ppo", False, 32768, 4096),
                                            ("learn_std", True, 8192, 1024), ("history", True, 8192, 1024), ("distill", True, 8192, 1024)])
def test_gradient_clip_matches_the_torch_learner(kind, graph, B, M):
    import torch
    _, _, dev = lib()
    # a first look at the reference's norms: the clip goes into their widest gap, so that some minibatches clip and some do not
    probe_model, _, args, kw, ref_cls, _, ckw = setup(kind, dev, B)
    probe = ref_cls(probe_model, lr=LR, minibatch=M, max_grad_norm=1e9, **ckw)
    probe.update(*args, epochs=2, generator=gen(dev, 10), **kw)
    norms = sorted(probe.grad_norms)
    gap, i = max((norms[j + 1] / norms[j], j) for j in range(len(norms) - 1))
    c = 0.5 * (norms[i] + norms[i + 1])
    ref_model, model, args, kw, ref_cls, fused_cls, ckw = setup(kind, dev, B)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    ref = ref_cls(ref_model, lr=LR, minibatch=M, max_grad_norm=c, **ckw)
    fused = fused_cls(model, lr=LR, minibatch=M, max_grad_norm=c, use_graph=graph, **ckw)
    s_ref = ref.update(*args, epochs=2, generator=gen(dev, 10), **kw)
    s_fused = fused.update(*args, epochs=2, generator=gen(dev, 10), **kw)
    steps = 2 * (B // M)
    print("%s: norms %s, clip at %.4f (gap x%.3f)" % (kind, " ".join("%.3f" % x for x in ref.grad_norms), c, gap))
    assert len(ref.grad_norms) == steps and all(abs(x - c) > 0.02 * c for x in ref.grad_norms)      # no clip decided by rounding
    r, f = ref.control_stats(), fused.control_stats()
    assert 0 < r["clipped"] < steps and r["clipped"] == sum(x > c for x in ref.grad_norms)
    assert f["clipped"] == r["clipped"] and f["calls"] == r["calls"] == steps and f["skipped_nonfinite"] == f["skipped_kl"] == 0
    assert abs(f["grad_norm_max"] - r["grad_norm_max"]) < 1e-3 * r["grad_norm_max"]
    assert abs(f["grad_norm_mean"] - r["grad_norm_mean"]) < 1e-3 * r["grad_norm_mean"]
    np.testing.assert_allclose(s_fused, s_ref, rtol=2e-4, atol=2e-5)
    assert fused.steps_taken() == steps
    same_parameters(ref_model, model, steps, names=fused.slots)
    assert max((model.p[k].detach() - before[k]).abs().max().item() for k in fused.slots) > 2 * LR
    assert fused.control_stats()["calls"] == 0               # reading cleared the counters


@pytest.mark.parametrize("B,M", SHAPES)
def test_a_non_finite_minibatch_is_skipped_on_the_device(B, M):
    import torch
    from openroborl_amd import learner_hip, ppo
    _, _, dev = lib()
    ref_model, model, (obs, act, adv, ret), kw, _, _, _ = setup("ppo", dev, B)
    perm = torch.randperm(B, device=dev, generator=gen(dev, 7))            # the permutation both learners will draw
    adv[perm[3 * M:4 * M]] = float("nan")                                 # the rows of the fourth minibatch
    ref, fused = ppo.PPO(ref_model, lr=LR, minibatch=M, max_grad_norm=1e9), learner_hip.FusedPPO(model, lr=LR, minibatch=M, max_grad_norm=1e9)
    ref.update(obs, act, adv, ret, epochs=1, generator=gen(dev, 7), **kw)
    fused.update(obs, act, adv, ret, epochs=1, generator=gen(dev, 7), **kw)
    nmb = B // M
    assert bool(torch.isfinite(fused.flat_p).all()) and bool(torch.isfinite(fused.m).all()) and bool(torch.isfinite(fused.v).all())
    assert fused.steps_taken() == nmb - 1
    f, r = fused.control_stats(), ref.control_stats()
    assert f["skipped_nonfinite"] == r["skipped_nonfinite"] == 1 and f["calls"] == r["calls"] == nmb - 1
    same_parameters(ref_model, model, nmb - 1)


def test_set_lr_mult_never_captures_again_and_is_not_a_skip():
    import torch
    from openroborl_amd import learner_hip, ppo
    _, _, dev = lib()
    B, M = SHAPES[0]
    ref_model, model, args, kw, _, _, _ = setup("ppo", dev, B)
    ref, fused = ppo.PPO(ref_model, lr=LR, minibatch=M), learner_hip.FusedPPO(model, lr=LR, minibatch=M, device_lr=True)
    key = fused._graph_key()
    graphs = None
    for it, mult in enumerate((1.0, 0.5)):
        ref.set_lr_mult(mult)
        fused.set_lr_mult(mult)
        ref.update(*args, epochs=1, generator=gen(dev, 20 + it), **kw)
        fused.update(*args, epochs=1, generator=gen(dev, 20 + it), **kw)
        P = fused._plan(B, M)
        assert graphs is None or P["graphs"] is graphs       # one capture
        graphs = P["graphs"]
    assert fused._graph_key() == key and ref.opt.param_groups[0]["lr"] == float(F32(LR) * F32(0.5))
    steps = 2 * (B // M)
    same_parameters(ref_model, model, steps)
    # the second update moved by half a learning rate per step: a run that ignored the multiplier is outside the bounds of one that did not
    # multiplier 0: the parameters stand, the moments move and the step counts - a skip would leave all three
    p, m, v = fused.flat_p.clone(), fused.m.clone(), fused.v.clone()
    fused.set_lr_mult(0.0)
    fused.update(*args, epochs=1, generator=gen(dev, 22), **kw)
    assert P["graphs"] is graphs and torch.equal(fused.flat_p, p) and not torch.equal(fused.m, m) and not torch.equal(fused.v, v)
    assert fused.steps_taken() == steps + B // M and fused.control_stats()["lr_mult"] == 0.0
    with pytest.raises(RuntimeError):
        learner_hip.FusedPPO(ppo.ActorCritic(dev, seed=1), lr=LR, minibatch=M).set_lr_mult(0.5)


# the KL gate: minibatch s of the first permutation has its old log-probabilities raised by KL_SHIFT[s], so its approx_kl is
# exp(-d) - 1 + d at the start and the minibatches' KLs grow over the update: 0.0012 0.015 0.043 0.084 0.136 0.197 0.266 0.343
KL_SHIFT = [0.05 + 0.13 * s for s in range(8)]
KL_TARGET, KL_STOP, KL_BOUNDS = 0.06, 0.23, (0.5, 2.0)      # target / 2 = 0.03, 2 target = 0.12 and the stop: each in a gap of that sequence


def kl_data(kind, dev, B, M, seed):
    import torch
    ref_model, model, (obs, act, adv, ret), _, ref_cls, fused_cls, ckw = setup(kind, dev, B)
    assert B // M == len(KL_SHIFT)
    with torch.no_grad():
        old = ref_model.log_prob(obs, act).clone()
    perm = torch.randperm(B, device=dev, generator=gen(dev, seed))
    for s, d in enumerate(KL_SHIFT):
        old[perm[s * M:(s + 1) * M]] += d
    return ref_model, model, (obs, act, adv, ret), {"old_logp": old}, ref_cls, fused_cls, ckw


KL_ON = dict(kl_stop=KL_STOP, kl_target=KL_TARGET, kl_lr_bounds=KL_BOUNDS)


@pytest.mark.parametrize("kind,B,M", [("ppo", 8192, 1024), ("ppo", 32768, 4096), ("learn_std", 8192, 1024)])
def test_kl_stop_and_kl_target_match_the_torch_learner(kind, B, M):
    import torch
    _, _, dev = lib()
    lr = 1e-5
    ref_model, model, args, kw, ref_cls, fused_cls, ckw = kl_data(kind, dev, B, M, 30)
    ref, fused = ref_cls(ref_model, lr=lr, minibatch=M, **KL_ON, **ckw), fused_cls(model, lr=lr, minibatch=M, **KL_ON, **ckw)
    s_ref = ref.update(*args, epochs=1, generator=gen(dev, 30), **kw)
    s_fused = fused.update(*args, epochs=1, generator=gen(dev, 30), **kw)
    print("%s: reference KLs %s" % (kind, " ".join("%.5f" % x for x in ref.kls)))
    # the condition under which the two learners must agree step for step: every reference KL at least 5 % away from every threshold
    for x in ref.kls:
        for thr in (KL_STOP, 2.0 * KL_TARGET, 0.5 * KL_TARGET):
            assert abs(x - thr) > 0.05 * thr, (x, thr)
    assert all(x > 0.0 for x in ref.kls) and ref.kls == sorted(ref.kls)
    taken = {int(s["step"]) for s in ref.opt.state.values()}
    assert taken == {6} and fused.steps_taken() == 6
    r, f = ref.control_stats(), fused.control_stats()
    assert f["skipped_kl"] == r["skipped_kl"] == 2 and f["skipped_nonfinite"] == 0
    assert f["kl_lr_mult"] == r["kl_lr_mult"] == float(F32(2.0) / F32(1.5) / F32(1.5))
    assert len(s_fused) == len(s_ref) == (5 if kind == "learn_std" else 2)      # a fixed-std model still returns its two stats
    np.testing.assert_allclose(s_fused, s_ref, rtol=2e-4, atol=2e-5)
    same_parameters(ref_model, model, 6, lr=2.0 * lr)      # six steps of at most lr x the multiplier's upper bound
    # the stop held for that update() only
    fused.update(*args, epochs=1, generator=gen(dev, 31), **kw)
    assert fused.steps_taken() > 6


def all_controls_run(dev, graph, seed=40, several=False):
    B, M = SHAPES[0]
    _, model, args, kw, _, fused_cls, _ = kl_data("ppo", dev, B, M, seed)
    fused = fused_cls(model, lr=LR, minibatch=M, use_graph=graph, max_grad_norm=15.0, device_lr=True, **KL_ON)
    fused.set_lr_mult(0.7)
    fused.update(*args, epochs=1, generator=gen(dev, seed), **kw)
    fused.update(*args, epochs=2, generator=gen(dev, seed + 1), **kw)
    assert fused._several() == several and len(fused._plan(B, M)["graphs"] or [None]) == (B // M if several and graph else 1)
    return fused.flat_p.clone(), fused.control_stats()


def test_all_controls_on_are_reproducible_bit_for_bit_graph_and_eager():
    import torch
    _, _, dev = lib()
    runs = [all_controls_run(dev, graph) for graph in (True, True, False)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][0], runs[2][0])
    assert runs[0][1] == runs[1][1] == runs[2][1] and runs[0][1]["calls"] == 24 and runs[0][1]["clipped"] > 0 and runs[0][1]["skipped_kl"] > 0


SEVERAL_RANKS_WORKER = r"""
import os, sys, torch
sys.path.insert(0, %r)
import torch.distributed as dist
from openroborl_amd import dist as odist
from tests.test_gpu_update_control import all_controls_run
dev = torch.device("cuda:0")
rank, world, local = odist.init_from_env()
assert dist.is_initialized() and dist.get_backend() == "nccl" and world == 1
p, stats = all_controls_run(dev, True, several=True)
dist.barrier(); dist.destroy_process_group()
torch.save((p.cpu(), stats), sys.argv[1])
print("learner ok")
"""


def test_the_several_ranks_path_gives_the_one_graph_paths_bits(tmp_path):
    """Per-minibatch graphs with the gradient's and the KL's all-reduce, orr_update_control and the step between replays, on RCCL with a
    one-rank group (ORR_FORCE_DIST=1, a fresh child process as in tests/test_gpu_dist.py): clip, schedule and KL gate give the bits of the
    path that captures them inside one graph, which runs here."""
    import torch
    _, _, dev = lib()
    script = tmp_path / "worker.py"
    script.write_text(SEVERAL_RANKS_WORKER % (ROOT,))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               ORR_FORCE_DIST="1")
    rccl = subprocess.run([sys.executable, str(script), str(tmp_path / "rccl.pt")], env=env, capture_output=True, text=True, timeout=300)
    assert rccl.returncode == 0 and "learner ok" in rccl.stdout, rccl.stdout[-2000:] + rccl.stderr[-3000:]
    p0, s0 = all_controls_run(dev, True)
    p1, s1 = torch.load(tmp_path / "rccl.pt")
    assert torch.equal(p0.cpu(), p1) and s0 == s1 and s0["skipped_kl"] > 0 and s0["clipped"] > 0


class Spy(object):
    """The library with a record of the entry points called through it."""

    def __init__(self, L):
        self._L, self.called = L, set()

    def __getattr__(self, name):
        self.called.add(name)
        return getattr(self._L, name)


def test_defaults_launch_what_they_always_did():
    from openroborl_amd import learner_hip, ppo
    _, _, dev = lib()
    B, M = 2048, 1024
    _, model, args, kw, _, _, _ = setup("ppo", dev, B)
    fused = learner_hip.FusedPPO(model, lr=LR, minibatch=M, use_graph=False)
    assert fused.ctl is None
    assert fused._graph_key() == (LR, 0.9, 0.999, 1e-5, 0, 0.2, 1.0, 0.125)      # the parent commit's key
    fused.L = Spy(fused.L)
    fused.update(*args, **kw)
    assert "orr_adam_step" in fused.L.called and "orr_ppo_head" in fused.L.called
    assert not fused.L.called & {"orr_update_control", "orr_adam_step_ctl", "orr_ppo_head_logstd"}
    with pytest.raises(RuntimeError):
        fused.control_stats()
    _, model, args, kw, _, _, _ = setup("ppo", dev, B)
    fused = learner_hip.FusedPPO(model, lr=LR, minibatch=M, use_graph=False, kl_stop=10.0)
    assert fused.ctl is not None and fused._graph_key() != (LR, 0.9, 0.999, 1e-5, 0, 0.2, 1.0, 0.125)
    fused.L = Spy(fused.L)
    assert len(fused.update(*args, **kw)) == 2
    assert {"orr_update_control", "orr_adam_step_ctl", "orr_ppo_head_logstd"} <= fused.L.called and "orr_adam_step" not in fused.L.called
