"""Running observation normalisation on the device: orr_running_stats_update, orr_normalize_rows and orr_policy_pack_norm against the
float64 references and bounds of tests/obs_norm_refs.py, the folded forward pass, FusedPPO against ppo.PPO on a normalised model, a
replayed GraphRollout after the statistics moved, and a model without a normaliser, which is what it was.  Every figure is printed before
it is asserted."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import learner_refs as lr
from tests import obs_norm_refs as onr

pytestmark = pytest.mark.gpu
CANARY = 4


def _dev():
    import torch
    return torch.device("cuda:0")


def _lib():
    from openroborl_amd import _lib
    return _lib.load()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _rec_tensor(rec):
    """a record dict -> the device words + a canary behind them"""
    import torch
    d = len(rec["mean"])
    w = np.zeros(4 + 3 * d + CANARY, np.float32)
    w[:2] = np.asarray([rec["count"]], np.int64).view(np.float32)
    w[4:4 + d], w[4 + d:4 + 2 * d], w[4 + 2 * d:4 + 3 * d] = rec["mean"], rec["var"], rec["rstd"]
    w[4 + 3 * d:] = np.float32(-7.25)
    return torch.from_numpy(w).to(_dev())


def _rec_dict(t, d):
    w = t.cpu().numpy()
    return {"count": int(w[:2].view(np.int64)[0]), "mean": w[4:4 + d].copy(), "var": w[4 + d:4 + 2 * d].copy(), "rstd": w[4 + 2 * d:4 + 3 * d].copy()}


def _update(rec_t, x, eps=onr.EPS):
    """one orr_running_stats_update of x (numpy or device) on the device record; checks both canaries; returns the partials"""
    import torch
    L = _lib()
    xt = torch.from_numpy(x).to(_dev()) if isinstance(x, np.ndarray) else x
    n, d = xt.shape
    need = int(L.orr_running_stats_partials(n, d))
    assert need == (n + onr.block_rows(d) - 1) // onr.block_rows(d) * 2 * d
    part = torch.full((need + CANARY,), -7.25, dtype=torch.float32, device=_dev())
    rc = L.orr_running_stats_update(xt.data_ptr(), n, d, float(eps), rec_t.data_ptr(), part.data_ptr(), _stream())
    assert rc == 0, L.orr_last_error()
    assert bool((part[need:] == -7.25).all()) and bool((rec_t[4 + 3 * d:] == -7.25).all()), "canary"
    return part[:need]


def _sizes(d):
    rows, side = onr.block_rows(d), onr.pass_rows(d)
    return sorted({n for n in (1, 7, 8, 9, 63, 64, 65, side - 1, side, side + 1, rows - 1, rows, rows + 1, 4096 * 3 + 1) if n >= 1})


@pytest.mark.parametrize("d", [160, 48, 4, 256])
def test_running_stats_update_matches_float64_on_every_edge_size(d):
    import torch
    worst = {}
    for n in _sizes(d):
        x = onr.columns(n, d, seed=1000 + n)
        rec_t = _rec_tensor(onr.fresh(d))
        part = _update(rec_t, x)
        got = _rec_dict(rec_t, d)
        r = onr.stats_ratios(got, [x])
        again = _rec_tensor(onr.fresh(d))
        part2 = _update(again, x)
        same = torch.equal(again, rec_t) and torch.equal(part, part2)
        exact = all(np.array_equal(lr.bits(got[g]), lr.bits(onr.stats_restate([x])[g])) for g in onr.GROUPS)
        print("d %3d n %6d: error / bound mean %.3g var %.3g rstd %.3g; count %d; two runs equal %s; equals the restatement %s"
              % (d, n, r["mean"], r["var"], r["rstd"], got["count"], same, exact))
        worst[n] = max(r.values())
        assert same
        assert np.array_equal(lr.bits(part.cpu().numpy()), lr.bits(onr.partials_restate(x).reshape(-1)))    # the float32 stage, operation for operation
        assert got["var"][onr.COL_CONST] == 0.0                    # a constant column has no variance, whatever its value
    assert max(worst.values()) <= 1.0, worst


def test_running_stats_update_at_the_workload_size():
    """262144 x 160, a segment of 8192 robots x 32 steps: one launch pair, 1024 workgroups"""
    n, d = 262144, 160
    x = onr.columns(n, d, seed=77)
    rec_t = _rec_tensor(onr.fresh(d))
    _update(rec_t, x)
    got = _rec_dict(rec_t, d)
    r = onr.stats_ratios(got, [x])
    print("262144 x 160: error / bound", r)
    assert max(r.values()) <= 1.0, r


def test_three_batches_merge_into_the_moments_of_their_concatenation():
    d = 160
    batches = [onr.columns(n, d, seed=30 + i, shift=s) for i, (n, s) in enumerate(((700, 0.0), (65, 1.5), (2049, -0.75)))]
    rec_t = _rec_tensor(onr.fresh(d))
    for i, x in enumerate(batches):
        _update(rec_t, x)
        r = onr.stats_ratios(_rec_dict(rec_t, d), batches[:i + 1])       # i = 0: a first update gives the batch's own moments
        print("after batch %d: error / bound" % i, r)
        assert max(r.values()) <= 1.0, (i, r)
    assert _rec_dict(rec_t, d)["count"] == 700 + 65 + 2049


def test_count_is_an_exact_integer_past_2_to_24():
    d = 48
    first, x = onr.columns(513, d, seed=40), onr.columns(700, d, seed=41, shift=0.5)
    seeded = dict(onr.stats_restate([first]), count=2 ** 24 + 1)
    rec_t = _rec_tensor(seeded)
    _update(rec_t, x)
    got = _rec_dict(rec_t, d)
    assert got["count"] == 2 ** 24 + 1 + 700 and int(np.float32(got["count"])) != got["count"]
    na = 2 ** 24 + 1
    n, mean, m2 = onr.chan64((na, seeded["mean"].astype(np.float64), seeded["var"].astype(np.float64) * na), onr.moments64(x))
    ref = {"mean": mean, "var": m2 / n, "rstd": onr.rstd64(m2 / n)}
    rest = onr.update_restate(seeded, x)
    for g in onr.GROUPS:
        ratio = lr.ratio_of(got[g], ref[g], lr.long_bound(rest[g], ref[g]))
        print("seeded count, %s: error / bound %.3g" % (g, ratio))
        assert ratio <= 1.0


def test_running_stats_refusals_write_nothing():
    import torch
    L = _lib()
    x = torch.from_numpy(onr.columns(64, 264, seed=1)).to(_dev())
    rec_t = _rec_tensor(onr.fresh(160))
    part = torch.full((4096,), -7.25, dtype=torch.float32, device=_dev())
    rec0, part0 = rec_t.clone(), part.clone()
    cases = {"d = 6": (x.data_ptr(), 64, 6, rec_t.data_ptr(), part.data_ptr()), "d = 260": (x.data_ptr(), 64, 260, rec_t.data_ptr(), part.data_ptr()),
             "n = 0": (x.data_ptr(), 0, 160, rec_t.data_ptr(), part.data_ptr()),
             "misaligned record": (x.data_ptr(), 64, 160, rec_t.data_ptr() + 4, part.data_ptr()),
             "misaligned x": (x.data_ptr() + 4, 64, 160, rec_t.data_ptr(), part.data_ptr()),
             "null partials": (x.data_ptr(), 64, 160, rec_t.data_ptr(), None)}
    for name, (xp, n, d, rp, pp) in cases.items():
        rc = L.orr_running_stats_update(xp, n, d, 1e-2, rp, pp, _stream())
        print("%s: %d %s" % (name, rc, L.orr_last_error().decode()))
        assert rc < 0 and b"orr_running_stats_update" in L.orr_last_error()
    assert L.orr_running_stats_update(x.data_ptr(), 64, 160, 0.0, rec_t.data_ptr(), part.data_ptr(), _stream()) < 0      # eps = 0
    assert L.orr_running_stats_partials(0, 160) == -1 and L.orr_running_stats_partials(64, 6) == -1
    assert L.orr_sizeof_running_stats(160) == 4 * (4 + 3 * 160) and L.orr_sizeof_running_stats(6) == -1
    torch.cuda.synchronize()
    assert torch.equal(rec_t, rec0) and torch.equal(part, part0)


@pytest.mark.parametrize("d", [160, 48])
def test_normalize_rows_within_two_roundings_and_in_place(d):
    import torch
    L = _lib()
    rec = onr.stats_restate([onr.columns(2049, d, seed=50)])
    mean_t, rstd_t = torch.from_numpy(rec["mean"]).to(_dev()), torch.from_numpy(rec["rstd"]).to(_dev())
    worst = 0.0
    for n in _sizes(d):
        x = onr.columns(n, d, seed=60 + n)
        xt = torch.from_numpy(x).to(_dev())
        out = torch.full((n * d + CANARY,), -7.25, dtype=torch.float32, device=_dev())
        assert L.orr_normalize_rows(xt.data_ptr(), n, d, mean_t.data_ptr(), rstd_t.data_ptr(), out.data_ptr(), _stream()) == 0, L.orr_last_error()
        got = out[:n * d].view(n, d)
        ratio = lr.ratio_of(got.cpu().numpy(), onr.normalize64(x, rec["mean"], rec["rstd"]), onr.normalize_bound(x, rec["mean"], rec["rstd"]))
        worst = max(worst, ratio)
        inplace = xt.clone()
        assert L.orr_normalize_rows(inplace.data_ptr(), n, d, mean_t.data_ptr(), rstd_t.data_ptr(), inplace.data_ptr(), _stream()) == 0
        assert torch.equal(inplace, got) and bool((out[n * d:] == -7.25).all())
        assert np.array_equal(lr.bits(got.cpu().numpy()), lr.bits(onr.normalize_restate(x, rec["mean"], rec["rstd"])))
    print("d %d: largest error / bound %.3g" % (d, worst))
    assert worst <= 1.0
    # refused: ranges that overlap without being equal, a misaligned table, d = 6; nothing is written
    buf = torch.zeros(64 * d + 8, dtype=torch.float32, device=_dev())
    keep = buf.clone()
    assert L.orr_normalize_rows(buf.data_ptr(), 64, d, mean_t.data_ptr(), rstd_t.data_ptr(), buf.data_ptr() + 16, _stream()) < 0
    assert b"overlap" in L.orr_last_error()
    assert L.orr_normalize_rows(buf.data_ptr(), 64, d, mean_t.data_ptr() + 4, rstd_t.data_ptr(), buf.data_ptr(), _stream()) < 0
    assert L.orr_normalize_rows(buf.data_ptr(), 64, 6, mean_t.data_ptr(), rstd_t.data_ptr(), buf.data_ptr(), _stream()) < 0
    assert L.orr_normalize_rows(buf.data_ptr(), 0, d, mean_t.data_ptr(), rstd_t.data_ptr(), buf.data_ptr(), _stream()) < 0
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)


@pytest.mark.parametrize("k,n", [(160, 512), (208, 512)])
def test_pack_norm_is_the_pack_of_the_scaled_matrix_and_the_folded_bias(k, n):
    import torch
    L = _lib()
    dev = _dev()
    rng = np.random.RandomState(k)
    w = lr.f32(rng.standard_normal((k, n)) * (2.0 / k) ** 0.5)
    b = lr.f32(0.1 * rng.standard_normal(n))
    mean = lr.f32(rng.uniform(-2.0, 2.0, k))
    rstd = lr.f32(1.0 / (np.exp(rng.uniform(np.log(0.05), np.log(3.0), k)) + 1e-2))
    wt, bt, mt, rt = (torch.from_numpy(v).to(dev) for v in (w, b, mean, rstd))
    size = int(L.orr_policy_packed_size(k, n))

    def pack_norm(m, r):
        out_w = torch.full((size + CANARY,), -7.25, dtype=torch.float32, device=dev)
        out_b = torch.full((n + CANARY,), -7.25, dtype=torch.float32, device=dev)
        assert L.orr_policy_pack_norm(wt.data_ptr(), k, n, m.data_ptr(), r.data_ptr(), bt.data_ptr(), out_w.data_ptr(), out_b.data_ptr(), _stream()) == 0, L.orr_last_error()
        assert bool((out_w[size:] == -7.25).all()) and bool((out_b[n:] == -7.25).all())
        return out_w[:size], out_b[:n]

    def pack(m):
        out = torch.empty(size, dtype=torch.float32, device=dev)
        assert L.orr_policy_pack(m.contiguous().data_ptr(), k, n, out.data_ptr(), _stream()) == 0
        return out
    img, fb = pack_norm(mt, rt)
    assert torch.equal(img, pack(rt[:, None] * wt))                       # one float32 multiplication per element
    _, b64 = onr.fold64(w, b, mean, rstd)
    ratio = lr.ratio_of(fb.cpu().numpy(), b64, onr.fold_bias_bound(w, b, mean, rstd))
    print("k %d: folded bias error / bound %.3g; equals the restatement %s" % (k, ratio, np.array_equal(lr.bits(fb.cpu().numpy()), lr.bits(onr.fold_restate(w, b, mean, rstd)[1]))))
    assert ratio <= 1.0
    assert np.array_equal(lr.bits(fb.cpu().numpy()), lr.bits(onr.fold_restate(w, b, mean, rstd)[1]))     # a float32 fmaf chain in a stated order
    assert lr.ratio_of(b, b64, onr.fold_bias_bound(w, b, mean, rstd)) > 1.0       # ... which a bias left alone does not meet
    img1, b1 = pack_norm(torch.zeros_like(mt), torch.ones_like(rt))        # the identity: orr_policy_pack's image and b, bit for bit
    assert torch.equal(img1, pack(wt)) and torch.equal(b1.view(torch.int32), bt.view(torch.int32))
    again = pack_norm(mt, rt)
    assert torch.equal(again[0], img) and torch.equal(again[1], fb)
    # refusals: orr_policy_pack's (k no multiple of 16), null or misaligned tables, a null bias; nothing is written
    out_w, out_b = torch.zeros(size, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
    args = lambda **kw: [kw.get(a, v) for a, v in (("w", wt.data_ptr()), ("k", k), ("n", n), ("mean", mt.data_ptr()), ("rstd", rt.data_ptr()),   # noqa: E731
                                                   ("b", bt.data_ptr()), ("out_w", out_w.data_ptr()), ("out_b", out_b.data_ptr()))] + [_stream()]
    for name, kw in (("k = 24", {"k": 24}), ("null mean", {"mean": None}), ("null rstd", {"rstd": None}), ("misaligned mean", {"mean": mt.data_ptr() + 4}),
                     ("misaligned rstd", {"rstd": rt.data_ptr() + 8}), ("null b", {"b": None}), ("null out_b", {"out_b": None}), ("null w", {"w": None})):
        rc = L.orr_policy_pack_norm(*args(**kw))
        print("%s: %d %s" % (name, rc, L.orr_last_error().decode()))
        assert rc < 0 and b"orr_policy_pack_norm" in L.orr_last_error()
    torch.cuda.synchronize()
    assert not bool(out_w.any()) and not bool(out_b.any())


def _fed_model(kw, seed=3, n=4096):
    """ActorCritic(obs_norm=True) on the device with non-trivial statistics, its twin without a normaliser, and the data behind them"""
    import torch
    from openroborl_amd import ppo
    dev = _dev()
    model, plain = ppo.ActorCritic(dev, seed=seed, obs_norm=True, **kw), ppo.ActorCritic(dev, seed=seed, **kw)
    obs = onr.columns(n, 160, seed=seed + 10)
    obs[:, onr.COL_OFFSET] = 3.0 + 0.25 * obs[:, onr.COL_TINY] * 1e4       # a plain column: 1000 +- 0.01 through rstd <= 100 swamps a float32 net
    priv = onr.columns(n, 48, seed=seed + 11) if kw else None
    if priv is not None:
        priv[:, onr.COL_OFFSET] = -1.0 + 0.5 * priv[:, onr.COL_TINY] * 1e4
    model.update_obs_norm(torch.from_numpy(obs).to(dev), *(() if priv is None else (torch.from_numpy(priv).to(dev),)))
    model.mark_updated()
    return model, plain, obs, priv


@pytest.mark.parametrize("kw", [{}, {"priv_dim": 48}, {"priv_dim": 48, "actor_priv_dim": 48}], ids=["plain", "priv", "teacher"])
def test_folded_forward_matches_the_float64_net_on_normalised_inputs(kw):
    """orr_policy_forward, _priv, _teacher on RAW inputs with the folded layer 0, and the same kernels with plain weights on
    orr_normalize_rows' output, both within the carried short bound of the float64 net on float64-normalised inputs"""
    import torch
    model, plain, obs, priv = _fed_model(kw)
    model.enable_fused()
    plain.enable_fused()
    p = {k: v.detach().cpu().numpy() for k, v in model.p.items()}
    om, orr = model.obs_norm.mean.cpu().numpy(), model.obs_norm.rstd.cpu().numpy()
    assert orr.max() > 10.0 * orr.min()
    for n in (1, 17, 256):
        o = torch.from_numpy(obs[:n]).to(_dev())
        pv = torch.from_numpy(priv[:n]).to(_dev()) if priv is not None else None
        _, _, v_f, mu_f = model.fused.forward(o, None, want_mean=True, priv=pv)
        on = model.obs_norm.normalize(o)
        pn = model.priv_norm.normalize(pv) if pv is not None else None
        _, _, v_n, mu_n = plain.fused.forward(on, None, want_mean=True, priv=pn)
        for net, folded, normed in (("pi", mu_f, mu_n), ("vf", v_f[:, None], v_n[:, None])):
            wide = p["model/%s_fc0/w:0" % net].shape[0] == 208
            x = np.concatenate((obs[:n], priv[:n]), axis=1) if wide else obs[:n]
            mean = np.concatenate((om, model.priv_norm.mean.cpu().numpy())) if wide else om
            rstd = np.concatenate((orr, model.priv_norm.rstd.cpu().numpy())) if wide else orr
            _, ref = onr.mlp64(p, net, onr.normalize64(x, mean, rstd))
            bound = onr.folded_forward_bound(p, net, x, mean, rstd)
            rf, rn = lr.ratio_of(folded.cpu().numpy(), ref, bound), lr.ratio_of(normed.cpu().numpy(), ref, bound)
            _, raw = onr.mlp64(p, net, x.astype(np.float64))
            print("%s n %3d %s: folded error / bound %.3g, plain weights on normalised inputs %.3g; the nets on raw inputs are %.3g bounds away"
                  % (sorted(kw), n, net, rf, rn, lr.ratio_of(raw, ref, bound)))
            assert rf <= 1.0 and rn <= 1.0
            assert lr.ratio_of(raw, ref, bound) > 1.0                    # the bound tells the fold from its absence


def _batch(model, obs, priv, seed):
    """test_gpu_learner's synthetic batch on given observations: ratios that leave [0.8, 1.2] for part of it, advantages with zeros"""
    import torch
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    B = obs.shape[0]
    with torch.no_grad():
        mu = model.mean(obs, model.actor_priv(priv))
    act = mu + 0.125 * torch.randn(B, 12, generator=g).to(dev)
    shifted = mu + 0.04 * torch.randn(B, 12, generator=g).to(dev)
    old = (-0.5 * ((act - shifted) ** 2) / 0.125 ** 2 - 0.5 * math.log(2.0 * math.pi * 0.125 ** 2)).sum(dim=1)
    adv = torch.randn(B, generator=g).to(dev)
    adv[::97] = 0.0
    return act, old, adv, torch.randn(B, generator=g).to(dev)


@pytest.mark.parametrize("kw", [{}, {"priv_dim": 48}], ids=["plain", "priv"])
def test_fused_ppo_matches_the_torch_learner_on_a_normalised_model(kw):
    """test_fused_update_matches_the_torch_learner's comparison at (graph=True, B=8192, M=1024), with its tolerances, both learners on
    ActorCritic(obs_norm=True) with non-trivial statistics; the observations are per-column offset + scale x a standard normal, so a learner
    that skipped the normaliser would train on other inputs than its twin.  The standard normal is that test's own draw (generator seed 1).

    What the parameter tolerance of that test is sensitive to, measured on an MI355X with and without the normaliser, with and without the
    privileged rows, four data seeds each (16 runs): in 11 the two learners' parameters agree to 6e-8 after the 32 steps; in 5 one hidden
    unit of the critic takes the other side of the ReLU's kink in one learner at some step, and one column of model/vf_fc1/w:0 (and what
    is behind it) then differs by 1e-6 to 1e-4 - 2.2e-5 and 1.6e-5 without the normaliser, 9.7e-6, 4.3e-5 and, once, 9.65e-5 with it,
    against the 6.4e-5 allowed.  The normaliser has no part in it: both learners read the same normalised bits (asserted below)."""
    import torch
    from openroborl_amd import learner_hip, ppo
    dev = _dev()
    B, M, lr_ = 8192, 1024, 1e-4
    rng, g = np.random.RandomState(5), torch.Generator().manual_seed(1)

    def data(d):
        off, scale = rng.uniform(-2.0, 2.0, d), np.exp(rng.uniform(np.log(0.05), np.log(3.0), d))
        return (torch.from_numpy(lr.f32(off)) + torch.from_numpy(lr.f32(scale)) * torch.randn(B, d, generator=g)).to(dev)
    obs, priv = data(160), (data(48) if kw else None)
    models = []
    for _ in range(2):
        m = ppo.ActorCritic(dev, seed=2, obs_norm=True, **kw)
        m.update_obs_norm(obs[:4096], *(() if priv is None else (priv[:4096],)))
        models.append(m)
    ref_model, model = models
    assert torch.equal(ref_model.obs_norm.rec, model.obs_norm.rec) and float(model.obs_norm.rstd.max()) > 5.0 * float(model.obs_norm.rstd.min())
    act, old, adv, ret = _batch(ref_model, obs, priv, seed=1)
    before = {k: v.detach().clone() for k, v in model.p.items()}
    stats = model.obs_norm.rec.clone()
    ref = ppo.PPO(ref_model, lr=lr_, minibatch=M)
    fused = learner_hip.FusedPPO(model, lr=lr_, minibatch=M, use_graph=True)
    for it in range(2):
        g1, g2 = torch.Generator(device=dev), torch.Generator(device=dev)
        g1.manual_seed(10 + it); g2.manual_seed(10 + it)
        s_ref = ref.update(obs, act, adv, ret, old_logp=old, epochs=2, generator=g1, priv=priv)
        s_fused = fused.update(obs, act, adv, ret, old_logp=old, epochs=2, generator=g2, priv=priv)
        print("update %d: torch %s fused %s" % (it, s_ref, s_fused))
        np.testing.assert_allclose(s_fused, s_ref, rtol=2e-4, atol=2e-5)
    assert fused.steps_taken() == 2 * 2 * (B // M)
    moved = 0.0
    for k in sorted(before):
        a, b = ref_model.p[k].detach(), model.p[k].detach()
        moved = max(moved, (a - before[k]).abs().max().item())
        print("%-20s max difference %.3g mean %.3g (of %g)" % (k, (a - b).abs().max().item(), (a - b).abs().mean().item(), 32 * lr_))
        kink = ("the data seeds are pinned: with other draws a hidden unit may take the other side of the ReLU's kink in one learner and one "
                "column differs by up to 1e-4, with or without the normaliser (see the docstring)")
        assert (a - b).abs().max().item() < 0.02 * 32 * lr_, (k, (a - b).abs().max().item(), kink)
        assert (a - b).abs().mean().item() < 2e-3 * 32 * lr_, (k, (a - b).abs().mean().item(), kink)
    assert moved > 10 * lr_
    assert torch.equal(model.obs_norm.rec, stats) and torch.equal(ref_model.obs_norm.rec, stats)      # an update leaves the statistics alone
    # the learner's static input is the normalised batch; old_logp=None goes through the model's normalising log_prob
    P = fused._plan(B, M)
    assert torch.equal(P["obs"], model.obs_norm.apply(obs)) and (priv is None or torch.equal(P["priv"], model.priv_norm.apply(priv)))
    with torch.no_grad():
        want = model.log_prob(obs, act)
    g2 = torch.Generator(device=dev)
    g2.manual_seed(3)
    assert np.isfinite(fused.update(obs, act, adv, ret, epochs=1, generator=g2, priv=priv)).all()
    assert torch.equal(P["aux"][:, 12], want) and not torch.equal(want, old)


def test_graph_rollout_replays_with_the_new_statistics():
    """After update_obs_norm + mark_updated a REPLAYED segment acts by the new statistics: its actions equal an eager model.act on the same
    observations and noise bit for bit, and differ from what the statistics before gave"""
    import torch
    from openroborl_amd import ppo, rollout
    from openroborl_amd.env import VecQuadrupedEnv
    dev = _dev()
    n, T = 64, 4
    env = VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=n, mode="train", auto_reset=True, seed=11, device=dev)
    model = ppo.ActorCritic(dev, seed=1, obs_norm=True, priv_dim=48).enable_fused()
    collector = rollout.GraphRollout(env, model, T)
    gen = torch.Generator(device=dev).manual_seed(0)
    obs, priv = env.reset(), None
    for it in range(3):                                    # eager, captured, replayed
        buf = collector.collect(obs, generator=gen, priv=priv)
        obs, priv = buf["last_obs"], buf["last_priv"]
    graph = collector.graph
    o0, p0, noise = buf["obs"][0].clone(), buf["priv"][0].clone(), collector.noise.clone()
    with torch.no_grad():
        old_raw = model.act(o0, p0, noise=noise[0])[1].clone()
    assert torch.equal(old_raw, buf["actions"][0])         # identity statistics so far
    model.update_obs_norm(buf["obs"].reshape(T * n, 160), buf["priv"].reshape(T * n, 48))
    model.mark_updated()
    buf = collector.collect(obs, noise=noise, priv=priv)
    assert collector.graph is graph                        # replayed, not captured again
    o1, p1 = buf["obs"][0].clone(), buf["priv"][0].clone()
    seg_raw, seg_val = buf["actions"][0].clone(), buf["vpred"][0].clone()
    with torch.no_grad():
        _, raw, val = model.act(o1, p1, noise=noise[0])
        torch_mu = model.mean(o1)
        stale = ppo.ActorCritic(dev, seed=1, priv_dim=48).enable_fused().act(o1, p1, noise=noise[0])[1]
    print("replayed against eager: equal %s; against the identity statistics: max difference %.3g; fused mean against torch's normalising mean %.3g"
          % (torch.equal(raw, seg_raw), (stale - seg_raw).abs().max().item(), (seg_raw - 0.125 * noise[0] - torch_mu).abs().max().item()))
    assert torch.equal(raw, seg_raw) and torch.equal(val, seg_val)
    assert not torch.equal(stale, seg_raw)
    assert (seg_raw - 0.125 * noise[0] - torch_mu).abs().max().item() < 1e-4
    assert model.obs_norm.count == T * n
    env.close()


def test_a_model_without_a_normaliser_is_what_it_was():
    """refresh() packs what orr_policy_pack gives called directly, the biases are the parameters', forward() the same outputs as a
    FusedActorCritic built without the new arguments"""
    import torch
    from openroborl_amd import policy_hip, ppo
    L = _lib()
    dev = _dev()
    model = ppo.ActorCritic(dev, seed=7, priv_dim=48).enable_fused()
    assert model.obs_norm is None and model.fused.obs_norm is None and model.fused._norm_tab is None
    for field, key in policy_hip.KEYS:
        w = model.p[key].detach()
        if field.startswith("w"):
            out = torch.empty_like(model.fused.packed[field])
            assert L.orr_policy_pack(w.data_ptr(), int(w.shape[0]), int(w.shape[1]), out.data_ptr(), _stream()) == 0
            assert torch.equal(out, model.fused.packed[field]), field
        else:
            assert torch.equal(model.fused.biases[field], w), field
    bare = policy_hip.FusedActorCritic(model.p, dev, std=0.125)
    obs, priv, noise = torch.randn(17, 160, device=dev), torch.randn(17, 48, device=dev), torch.randn(17, 12, device=dev)
    for a, b in zip(model.fused.forward(obs, noise, want_mean=True, priv=priv), bare.forward(obs, noise, want_mean=True, priv=priv)):
        assert torch.equal(a, b)
