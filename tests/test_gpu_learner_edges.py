"""The learner-side kernels (include/openroborl_learner.h, orr_gae_flags) at the edges of their index arithmetic: every admitted column
width, row counts around a workgroup's and a tile's size, both paths of the column sum and their switch, ties of the clip rule, large step
counts, the legacy GAE index across a workgroup's edge.  Each output against float64 within the bound tests/learner_refs.py derives for it
(tests/test_learner_refs_cpu.py shows on the CPU that these comparisons reject seeded defects); selects and exact zeros bit for bit.
Every output and the workspace sit between guard words of a NaN pattern, and a workspace is filled with it: a write out of range or a read of
a word nobody wrote fails an assertion.  Each test prints `EDGE <group> <largest error / bound>`; DESIGN.md section 3 records them."""
import ctypes as C

import numpy as np
import pytest

from tests import learner_refs as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GUARD = 64                       # words on either side: 256 bytes, so the words between them keep the allocation's alignment
SENTINEL = 0x7FC0BEEF            # a quiet NaN no kernel produces
STD, CLIP, VF = 0.125, 0.2, 0.5
_CTX = {}


def ctx():
    """the library, loaded once per module"""
    if not _CTX:
        import torch
        from openroborl_amd import _abi, _lib
        _CTX.update(torch=torch, _lib=_lib, _abi=_abi, L=_lib.load(), dev=torch.device("cuda:0"))
    return _CTX["torch"], _CTX["_lib"], _CTX["L"], _CTX["dev"]


def stream():
    torch, _, _, dev = ctx()
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class Guarded(object):
    """n words of device memory between guard words; filled with the sentinel, or with `init`"""

    def __init__(self, n, init=None, dtype=None):
        torch, _, _, dev = ctx()
        self.n = int(n)
        self.whole = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.i = self.whole[GUARD:GUARD + self.n]
        self.t = self.i.view(dtype or torch.float32)
        if init is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(init)).reshape(-1).to(dev))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.whole[:GUARD] == SENTINEL).all()) and bool((self.whole[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.whole == SENTINEL).all())

    def np(self, *shape):
        a = self.t.cpu().numpy()
        return a.reshape(shape) if shape else a


def intact(*bufs):
    return all(b.guards_intact() for b in bufs)


def report(group, ratio):
    print("EDGE %s %.3f" % (group, ratio))
    return ratio


def within(group, got, ref, bound):
    r = report(group, R.ratio_of(got, ref, bound))
    assert r <= 1.0, (group, r)


def workspace(m, c):
    _, _, L, _ = ctx()
    return Guarded(int(L.orr_learner_workspace_floats(m, c)))


def refused(rc, who):
    _, _, L, _ = ctx()
    return rc == -1 and who in L.orr_last_error()


# ---- orr_relu_backward ----------------------------------------------------------------------------------------------------------------------

def run_relu(g, h):
    _, _lib, L, _ = ctx()
    m, c = h.shape
    dg, dh, gb = Guarded(m * c, g), Guarded(m * c, h), Guarded(c)
    ws = Guarded(int(L.orr_learner_partial_rows(m)) * c)               # [rows][c], as the trainer sizes ws1
    _lib.check(L.orr_relu_backward(dg.ptr, dh.ptr, m, c, gb.ptr, ws.ptr, stream()), L)
    assert intact(dg, dh, gb, ws) and np.array_equal(R.bits(dh.np(m, c)), R.bits(h))
    return dg.np(m, c), gb.np()


@pytest.mark.parametrize("c", R.RELU_COLS)
def test_relu_backward_over_every_admitted_width(c):
    worst = 0.0
    for m in R.RELU_ROWS:
        g, h = R.relu_data(m, c)
        out, gb = run_relu(g, h)
        assert np.array_equal(R.bits(out), R.bits(R.relu_select(g, h))), (m, c)            # a select: g in or +0.0
        worst = max(worst, R.ratio_of(gb, *R.relu_backward_ref(g, h)))
        out2, gb2 = run_relu(g, h)
        assert np.array_equal(R.bits(out), R.bits(out2)) and np.array_equal(R.bits(gb), R.bits(gb2))
    assert report("relu_backward.gb", worst) <= 1.0


@pytest.mark.parametrize("c", R.RELU_COLS)
def test_relu_backward_keeps_poison_behind_the_mask(c):
    """NaN and +-Inf in g where h == 0; -0.0 and denormals of both signs in h: the output and the column sums are what h > 0 says"""
    m = 65
    g, h = R.relu_data(m, c, seed=1)
    gf, hf = g.reshape(-1), h.reshape(-1)
    z = np.flatnonzero(hf == 0)
    assert len(z) >= 8
    gf[z[0::4]], gf[z[1::4]], gf[z[2::4]] = np.nan, np.inf, -np.inf
    hf[z[1::4]], hf[z[2::4]], hf[z[3::4]] = -0.0, -1e-40, 1e-40            # z[3::4]: a positive denormal keeps its (finite) g
    out, gb = run_relu(g, h)
    want = R.relu_select(g, h)
    assert np.isfinite(want).all() and (want.reshape(-1)[z[3::4]] == gf[z[3::4]]).all()
    assert np.array_equal(R.bits(out), R.bits(want))
    with np.errstate(invalid="ignore"):
        within("relu_backward.gb_poisoned", gb, *R.relu_backward_ref(np.where(h > 0, g, F32(0.0)), h))


def test_relu_backward_refusals_write_nothing():
    _, _, L, _ = ctx()
    m = 33
    for c in (0, 2, 6, 12, 2048):
        assert not R.cols_ok(c)
        g, h, gb, ws = Guarded(m * max(c, 4)), Guarded(m * max(c, 4)), Guarded(max(c, 4)), Guarded(2 * max(c, 4))
        assert refused(L.orr_relu_backward(g.ptr, h.ptr, m, c, gb.ptr, ws.ptr, stream()), b"orr_relu_backward"), c
        assert g.untouched() and gb.untouched() and ws.untouched()
    for bad in range(3):         # g, h, the workspace four bytes off
        g, h, gb, ws = Guarded(m * 16 + 4), Guarded(m * 16 + 4), Guarded(16), Guarded(2 * 16 + 4)
        ptrs = [g.ptr, h.ptr, ws.ptr]
        ptrs[bad] += 4
        assert refused(L.orr_relu_backward(ptrs[0], ptrs[1], m, 16, gb.ptr, ptrs[2], stream()), b"orr_relu_backward"), bad
        assert g.untouched() and gb.untouched() and ws.untouched()


# ---- orr_head_backward ----------------------------------------------------------------------------------------------------------------------

def run_head_backward(gy, w, h, deferred=False):
    _, _lib, L, _ = ctx()
    abi = _CTX["_abi"]
    (m, c), k = h.shape, gy.shape[1]
    dgy, dw, dh = Guarded(m * k, gy), Guarded(c * k, w), Guarded(m * c, h)
    gz, gb, gw, ws = Guarded(m * c), Guarded(c), Guarded(c * k), workspace(m, c)
    if not deferred:
        _lib.check(L.orr_head_backward(dgy.ptr, k, dw.ptr, dh.ptr, m, c, gz.ptr, gb.ptr, gw.ptr, ws.ptr, stream()), L)
    else:
        rows = int(L.orr_learner_partial_rows(m))
        _lib.check(L.orr_head_backward(dgy.ptr, k, dw.ptr, dh.ptr, m, c, gz.ptr, None, None, ws.ptr, stream()), L)
        jobs = (abi.OrrColsumJob * 2)(abi.OrrColsumJob(ws.ptr, gb.ptr, rows, c), abi.OrrColsumJob(ws.ptr + 4 * rows * c, gw.ptr, rows, c * k))
        _lib.check(L.orr_colsum_finish(jobs, 2, stream()), L)
    assert intact(dgy, dw, dh, gz, gb, gw, ws)
    return {"gz": gz.np(m, c), "gb": gb.np(), "gw": gw.np(c, k)}


@pytest.mark.parametrize("k", R.HEADB_K)
@pytest.mark.parametrize("c", R.HEADB_COLS)
def test_head_backward_over_widths_and_fan_outs(c, k):
    worst = {"gz": 0.0, "gb": 0.0, "gw": 0.0}
    for m in R.HEADB_ROWS:
        gy, w, h = R.head_backward_data(m, c, k)
        got, ref = run_head_backward(gy, w, h), R.head_backward_ref(gy, w, h)
        for name in worst:
            worst[name] = max(worst[name], R.ratio_of(got[name], *ref[name]))
        assert not (R.bits(got["gz"][h == 0])).any()                                       # masked by a select: +0.0
        again = run_head_backward(gy, w, h, deferred=True)
        for name in worst:
            assert np.array_equal(R.bits(got[name]), R.bits(again[name])), (name, m)
    for name in worst:
        assert report("head_backward.k%d.%s" % (k, name), worst[name]) <= 1.0, (name, c, k)


@pytest.mark.parametrize("k", R.HEADB_K)
@pytest.mark.parametrize("c", R.HEADB_COLS)
def test_head_backward_keeps_poison_behind_the_mask(c, k):
    """dead units (h == 0 in every row) whose output weights are NaN or +-Inf: gz is masked by a select, gw = h^T gy reads the finite h"""
    m = 33
    gy, w, h = R.head_backward_data(m, c, k, seed=1)
    dead = np.arange(c) % 3 == 1
    h[:, dead] = 0.0
    w[dead] = np.array([np.nan, np.inf, -np.inf], dtype=F32)[np.arange(dead.sum()) % 3][:, None]
    got = run_head_backward(gy, w, h)
    assert np.isfinite(got["gz"]).all() and np.isfinite(got["gb"]).all() and np.isfinite(got["gw"]).all()
    assert not R.bits(got["gz"][:, dead]).any() and not (got["gb"][dead] != 0).any() and not (got["gw"][dead] != 0).any()
    clean = np.where(dead[:, None], F32(0.0), w)
    ref = R.head_backward_ref(gy, clean, h)
    for name in ("gz", "gb", "gw"):
        within("head_backward_poisoned.k%d.%s" % (k, name), got[name], *ref[name])


# ---- orr_colsum_finish on its own ------------------------------------------------------------------------------------------------------------

def run_colsum(tables):
    """tables: [partials [rows, cols]] -> their column sums from ONE launch"""
    _, _lib, L, _ = ctx()
    abi = _CTX["_abi"]
    ins = [Guarded(p.size, p) for p in tables]
    outs = [Guarded(p.shape[1]) for p in tables]
    jobs = (abi.OrrColsumJob * len(tables))(*(abi.OrrColsumJob(i.ptr, o.ptr, p.shape[0], p.shape[1]) for i, o, p in zip(ins, outs, tables)))
    _lib.check(L.orr_colsum_finish(jobs, len(tables), stream()), L)
    assert intact(*(ins + outs))
    return [o.np() for o in outs]


def colsum_table(rows, cols, seed):
    return R.mixed(np.random.RandomState(seed * 100003 + rows * 1000 + cols), rows, cols)


@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_finish_single_jobs(rows):
    worst = 0.0
    for cols in R.COLSUM_COLS:
        p = colsum_table(rows, cols, 0)
        out, = run_colsum([p])
        worst = max(worst, R.ratio_of(out, *R.colsum_ref(p)))
        again, = run_colsum([p])
        assert np.array_equal(R.bits(out), R.bits(again)), (rows, cols)
    assert report("colsum_finish.%s" % ("few" if rows <= R.K_FEW else "many"), worst) <= 1.0, rows


@pytest.mark.parametrize("shapes", [
    # twelve jobs, the two paths in turn, unequal column counts (so every job's first workgroup sits at another place of the prefix table)
    [(16, 257), (17, 15), (1, 1), (65, 256), (15, 17), (513, 255), (8, 300), (49, 16), (16, 1), (127, 31), (2, 513), (64, 5)],
    # the first job has a single column
    [(17, 1), (3, 257), (65, 1), (1, 15)]])
def test_colsum_finish_tables_that_mix_both_paths(shapes):
    tables = [colsum_table(r, c, 1 + j) for j, (r, c) in enumerate(shapes)]
    outs = run_colsum(tables)
    worst = max(R.ratio_of(o, *R.colsum_ref(p)) for o, p in zip(outs, tables))
    assert report("colsum_finish.table", worst) <= 1.0
    for a, b in zip(outs, run_colsum(tables)):
        assert np.array_equal(R.bits(a), R.bits(b))
    for j, p in enumerate(tables):           # a job of a table gives the bits it gives alone: no job reads another's rows
        assert np.array_equal(R.bits(outs[j]), R.bits(run_colsum([p])[0])), j


def test_colsum_finish_refusals_write_nothing():
    _, _, L, _ = ctx()
    abi = _CTX["_abi"]
    p, o = Guarded(64, np.ones(64, dtype=F32)), Guarded(16)
    good = abi.OrrColsumJob(p.ptr, o.ptr, 4, 16)
    for n, jobs in ((0, [good]), (13, [good] * 13), (1, [abi.OrrColsumJob(p.ptr, o.ptr, 0, 16)]), (1, [abi.OrrColsumJob(p.ptr, o.ptr, 4, 0)]),
                    (2, [good, abi.OrrColsumJob(p.ptr, o.ptr, 0, 16)])):
        assert refused(L.orr_colsum_finish((abi.OrrColsumJob * len(jobs))(*jobs), n, stream()), b"orr_colsum_finish"), n
        assert o.untouched()


# ---- orr_ppo_head, orr_ppo_head_logstd -------------------------------------------------------------------------------------------------------

def run_ppo_head(mean, value, batch, clip, log_std=None, ent_coef=0.0):
    _, _lib, L, _ = ctx()
    m = len(mean)
    dm, dv, db = Guarded(m * 12, mean), Guarded(m, value), Guarded(m * 16, batch)
    gm, gv, gbm, gbv = Guarded(m * 12), Guarded(m), Guarded(12), Guarded(1)
    if log_std is None:
        stats, ws = Guarded(2), workspace(m, 16)
        _lib.check(L.orr_ppo_head(dm.ptr, dv.ptr, db.ptr, m, STD, clip, VF, gm.ptr, gv.ptr, gbm.ptr, gbv.ptr, stats.ptr, ws.ptr, stream()), L)
        bufs = (dm, dv, db, gm, gv, gbm, gbv, stats, ws)
    else:
        stats, ws, dls, gls = Guarded(5), workspace(m, 32), Guarded(12, log_std), Guarded(12)
        _lib.check(L.orr_ppo_head_logstd(dm.ptr, dv.ptr, db.ptr, dls.ptr, m, clip, VF, ent_coef, gm.ptr, gv.ptr, gls.ptr, gbm.ptr, gbv.ptr, stats.ptr,
                                         ws.ptr, stream()), L)
        bufs = (dm, dv, db, gm, gv, gbm, gbv, stats, ws, dls, gls)
    assert intact(*bufs)
    s = stats.np()
    out = {"g_mean": gm.np(m, 12), "g_value": gv.np(), "gb_mean": gbm.np(), "gb_value": gbv.np()[0], "surr": s[0], "vloss": s[1]}
    if log_std is not None:
        out.update({"entropy": s[2], "kl": s[3], "clipfrac": s[4], "g_logstd": gls.np()})
    return out


def check_ppo_head(tag, data, clip, log_std=None, ent_coef=0.0):
    mean, value, batch = data
    ref = R.ppo_head_ref(mean, value, batch, STD, clip, VF, log_std, ent_coef)
    restated = R.ppo_head_restate(mean, value, batch, STD, clip, VF, log_std, ent_coef)
    B = R.ppo_head_bounds(ref, restated, VF)
    got = run_ppo_head(mean, value, batch, clip, log_std, ent_coef)
    for k in sorted(B):
        within("%s.%s" % (tag, k), got[k], ref[k], B[k])
    near = R.near_clip_edge(ref, restated, clip) if clip > 0 else np.zeros(len(mean), dtype=bool)
    assert near.mean() <= 0.01
    # a sample whose float64 gradient is exactly zero (A = 0, or clipped on the constant side) gets zeros (of the sign its product gives)
    keep = ref["dead"] & ~near
    assert not (R.bits(got["g_mean"][keep]) & 0x7FFFFFFF).any()
    if log_std is not None and not near.any():
        assert got["clipfrac"] == F32(ref["clipfrac"]), (got["clipfrac"], ref["clipfrac"])
    again = run_ppo_head(mean, value, batch, clip, log_std, ent_coef)
    for k in got:
        assert np.array_equal(R.bits(got[k]), R.bits(again[k])), k
    return got, ref, restated


@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("m", R.HEAD_ROWS)
def test_ppo_head_at_workgroup_and_row_group_edges(m, spread):
    check_ppo_head("ppo_head" + (".spread" if spread else ""), R.head_data(m, STD, None, spread), CLIP)


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("m", R.HEAD_ROWS)
def test_ppo_head_logstd_at_workgroup_and_row_group_edges(m, spread, ent_coef):
    ls = R.uneven_log_std()
    check_ppo_head("ppo_head_logstd" + (".spread" if spread else ""), R.head_data(m, STD, ls, spread), CLIP, ls, ent_coef)


@pytest.mark.parametrize("logstd", [False, True])
@pytest.mark.parametrize("m", [257, 769])
def test_ppo_heads_on_the_constructed_tie(m, logstd):
    """act == mean and old log-probability == log_norm: ratio exactly 1, clip = 0, advantages of both signs and zero.  The reference is the
    float64 autograd of ppo.PPO.update's formula; every g_mean is a zero whose sign the clip rule decides."""
    torch = ctx()[0]
    ls = R.uneven_log_std() if logstd else None
    log_norm = R.log_norm_of(ls) if logstd else R.ppo_head_scalars(m, STD)["log_norm"]
    data = R.tie_data(m, log_norm)
    got, ref, restated = check_ppo_head("ppo_head%s.tie" % ("_logstd" if logstd else ""), data, 0.0, ls, 0.0)
    tie = np.arange(m) % 5 != 0
    assert (ref["ratio"][tie] == 1.0).all() and (restated["ratio"][tie] == 1.0).all()
    assert np.array_equal(R.bits(got["g_mean"]), R.bits(restated["g_mean"]))
    # float64 autograd of the formula, on the float32 constants the kernel is given
    mean, value, batch = (torch.from_numpy(np.asarray(x, F64)) for x in data)
    mu, v = mean.clone().requires_grad_(True), value.clone().requires_grad_(True)
    if ls is None:
        inv_std = torch.sqrt(torch.tensor(float(R.ppo_head_scalars(m, STD)["inv_var"]), dtype=torch.float64)).expand(12)
    else:
        inv_std = torch.exp(-torch.from_numpy(np.asarray(ls, F64)))
    logp = -0.5 * (((batch[:, :12] - mu) * inv_std) ** 2).sum(dim=1) + float(log_norm)
    ratio = torch.exp(logp - batch[:, 12])
    adv = batch[:, 13]
    surr = -torch.min(ratio * adv, torch.clamp(ratio, 1.0, 1.0) * adv).mean()
    vf = ((v - batch[:, 14]) ** 2).mean()
    (surr + VF * vf).backward()
    assert bool((ratio[torch.from_numpy(tie)] == 1.0).all()) and not bool(mu.grad.any())
    B = R.ppo_head_bounds(ref, restated, VF)
    within("ppo_head.tie_autograd.surr", got["surr"], surr.item(), B["surr"] + 4 * R.U * abs(surr.item()))        # 1 / m: float32 there, exact here
    within("ppo_head.tie_autograd.g_value", got["g_value"], v.grad.numpy(), 2 * B["g_value"] + 1e-30)
    assert not got["g_mean"].any() and not got["gb_mean"].any()


# ---- orr_distill_head, orr_regress_head ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", R.SMALL_HEAD_ROWS)
def test_distill_head_edges(m):
    _, _lib, L, _ = ctx()
    rng = np.random.RandomState(m)
    mean, target = R.mixed(rng, m, 12), R.mixed(rng, m, 12)
    dm, dt, g, gb, stats, ws = Guarded(m * 12, mean), Guarded(m * 12, target), Guarded(m * 12), Guarded(12), Guarded(1), workspace(m, 16)
    _lib.check(L.orr_distill_head(dm.ptr, dt.ptr, m, g.ptr, gb.ptr, stats.ptr, ws.ptr, stream()), L)
    assert intact(dm, dt, g, gb, stats, ws)
    ref = R.distill_head_ref(mean, target)
    for k, x in (("g_mean", g.np(m, 12)), ("gb_mean", gb.np()), ("loss", stats.np()[0])):
        within("distill_head." + k, x, *ref[k])


@pytest.mark.parametrize("c", R.REGRESS_COLS)
def test_regress_head_edges(c):
    _, _lib, L, _ = ctx()
    worst = {"g": 0.0, "gb": 0.0, "loss": 0.0}
    for m in R.SMALL_HEAD_ROWS:
        rng = np.random.RandomState(100 * c + m)
        pred, target = R.mixed(rng, m, c), R.mixed(rng, m, c)
        dp, dt, g, gb, stats, ws = Guarded(m * c, pred), Guarded(m * c, target), Guarded(m * c), Guarded(c), Guarded(1), workspace(m, 64)
        _lib.check(L.orr_regress_head(dp.ptr, dt.ptr, m, c, g.ptr, gb.ptr, stats.ptr, ws.ptr, stream()), L)
        assert intact(dp, dt, g, gb, stats, ws)
        ref = R.regress_head_ref(pred, target)
        for k, x in (("g", g.np(m, c)), ("gb", gb.np()), ("loss", stats.np()[0])):
            worst[k] = max(worst[k], R.ratio_of(x, *ref[k]))
    for k in worst:
        assert report("regress_head." + k, worst[k]) <= 1.0, (k, c)


def test_regress_head_refusals_write_nothing():
    _, _, L, _ = ctx()
    m = 65
    for c in (0, 2, 68):
        n = m * max(c, 4)
        dp, dt, g, gb, stats, ws = Guarded(n, np.ones(n, dtype=F32)), Guarded(n, np.ones(n, dtype=F32)), Guarded(n), Guarded(max(c, 4)), Guarded(1), workspace(m, 64)
        assert refused(L.orr_regress_head(dp.ptr, dt.ptr, m, c, g.ptr, gb.ptr, stats.ptr, ws.ptr, stream()), b"orr_regress_head"), c
        assert g.untouched() and gb.untouched() and stats.untouched() and ws.untouched()


# ---- orr_gauss_prepare -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gauss_prepare_at_workgroup_edges(n):
    """what tests/test_gpu_learn_std.py leaves out: the sizes around one workgroup, log-stds over the trainer's whole range, guard words"""
    _, _lib, L, _ = ctx()
    rng = np.random.RandomState(n)
    noise, ls = F32(rng.standard_normal((n, 12))), R.uneven_log_std()
    want, want_logp = R.gauss_prepare_ref(noise, ls)
    r_scaled, r_logp = R.gauss_prepare_restate(noise, ls)
    b_scaled, b_logp = R.long_bound(r_scaled / want, np.ones_like(want), "gauss.scaled"), R.long_bound(r_logp, want_logp, "gauss.logp")
    first = None
    for in_place in (False, True):
        for with_logp in (True, False):
            src, dls, logp = Guarded(n * 12, noise), Guarded(12, ls), Guarded(n)
            dst = src if in_place else Guarded(n * 12)
            _lib.check(L.orr_gauss_prepare(src.ptr, dls.ptr, dst.ptr, logp.ptr if with_logp else None, n, stream()), L)
            assert intact(src, dst, dls, logp)
            scaled = dst.np(n, 12)
            within("gauss_prepare.scaled", scaled / want, np.ones_like(want), b_scaled)          # relative: the stds span two decades
            if with_logp:
                within("gauss_prepare.logp", logp.np(), want_logp, b_logp)
            else:
                assert logp.untouched()
            if not in_place:
                assert np.array_equal(R.bits(src.np(n, 12)), R.bits(noise))
            if first is None:
                first = (scaled, logp.np())
            assert np.array_equal(R.bits(scaled), R.bits(first[0])) and (not with_logp or np.array_equal(R.bits(logp.np()), R.bits(first[1])))


# ---- orr_adam_step, orr_adam_step_ctl --------------------------------------------------------------------------------------------------------

HYPER = (1e-3, 0.9, 0.999, 1e-5)


def run_adam(n, p, g, m, v, t0, gscale, flags, ctl=None):
    """three steps from state = [t0, 0] -> (p, m, v, state); the buffers end AT n: the guard words start there"""
    torch, _lib, L, _ = ctx()
    dp, dm, dv = Guarded(n, p), Guarded(n, m), Guarded(n, v)
    state = Guarded(2, np.array([t0, 0], dtype=np.int32), dtype=torch.int32)
    for gr in g:
        dg = Guarded(n, gr)
        if ctl is None:
            _lib.check(L.orr_adam_step(dp.ptr, dg.ptr, dm.ptr, dv.ptr, n, *HYPER, gscale, flags, state.ptr, stream()), L)
        else:
            _lib.check(L.orr_adam_step_ctl(dp.ptr, dg.ptr, dm.ptr, dv.ptr, n, *HYPER, gscale, flags, state.ptr, ctl.data_ptr(), stream()), L)
        assert intact(dg)
    assert intact(dp, dm, dv, state)                                   # nothing at or beyond n changes
    return dp.np(), dm.np(), dv.np(), state.np().tolist()


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_step_at_workgroup_edges_and_large_step_counts(n, flags):
    from tests import test_gpu_update_control as uc
    uc.lib()
    dev = ctx()[3]
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for t0 in R.ADAM_T0:
        for gscale in (1.0, 0.25):
            p, m, v, g = R.adam_data(n)
            if t0 == 0:
                m, v = np.zeros_like(m), np.zeros_like(v)
            p64, m64, v64, bm, bv = R.adam_ref(p, g, m, v, t0, *HYPER, gscale, flags)
            bp = R.long_bound(R.adam_restate(p, g, m, v, t0, *HYPER, gscale, flags)[0], p64, "adam.p")
            got = run_adam(n, p, g, m, v, t0, gscale, flags)
            assert got[3] == [t0 + 3, 0], (t0, got[3])
            for k, x, ref, b in (("p", got[0], p64, bp), ("m", got[1], m64, bm), ("v", got[2], v64, bv)):
                worst[k] = max(worst[k], R.ratio_of(x, ref, b))
            # the control record: neutral gives orr_adam_step's bits; a skip word leaves everything where it was
            neutral = run_adam(n, p, g, m, v, t0, gscale, flags, ctl=uc.new_ctl(dev))
            assert all(np.array_equal(R.bits(a), R.bits(b)) for a, b in zip(got[:3], neutral[:3])) and neutral[3] == got[3]
            for word in (1, 2, 3):
                skipped = run_adam(n, p, g, m, v, t0, gscale, flags, ctl=uc.new_ctl(dev, skip=word))
                assert all(np.array_equal(R.bits(a), R.bits(b)) for a, b in zip(skipped[:3], (p, m, v))) and skipped[3] == [t0, 0]
    for k in worst:
        assert report("adam.%s.%s" % ("mpi" if flags else "torch", k), worst[k]) <= 1.0, (k, n)


# ---- orr_update_control's gradient norm ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_update_control_norm_at_partial_edges(n):
    """n = 65537: 65 partials, so a lane of the second launch adds two.  The buffer ends at n: a read beyond it meets the guard's NaN."""
    from tests import test_gpu_update_control as uc
    _lib, L, dev = uc.lib()
    g = R.mixed(np.random.RandomState(n), n)
    dg = Guarded(n, g)
    P = int(L.orr_update_control_partials(n))
    assert P == (n + 1023) // 1024
    partials, ctl = Guarded(P), uc.new_ctl(dev)
    c = uc.control(_lib, L, dev, dg.t, n, partials.t, ctl)
    assert intact(dg, partials)
    s64 = float((np.asarray(g, F64) ** 2).sum())
    s32 = float(uc.fold_like_the_kernel(partials.np()))
    within("update_control.sumsq", s32, s64, R.sumsq_bound(n) * s64)                        # the bound csrc/orr_learner.hip states
    within("update_control.grad_norm", c["grad_norm"], np.sqrt(s64), (0.5 * R.sumsq_bound(n) + 2 * R.U) * np.sqrt(s64))
    assert c["skip"] == 0 and c["grad_scale"] == 1.0 and c["n_calls"] == 1
    partials2, ctl2 = Guarded(P), uc.new_ctl(dev)
    uc.control(_lib, L, dev, dg.t, n, partials2.t, ctl2)
    assert np.array_equal(R.bits(partials.np()), R.bits(partials2.np())) and bool((ctl == ctl2).all())


# ---- orr_gae_flags ---------------------------------------------------------------------------------------------------------------------------

def run_gae(r, v, d, first, boot, flags, eps):
    torch, _lib, L, dev = ctx()
    T, N = r.shape
    dr, dv, adv, ret = Guarded(T * N, r), Guarded(T * N, v), Guarded(T * N), Guarded(T * N)
    dd = torch.from_numpy(d.astype(np.uint8)).to(dev)
    df = None if first is None else torch.from_numpy(first.astype(np.uint8)).to(dev)
    db = None if boot is None else Guarded(N, boot)
    _lib.check(L.orr_gae_flags(dr.ptr, dv.ptr, dd.data_ptr(), None if df is None else df.data_ptr(), None if db is None else db.ptr, T, N, 0.95, 0.95,
                               flags, eps, adv.ptr, ret.ptr, stream()), L)
    assert intact(dr, dv, adv, ret)
    return adv.np(T, N), ret.np(T, N)


@pytest.mark.parametrize("T,N", R.GAE_SHAPES)
def test_gae_flags_over_robot_counts_and_the_legacy_index(T, N):
    torch = ctx()[0]
    from openroborl_amd import rollout
    worst = {"adv": 0.0, "ret": 0.0, "normalized": 0.0}
    gamma = lam = float(F32(0.95))
    for rate in R.GAE_RATES:
        r, v, d, fs, boot = R.gae_data(T, N, rate)
        for legacy in (False, True):
            for first in (None, fs, np.zeros(N, dtype=bool)):
                for b in (None, boot):
                    a64, r64 = rollout.gae(torch.from_numpy(r).double(), torch.from_numpy(v).double(), torch.from_numpy(d), gamma, lam,
                                           None if b is None else torch.from_numpy(b).double(), legacy, None if first is None else torch.from_numpy(first))
                    (_, b_adv), (_, b_ret) = R.gae_ref(r, v, d, 0.95, 0.95, b, legacy, first)
                    adv, ret = run_gae(r, v, d, first, b, 2 if legacy else 0, 0.0)
                    worst["adv"] = max(worst["adv"], R.ratio_of(adv, a64.numpy(), b_adv))
                    worst["ret"] = max(worst["ret"], R.ratio_of(ret, r64.numpy(), b_ret))
                    if T == 1:
                        continue
                    want = rollout.normalize_per_robot(a64, eps=float(F32(1e-8))).numpy()
                    keep = a64.numpy().var(axis=0) >= R.MIN_VAR
                    assert keep.all() or rate == 1.0
                    if not keep.any():
                        continue
                    restated = R.gae_run(r, v, d, 0.95, 0.95, b, legacy, first, True, 1e-8, F32)[0]
                    nrm, ret_n = run_gae(r, v, d, first, b, 1 | (2 if legacy else 0), 1e-8)
                    assert np.array_equal(R.bits(ret_n), R.bits(ret))
                    worst["normalized"] = max(worst["normalized"], R.ratio_of(nrm[:, keep], want[:, keep],
                                                                            R.long_bound(restated[:, keep], want[:, keep], "gae.normalized")))
    for k in worst:
        assert report("gae.%s" % k, worst[k]) <= 1.0, (k, T, N)
