"""The comparisons of tests/learner_refs.py can fail: on the CPU, the float32 restatement of every learner kernel passes its bound at the
smallest shapes of the GPU grid (tests/test_gpu_learner_edges.py), and the same restatement with ONE seeded defect is rejected at a shape
of that grid.  Nothing here, and nothing on the device, runs a kernel with a defect in it.  The two exclusion caps of the GPU tests
(samples near a clip edge, robots of low variance) are asserted here on the float64 reference alone."""
import numpy as np
import pytest

from tests import learner_refs as R

F32, F64 = R.F32, R.F64
STD, CLIP, VF = 0.125, 0.2, 0.5


def ok(got, ref, bound):
    return R.ratio_of(got, ref, bound) <= 1.0


# ---- orr_colsum_finish ----------------------------------------------------------------------------------------------------------------------

def _colsum_case(rows, cols):
    return R.mixed(np.random.RandomState(rows * 1000 + cols), rows, cols)


@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_restatement_passes_over_the_grid(rows):
    for cols in R.COLSUM_COLS:
        p = _colsum_case(rows, cols)
        assert ok(R.colsum_restate(p), *R.colsum_ref(p)), (rows, cols)


@pytest.mark.parametrize("rows", [49, 65])
def test_colsum_rejects_a_row_skipped_behind_the_unrolled_body(rows):
    for cols in (1, 17, 257):
        p = _colsum_case(rows, cols)
        assert not ok(R.colsum_restate(p, "tail_skip"), *R.colsum_ref(p)), (rows, cols)


def test_colsum_rejects_the_path_switch_at_15():
    """16 rows: the host sizes the grid for a thread per column, a kernel that switched at 15 would take 16 columns per workgroup"""
    for cols in (17, 255, 257):
        p = _colsum_case(16, cols)
        assert not ok(R.colsum_restate(p, "switch15"), *R.colsum_ref(p)), cols
    p = _colsum_case(15, 257)                # below the switch the two agree: the defect is caught AT 16
    assert ok(R.colsum_restate(p, "switch15"), *R.colsum_ref(p))


# ---- orr_relu_backward, orr_head_backward --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.RELU_COLS)
def test_relu_backward_restatement_passes_and_rejects(c):
    assert R.cols_ok(c)
    for m in (1, 33):
        g, h = R.relu_data(m, c)
        out, gb = R.relu_backward_restate(g, h)
        assert np.array_equal(R.bits(out), R.bits(R.relu_select(g, h)))
        assert ok(gb, *R.relu_backward_ref(g, h)), (m, c)
    g, h = R.relu_data(33, c)
    assert (h == 0).any() and (h > 0).any()
    for defect in ("last_row", "mask_ge"):
        out, gb = R.relu_backward_restate(g, h, defect=defect)
        assert not np.array_equal(R.bits(out), R.bits(R.relu_select(g, h))), defect
        assert not ok(gb, *R.relu_backward_ref(g, h)), defect


def test_relu_mask_treats_signed_zeros_and_denormals_as_h_gt_0_says():
    h = f = np.array([[0.0, -0.0, 1e-45, -1e-45], [1e-39, -1e-39, 1.0, -1.0]], dtype=F32)
    g = np.array([[np.nan, np.inf, 2.0, -np.inf], [3.0, np.nan, 4.0, np.nan]], dtype=F32)
    want = np.array([[0.0, 0.0, 2.0, 0.0], [3.0, 0.0, 4.0, 0.0]], dtype=F32)
    out, gb = R.relu_backward_restate(g, h)
    assert np.array_equal(R.bits(out), R.bits(want)) and np.array_equal(R.bits(R.relu_select(g, f)), R.bits(want))
    assert ok(gb, *R.relu_backward_ref(g, h)) and np.array_equal(gb, [3.0, 0.0, 6.0, 0.0])
    out, _ = R.relu_backward_restate(g, h, defect="mask_ge")
    assert not np.isfinite(out).all()


@pytest.mark.parametrize("k", R.HEADB_K)
@pytest.mark.parametrize("c", [4, 16, 64])
def test_head_backward_restatement_passes_and_rejects(c, k):
    for m in (1, 33):
        gy, w, h = R.head_backward_data(m, c, k)
        ref = R.head_backward_ref(gy, w, h)
        for name, x in zip(("gz", "gb", "gw"), R.relu_backward_restate(None, h, gy, w)):
            assert ok(x, *ref[name]), (name, m, c, k)
    for defect in ("last_row", "mask_ge"):
        got = dict(zip(("gz", "gb", "gw"), R.relu_backward_restate(None, h, gy, w, defect=defect)))
        assert not ok(got["gz"], *ref["gz"]) and not ok(got["gb"], *ref["gb"]), defect
    assert not ok(R.relu_backward_restate(None, h, gy, w, defect="last_row")[2], *ref["gw"])
    swapped = R.relu_backward_restate(None, h, gy, w, defect="wpart_swap")[2]
    assert ok(swapped, *ref["gw"]) == (k == 1)          # (e / 1, e % 1) swapped addresses the same word: the defect is caught at K = 12


# ---- the loss heads -----------------------------------------------------------------------------------------------------------------------------

def _head(m, log_std=None, spread=False, defect=None, data=None, clip=CLIP, ent=0.01):
    mean, value, batch = data or R.head_data(m, STD, log_std, spread)
    ref = R.ppo_head_ref(mean, value, batch, STD, clip, VF, log_std, ent)
    clean = R.ppo_head_restate(mean, value, batch, STD, clip, VF, log_std, ent)
    got = clean if defect is None else R.ppo_head_restate(mean, value, batch, STD, clip, VF, log_std, ent, defect)
    return ref, clean, got, R.ppo_head_bounds(ref, clean, VF)


@pytest.mark.parametrize("logstd", [False, True])
@pytest.mark.parametrize("m", [1, 255, 257, 769])
def test_ppo_head_restatement_passes(m, logstd):
    for spread in (False, True):
        ref, clean, got, B = _head(m, R.uneven_log_std() if logstd else None, spread)
        for k in B:
            assert ok(got[k], ref[k], B[k]), (k, m, spread)
        # the caps the GPU test relies on, on the reference alone: at most 1 % of the samples within the ratio's bound of a clip edge,
        # samples on both sides of the range, exactly-zero gradients present
        near = R.near_clip_edge(ref, clean, CLIP)
        assert near.mean() <= 0.01, (m, spread, near.sum())
        if m > 1:
            assert ref["dead"].any() and not ref["dead"].all() and ref["inside"].any() and not ref["inside"].all()
        keep = ref["dead"] & ~near
        assert not (R.bits(got["g_mean"][keep]) & 0x7fffffff).any()
        if logstd:
            assert got["clipfrac"] == F32(ref["clipfrac"]) or near.any()


@pytest.mark.parametrize("logstd", [False, True])
def test_ppo_head_rejects_a_dropped_row_and_a_dropped_row_group(logstd):
    ls = R.uneven_log_std() if logstd else None
    for m in (257, 769):
        ref, _, got, B = _head(m, ls, defect="last_row")
        assert not ok(got["g_mean"], ref["g_mean"], B["g_mean"]) and not ok(got["g_value"], ref["g_value"], B["g_value"])
        assert not ok(got["gb_value"], ref["gb_value"], B["gb_value"]) and not ok(got["vloss"], ref["vloss"], B["vloss"])
    for m in (769, 1025):       # four and five workgroups: the fourth row group holds one
        ref, _, got, B = _head(m, ls, defect="three_groups")
        for k in ("gb_mean", "gb_value", "surr", "vloss") + (("g_logstd", "kl") if logstd else ()):
            assert not ok(got[k], ref[k], B[k]), (k, m)
    ref, _, got, B = _head(255, ls, defect="three_groups")          # one workgroup: nothing in the dropped group
    assert all(ok(got[k], ref[k], B[k]) for k in B)


@pytest.mark.parametrize("logstd", [False, True])
def test_the_tie_case_pins_the_clip_rule(logstd):
    ls = R.uneven_log_std() if logstd else None
    m = 257
    log_norm = R.log_norm_of(ls) if logstd else R.ppo_head_scalars(m, STD)["log_norm"]
    data = R.tie_data(m, log_norm)
    ref, clean, got, B = _head(m, ls, data=data, clip=0.0)
    tie = np.arange(m) % 5 != 0
    assert (clean["ratio"][tie] == 1.0).all() and (ref["ratio"][tie] == 1.0).all() and (np.abs(ref["ratio"][~tie] - 1.0) > 0.5).all()
    A = data[2][:, 13]
    assert (A[tie] > 0).any() and (A[tie] < 0).any() and (A[tie] == 0).any() and (A[~tie] == 0).any()
    # on a tie both branches are the same value: the sample passes -A, for either sign
    assert np.array_equal(ref["gl"][tie] == 0.0, A[tie] == 0) and abs(ref["surr"] - clean["surr"]) <= B["surr"]
    for k in B:
        assert ok(got[k], ref[k], B[k]), k
    assert not (R.bits(clean["g_mean"]) & 0x7fffffff).any()         # act == mean: every gradient is a zero; its sign is the rule's
    wrong = R.ppo_head_restate(*data, STD, 0.0, VF, ls, 0.01, "clip_le")
    assert not np.array_equal(R.bits(wrong["g_mean"]), R.bits(clean["g_mean"]))
    assert np.array_equal(R.bits(wrong["g_mean"][tie]), R.bits(clean["g_mean"][tie]))       # caught by the zero advantages outside the range


@pytest.mark.parametrize("m", R.SMALL_HEAD_ROWS)
def test_distill_and_regress_heads_pass_and_reject_a_dropped_row(m):
    rng = np.random.RandomState(m)
    mean, target = R.mixed(rng, m, 12), R.mixed(rng, m, 12)
    ref = R.distill_head_ref(mean, target)
    got, bad = R.distill_head_restate(mean, target), R.distill_head_restate(mean, target, "last_row")
    for k in ref:
        assert ok(got[k], *ref[k]), k
        assert not ok(bad[k], *ref[k]), k
    for c in R.REGRESS_COLS:
        pred, target = R.mixed(rng, m, c), R.mixed(rng, m, c)
        ref = R.regress_head_ref(pred, target)
        got, bad = R.regress_head_restate(pred, target), R.regress_head_restate(pred, target, "last_row")
        for k in ref:
            assert ok(got[k], *ref[k]), (k, c)
            assert not ok(bad[k], *ref[k]), (k, c)


def test_head_finish_of_the_distill_head_rejects_three_groups():
    rng = np.random.RandomState(3)
    mean, target = R.mixed(rng, 769, 12), R.mixed(rng, 769, 12)
    ref, bad = R.distill_head_ref(mean, target), R.distill_head_restate(mean, target, "three_groups")
    assert not ok(bad["gb_mean"], *ref["gb_mean"]) and not ok(bad["loss"], *ref["loss"])


@pytest.mark.parametrize("n", [1, 255, 257])
def test_gauss_prepare_restatement_is_close_to_float64(n):
    """the long rule's floor here: the restatement's own error stays at a few units of float32 (so twice it is a tight bound)"""
    rng = np.random.RandomState(n)
    noise, ls = f = F32(rng.standard_normal((n, 12))), R.uneven_log_std()
    scaled, logp = R.gauss_prepare_restate(noise, ls)
    want, want_logp = R.gauss_prepare_ref(noise, ls)
    assert np.abs(scaled / want - 1.0).max() <= 4 * R.U and np.abs(logp - want_logp).max() <= 16 * R.U * np.abs(want_logp).max()


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------------

HYPER = (1e-3, 0.9, 0.999, 1e-5)


def _adam(n, t0, flags, gscale, defect=None):
    p, m, v, g = R.adam_data(n)
    if t0 == 0:
        m, v = np.zeros_like(m), np.zeros_like(v)
    p64, m64, v64, bm, bv = R.adam_ref(p, g, m, v, t0, *HYPER, gscale, flags)
    clean = R.adam_restate(p, g, m, v, t0, *HYPER, gscale, flags)
    got = clean if defect is None else R.adam_restate(p, g, m, v, t0, *HYPER, gscale, flags, defect)
    return got, (p64, m64, v64), (R.long_bound(clean[0], p64, "adam.p"), bm, bv)


@pytest.mark.parametrize("t0", R.ADAM_T0)
@pytest.mark.parametrize("flags", [0, 1])
def test_adam_restatement_passes_and_rejects(flags, t0):
    for n in (1, 5, 257):
        for gscale in (1.0, 0.25):
            got, ref, B = _adam(n, t0, flags, gscale)
            assert all(ok(g, r, b) for g, r, b in zip(got, ref, B)), (n, gscale)
    got, ref, B = _adam(257, t0, flags, 1.0, "t_not_plus_one")
    assert ok(got[0], ref[0], B[0]) == (t0 == 99999)        # at t = 1e5 both bias corrections are 1 either way: caught from t = 0 and 999
    if not flags:
        got, ref, B = _adam(257, t0, flags, 1.0, "mpi_always")
        assert ok(got[0], ref[0], B[0]) == (t0 == 99999)    # the two forms differ through sqrt(1 - b2^t) alone


@pytest.mark.parametrize("n", R.SUMSQ_N)
def test_gradient_norm_restatement_passes_the_bound_the_source_states(n):
    g = R.mixed(np.random.RandomState(n), n)
    g[-1] = 1.5
    s64 = float((np.asarray(g, F64) ** 2).sum())
    assert abs(float(R.sumsq_restate(g)) - s64) <= R.sumsq_bound(n) * s64
    assert abs(float(R.sumsq_restate(g[:-1])) - s64) > R.sumsq_bound(n) * s64      # the last element dropped


# ---- GAE -----------------------------------------------------------------------------------------------------------------------------------------

def _first(kind, fs, N):
    return {"absent": None, "random": fs, "zero": np.zeros(N, dtype=bool)}[kind]


@pytest.mark.parametrize("T,N", R.GAE_SHAPES)
def test_gae_restatement_passes_over_the_grid(T, N):
    import torch
    from openroborl_amd import rollout
    for rate in R.GAE_RATES:
        r, v, d, fs, boot = R.gae_data(T, N, rate)
        for legacy in (False, True):
            for kind in ("absent", "random", "zero"):
                for b in (None, boot):
                    first = _first(kind, fs, N)
                    (adv, b_adv), (ret, b_ret) = R.gae_ref(r, v, d, 0.95, 0.95, b, legacy, first)
                    # the numpy recursion is rollout.gae in float64, given the float32 values of gamma and lambda
                    ta, tr = rollout.gae(torch.from_numpy(r).double(), torch.from_numpy(v).double(), torch.from_numpy(d), float(F32(0.95)),
                                         float(F32(0.95)), None if b is None else torch.from_numpy(b).double(), legacy,
                                         None if first is None else torch.from_numpy(first))
                    assert np.abs(ta.numpy() - adv).max() <= 1e-13 and np.abs(tr.numpy() - ret).max() <= 1e-13
                    a32, r32, _ = R.gae_run(r, v, d, 0.95, 0.95, b, legacy, first, False, 0.0, F32)
                    assert ok(a32, adv, b_adv) and ok(r32, ret, b_ret), (rate, legacy, kind)
                    if T > 1:
                        want, var = R.normalize64(adv, 1e-8)
                        if rate < 1.0:
                            assert (var >= R.MIN_VAR).all(), (T, N, rate, var.min())        # no robot is left out at these rates
                        keep = var >= R.MIN_VAR
                        n32, _, _ = R.gae_run(r, v, d, 0.95, 0.95, b, legacy, first, True, 1e-8, F32)
                        assert np.abs(n32[:, keep] - want[:, keep]).max() <= 64 * R.U * np.abs(want[:, keep]).max() * T


def test_gae_rejects_the_own_flag_under_the_legacy_index_for_more_than_one_robot():
    for T, N in R.GAE_SHAPES:
        r, v, d, fs, boot = R.gae_data(T, N, 0.5)
        (adv, b_adv), _ = R.gae_ref(r, v, d, 0.95, 0.95, boot, True, fs)
        bad, _, _ = R.gae_run(r, v, d, 0.95, 0.95, boot, True, fs, False, 0.0, F32, defect="legacy_own")
        if N == 1 or T == 1:          # one robot: the legacy index IS the robot's own next flag; one step: no recursion
            assert ok(bad, adv, b_adv), (T, N)
        else:
            assert not ok(bad, adv, b_adv), (T, N)


def test_gae_rejects_ignored_first_starts():
    caught = 0
    for T, N in R.GAE_SHAPES:
        r, v, d, fs, boot = R.gae_data(T, N, 0.0)
        zero = np.zeros(N, dtype=bool)
        (adv, b_adv), _ = R.gae_ref(r, v, d, 0.95, 0.95, boot, True, zero)
        bad, _, _ = R.gae_run(r, v, d, 0.95, 0.95, boot, True, zero, False, 0.0, F32, defect="first_ignored")
        reads_first = N > 1 and T > 1          # step 0 reads first_starts[2 n + 1] for 2 n + 1 < N
        assert ok(bad, adv, b_adv) != reads_first, (T, N)
        caught += reads_first
    assert caught >= 5


def test_the_grid_constants_match_the_package():
    from openroborl_amd import ppo
    assert tuple(ppo.LOG_STD_BOUNDS) == tuple(R.LOG_STD_BOUNDS)
    ls = R.uneven_log_std()
    assert ls.min() == F32(R.LOG_STD_BOUNDS[0]) and ls.max() == F32(R.LOG_STD_BOUNDS[1]) and len(set(ls.tolist())) == 12
