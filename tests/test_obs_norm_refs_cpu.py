"""tests/obs_norm_refs.py on the CPU: every comparison the GPU tests apply passes on the float32 restatement of the kernels, and each seeded
defect is rejected by it.  The data carries the three column kinds the moments go wrong on: mean 1000 with std 0.01, a constant, magnitude
1e-4."""
import numpy as np
import pytest

from tests import learner_refs as lr
from tests import obs_norm_refs as onr

D = 160
# three unequal batches whose means differ (a merge that forgets delta, or weighs batches and not rows, shows on every ordinary column)
SIZES, SHIFTS = (700, 65, 2049), (0.0, 1.5, -0.75)


@pytest.fixture(scope="module")
def batches():
    return [onr.columns(n, D, seed=10 + i, shift=s) for i, (n, s) in enumerate(zip(SIZES, SHIFTS))]


@pytest.fixture(scope="module")
def layer():
    rng = np.random.RandomState(3)
    k, n = 208, 64
    w = lr.f32(rng.standard_normal((k, n)) * (2.0 / k) ** 0.5)
    b = lr.f32(0.1 * rng.standard_normal(n))
    mean = lr.f32(rng.uniform(-2.0, 2.0, k))
    rstd = lr.f32(1.0 / (np.exp(rng.uniform(np.log(0.05), np.log(3.0), k)) + 1e-2))
    return w, b, mean, rstd


def test_the_data_has_the_three_column_kinds(batches):
    x = batches[0].astype(np.float64)
    assert abs(x[:, onr.COL_OFFSET].mean() - 1000.0) < 0.01 and 0.005 < x[:, onr.COL_OFFSET].std() < 0.02
    assert np.ptp(x[:, onr.COL_CONST]) == 0.0
    assert 5e-5 < x[:, onr.COL_TINY].std() < 2e-4


@pytest.mark.parametrize("d", [160, 48, 4, 256])
def test_restated_update_passes_on_every_edge_size(d):
    rows, side = onr.block_rows(d), onr.pass_rows(d)
    for n in (1, 7, 8, 9, 63, 64, 65, side - 1, side + 1, rows - 1, rows, rows + 1):
        if n < 1:
            continue
        x = [onr.columns(n, d, seed=n)]
        r = onr.stats_ratios(onr.stats_restate(x), x)
        assert max(r.values()) <= 1.0, (d, n, r)


def test_restated_merge_of_three_batches_passes(batches):
    r = onr.stats_ratios(onr.stats_restate(batches), batches)
    assert max(r.values()) <= 1.0, r
    # a first update on the identity record gives the batch's own moments
    one = onr.stats_restate(batches[:1])
    n, mean, m2 = onr.moments64(batches[0])
    assert one["count"] == n and np.abs(one["mean"] - mean).max() <= lr.long_bound(one["mean"], mean)
    # the constant column: variance exactly 0, rstd exactly 1 / eps
    assert one["var"][onr.COL_CONST] == 0.0 and one["rstd"][onr.COL_CONST] == np.float32(1.0 / np.float64(onr.EPS))


def test_count_is_an_integer_past_2_to_24(batches):
    rec = onr.fresh(D)
    rec["count"] = 2 ** 24 + 1
    out = onr.update_restate(rec, batches[0])            # an odd sum: no float32 holds it
    assert out["count"] == 2 ** 24 + 1 + SIZES[0] and int(np.float32(out["count"])) != out["count"]


@pytest.mark.parametrize("defect,group", [("naive", "var"), ("no_delta", "var"), ("batch_weight", "mean"), ("rstd_inside", "rstd")])
def test_seeded_moment_defects_are_rejected(batches, defect, group):
    r = onr.stats_ratios(onr.stats_restate(batches, defect=defect), batches)
    assert r[group] > 1.0, (defect, r)


def test_naive_moments_fail_on_the_offset_column(batches):
    """E[x^2] - E[x]^2 in float32: the column of mean 1000 and std 0.01 loses its variance altogether"""
    bad, ref = onr.stats_restate(batches[:1], defect="naive"), onr.stats64(batches[:1])
    assert abs(bad["var"][onr.COL_OFFSET] - ref["var"][onr.COL_OFFSET]) > 10.0 * ref["var"][onr.COL_OFFSET]
    good = onr.stats_restate(batches[:1])
    assert abs(good["var"][onr.COL_OFFSET] - ref["var"][onr.COL_OFFSET]) < 1e-4 * ref["var"][onr.COL_OFFSET]


def test_restated_normalize_passes(batches):
    rec = onr.stats_restate(batches)
    x = batches[2]
    ref = onr.normalize64(x, rec["mean"], rec["rstd"])
    assert lr.ratio_of(onr.normalize_restate(x, rec["mean"], rec["rstd"]), ref, onr.normalize_bound(x, rec["mean"], rec["rstd"])) <= 1.0
    # the float64 value rounded once is within it too
    assert lr.ratio_of(lr.f32(ref), ref, onr.normalize_bound(x, rec["mean"], rec["rstd"])) <= 1.0


def test_restated_fold_passes_and_identity_is_exact(layer):
    w, b, mean, rstd = layer
    wf, bf = onr.fold_restate(w, b, mean, rstd)
    w64, b64 = onr.fold64(w, b, mean, rstd)
    assert lr.ratio_of(wf, w64, 2 * lr.U * np.abs(w64)) <= 1.0
    assert lr.ratio_of(bf, b64, onr.fold_bias_bound(w, b, mean, rstd)) <= 1.0
    wi, bi = onr.fold_restate(w, b, np.zeros_like(mean), np.ones_like(rstd))
    assert np.array_equal(lr.bits(wi), lr.bits(w)) and np.array_equal(lr.bits(bi), lr.bits(b))


@pytest.mark.parametrize("defect", ["bias_left", "mean_only"])
def test_seeded_fold_defects_are_rejected(layer, defect):
    w, b, mean, rstd = layer
    _, bf = onr.fold_restate(w, b, mean, rstd, defect=defect)
    _, b64 = onr.fold64(w, b, mean, rstd)
    assert lr.ratio_of(bf, b64, onr.fold_bias_bound(w, b, mean, rstd)) > 1.0


def test_folded_net_equals_the_net_on_normalised_inputs(layer):
    """the identity the fold rests on, in float64, and the carried bound on the float32 restatement of layer 0"""
    rng = np.random.RandomState(5)
    k = 160
    p = {}
    for name, (fi, fo) in (("model/pi_fc0", (k, 512)), ("model/pi_fc1", (512, 256)), ("model/pi", (256, 12))):
        p[name + "/w:0"] = lr.f32(rng.standard_normal((fi, fo)) * (2.0 / fi) ** 0.5)
        p[name + "/b:0"] = lr.f32(0.1 * rng.standard_normal(fo))
    x = onr.columns(17, k, seed=8)
    rec = onr.stats_restate([onr.columns(513, k, seed=9)])
    mean, rstd = rec["mean"], rec["rstd"]
    z0, out = onr.mlp64(p, "pi", onr.normalize64(x, mean, rstd))
    wf, bf = onr.fold64(p["model/pi_fc0/w:0"], p["model/pi_fc0/b:0"], mean, rstd)
    z0f, outf = onr.mlp64(dict(p, **{"model/pi_fc0/w:0": wf, "model/pi_fc0/b:0": bf}), "pi", x.astype(np.float64))
    bound = onr.folded_forward_bound(p, "pi", x, mean, rstd)
    assert bound.shape == out.shape and np.abs(outf - out).max() < 1e-3 * bound.min()      # float64: far inside
    # float32 restatement of the folded layer 0 (a k-ordered fmaf chain from 0, then the bias) against the float64 pre-activation
    wr, br = onr.fold_restate(p["model/pi_fc0/w:0"], p["model/pi_fc0/b:0"], mean, rstd)
    acc = np.zeros((x.shape[0], 512), np.float32)
    for i in range(k):
        acc = lr.fma(x[:, i:i + 1], wr[i][None, :], acc)
    b0 = (k + 3) * lr.U * (np.abs(x.astype(np.float64)) @ np.abs(wf) + np.abs(bf)) + onr.fold_bias_bound(p["model/pi_fc0/w:0"], p["model/pi_fc0/b:0"], mean, rstd)
    assert lr.ratio_of(acc + br, z0, b0) <= 1.0
    # a fold that leaves the bias is nowhere near
    acc_bad = acc + p["model/pi_fc0/b:0"]
    assert lr.ratio_of(acc_bad, z0, b0) > 1.0
