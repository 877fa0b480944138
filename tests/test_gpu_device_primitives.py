"""The env kernels' device primitives, one by one, on the GPU (through the test-only probe, tests/probe_lib.py).

The leaf helpers of csrc/orr_device.h / orr_physics.h / orr_task.h are each called from a small kernel of their own and compared with a
plain definition (tests/primitive_refs.py): lane movement exactly against float32 numpy (row_sum16, bcast_lane, pick4, zero_in_lane,
dpp_bcast_max0, the part_suffix_sum family, dpp_contact_triplet), the branch-free math against float64 of the float32 inputs
(joint_sincos, atan2_bf, asin_bf, map_pi, euler_from_quat, qheading, q_norm_angle, q_to_mat, qrot, qslerp), the Cholesky (chol6, chol6_pk)
by its backward error, the RNG and the step limit (philox_block, time_limit) exactly against the oracle.
Elsewhere: normal_pair in tests/test_gpu_init_noise.py; the solver stages built from these leaves (delassus_columns, pgs_sweeps) in
tests/test_gpu_solver_primitives.py.  Not probed at all: row_setup_*, row_response and leg_dynamics work on the per-robot LDS image, not
on register operands; they stay with the sub-step parity tests (tests/test_gpu_parity.py, tests/test_gpu_substep_paths.py).
Both probe builds are tested: `one` has the flags of the one-wave env unit, `w2` those of the two-wave unit (-Os, other scheduler).
Each test prints `PRIMITIVE <name> <build> max_err=... bound=... n=...` (profiles/device_primitives.txt keeps the lines of one run).

Bounds: absolute ones are derived (the helper's documented error + the 1-ulp hardware rcp / rsq / sqrt on its path); where the
conditioning rules an absolute bound out (gimbal lock, w = +-1) the bound is relative to the FLOOR, the same formula in numpy float32
on the same inputs, per bucket: max error <= 2 x floor max error + 4.2e-7.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from openroborl_amd import _abi
from tests import primitive_refs as R
from tests import probe_lib

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS24 = 2.0 ** -24
ATAN2_BOUND = 4.2e-7     # the documented 3e-7 + one ulp of v_rcp_f32 on t <= 1, twice in the (t - 1) / (t + 1) branch
FLOOR_FACTOR, FLOOR_SLACK = 2.0, 4.2e-7
N_WAVE = 64 * 64         # 64 blocks of one wave: 256 robots


@pytest.fixture(scope="module", params=["one", "w2"])
def build(request):
    probe_lib.lib(request.param)
    return request.param


def report(name, build, err, bound, n):
    print("PRIMITIVE %s %s max_err=%.3e bound=%.3e n=%d" % (name, build, err, bound, n))


def same_value(a, b):
    """a == b elementwise (+0 == -0), NaNs never equal"""
    return np.asarray(a) == np.asarray(b)


cached = functools.lru_cache(maxsize=None)


# =====================================================================================================================
# A. lane movement
# =====================================================================================================================
def test_row_sum16(build):
    x = R.wave_inputs(N_WAVE, 1, 1, "int")[:, 0]
    got = probe_lib.run(build, "row_sum16", x)
    want, _ = R.row_sum_ref64(x)
    assert np.array_equal(got.astype(np.float64), want)
    x = R.wave_inputs(N_WAVE, 1, 2)[:, 0]
    got = probe_lib.run(build, "row_sum16", x)
    g = got.reshape(-1, 16).view(np.uint32)
    assert (g == g[:, :1]).all(), "the butterfly is symmetric: one bit pattern in all 16 lanes"
    want, mag = R.row_sum_ref64(x)
    rel = np.abs(got - want) / mag
    report("row_sum16", build, rel.max(), 4 * EPS24, len(x))
    assert rel.max() <= 4 * EPS24        # four rounding levels


def test_bcast_lane_pick4_zero_in_lane(build):
    x = R.wave_inputs(N_WAVE, 1, 3)[:, 0]
    got = probe_lib.run(build, "bcast_lane", x)
    assert np.array_equal(got.view(np.uint32), R.bcast_ref(x, range(16)).view(np.uint32))
    report("bcast_lane", build, 0.0, 0.0, got.size)
    got = probe_lib.run(build, "zero_in_lane", x)
    want = np.repeat(x[:, None], 16, axis=1)
    want[np.arange(len(x)), np.arange(len(x)) & 15] = 0.0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    report("zero_in_lane", build, 0.0, 0.0, got.size)
    x4 = R.wave_inputs(1000, 4, 4)      # no multiple of the block: the last one is partial
    got = probe_lib.run(build, "pick4", x4)
    assert np.array_equal(got.view(np.uint32), x4[np.arange(1000), np.arange(1000) & 3].view(np.uint32))
    report("pick4", build, 0.0, 0.0, got.size)


def test_dpp_bcast_max0(build):
    x = R.wave_inputs(N_WAVE, 1, 5)[:, 0]
    x[::7] = 0.0
    x[3::11] = -0.0
    got = probe_lib.run(build, "dpp_bcast_max0", x)
    want = np.maximum(R.bcast_ref(x, range(4, 16)), F32(0))
    assert same_value(got, want).all()           # max(-0, 0) may be either zero
    assert (x > 0).sum() > 1000 and (x < 0).sum() > 1000 and (x == 0).sum() > 500
    report("dpp_bcast_max0", build, 0.0, 0.0, got.size)


def test_part_suffix_sums(build):
    x = R.wave_inputs(N_WAVE, 6, 6)
    x[5::9] = -0.0
    want = R.suffix_sum_ref(x)
    got = probe_lib.run(build, "part_suffix_sum_inplace", x)          # all six values of the block in one call
    assert same_value(got, want).all()                                # bit-exact up to the documented sign of zero
    nz = want != 0
    assert np.array_equal(got.view(np.uint32)[nz], want.view(np.uint32)[nz])
    got1 = probe_lib.run(build, "part_suffix_sum", x[:, 0].copy())
    assert same_value(got1, want[:, 0]).all() and np.array_equal(got1.view(np.uint32)[nz[:, 0]], want[:, 0].view(np.uint32)[nz[:, 0]])
    # part 3 is never a source: NaN in every part-3 lane stays there
    part = (np.arange(N_WAVE) >> 2) & 3
    xn = x.copy()
    xn[part == 3] = np.nan
    for name, arg in (("part_suffix_sum_inplace", xn), ("part_suffix_sum", xn[:, 0].copy())):
        got = probe_lib.run(build, name, arg).reshape(N_WAVE, -1)
        assert np.isfinite(got[part < 3]).all(), name
        assert same_value(got[part < 3], want[part < 3][:, :got.shape[1]]).all(), name
        assert np.isnan(got[part == 3]).all(), name
    report("part_suffix_sum", build, 0.0, 0.0, got1.size)
    report("part_suffix_sum_inplace", build, 0.0, 0.0, want.size)


@pytest.mark.parametrize("with_m", [False, True])
def test_part_suffix_sum_first_moment(build, with_m):
    name = "part_suffix_sum_first_moment_m%d" % with_m
    part = (np.arange(N_WAVE) >> 2) & 3
    # dyadic inputs: every product and sum is exact in float32, so the result is the float64 one
    rec = R.first_moment_inputs(N_WAVE, 7, "dyadic")
    got = probe_lib.run(build, name, rec)
    want, _ = R.first_moment_ref64(rec)
    assert np.array_equal(got[:, :3].astype(np.float64), want)
    mass = R.suffix_sum_ref(rec[:, 0]) if with_m else rec[:, 0]
    assert np.array_equal(got[:, 3].view(np.uint32), mass.view(np.uint32))
    # random inputs: two roundings, each at most half an ulp of a partial sum
    rec = R.first_moment_inputs(N_WAVE, 8, "random")
    got = probe_lib.run(build, name, rec)
    want, scale = R.first_moment_ref64(rec)
    ulps = np.abs(got[:, :3] - want) / np.spacing(scale.astype(F32)).astype(np.float64)
    report(name, build, ulps.max(), 1.0, want.size)
    assert ulps.max() <= 1.0
    mass = R.suffix_sum_ref(rec[:, 0]) if with_m else rec[:, 0]
    assert np.array_equal(got[:, 3].view(np.uint32), mass.view(np.uint32))
    # NaN in the part-3 lanes reaches no link lane
    recn = rec.copy()
    recn[part == 3] = np.nan
    got = probe_lib.run(build, name, recn)
    assert np.isfinite(got[part < 3]).all()


def test_dpp_contact_triplet(build):
    rec = R.wave_inputs(N_WAVE, 21, 9, "dyadic")     # products of two and sums of six are exact
    got = probe_lib.run(build, "dpp_contact_triplet", rec)
    want, _ = R.triplet_ref64(rec)
    assert np.array_equal(got.astype(np.float64), want)
    rec = R.wave_inputs(N_WAVE, 21, 10)
    got = probe_lib.run(build, "dpp_contact_triplet", rec)
    want, mag = R.triplet_ref64(rec)
    rel = np.abs(got - want) / mag
    report("dpp_contact_triplet", build, rel.max(), 8 * EPS24, want.size)
    assert rel.max() <= 8 * EPS24          # seven chained operations


# =====================================================================================================================
# B. math
# =====================================================================================================================
gen_sincos, gen_atan2, gen_map_pi = cached(R.gen_sincos), cached(R.gen_atan2), cached(R.gen_map_pi)
gen_asin, gen_euler, gen_heading, gen_norm_angle = cached(R.gen_asin), cached(R.gen_euler), cached(R.gen_heading), cached(R.gen_norm_angle)
gen_quat_points, gen_slerp, gen_chol = cached(R.gen_quat_points), cached(R.gen_slerp), cached(R.gen_chol)


def test_joint_sincos(build):
    a = gen_sincos()
    got = probe_lib.run(build, "joint_sincos", a)
    a64 = a.astype(np.float64)
    err = np.maximum(np.abs(got[:, 0] - np.sin(a64)), np.abs(got[:, 1] - np.cos(a64)))
    report("joint_sincos", build, err.max(), 1e-7, len(a))
    assert err.max() <= 1e-7, a[np.argmax(err)]


def test_atan2_bf(build):
    x, buckets = gen_atan2()
    got = probe_lib.run(build, "atan2_bf", x)
    err = np.abs(got - np.arctan2(x[:, 0].astype(np.float64), x[:, 1].astype(np.float64)))
    for name, m in buckets.items():
        report("atan2_bf[%s]" % name, build, err[m].max(), ATAN2_BOUND, int(m.sum()))
    report("atan2_bf", build, err.max(), ATAN2_BOUND, len(x))
    assert np.isfinite(got).all()
    assert err.max() <= ATAN2_BOUND, x[np.argmax(err)]


def test_atan2_bf_signed_zeros(build):
    pairs = np.array([p for p, _ in R.ATAN2_EXACT] + [(-0.0, 0.0)] * (128 - len(R.ATAN2_EXACT)), dtype=F32)
    got = probe_lib.run(build, "atan2_bf", pairs)
    for (p, want), g in zip(R.ATAN2_EXACT, got):
        assert g == F32(want), (p, g)
    assert got[3] == 0 and np.signbit(got[3])       # (-0.0, 0): a negative-signed result
    report("atan2_bf[signed zeros]", build, 0.0, 0.0, 4)


def test_atan2_bf_subnormal_arguments(build):
    """Nothing non-finite may leave atan2_bf, subnormal arguments included (v_rcp_f32 of a subnormal is +inf): the result is within the
    bound of float64 atan2 taken with the subnormals either kept or flushed to zero."""
    base = np.array(R.ATAN2_SUBNORMAL, dtype=F32)
    pairs = np.concatenate([base * F32(sy) * np.array([1, sx], dtype=F32) for sy in (1, -1) for sx in (1, -1)])
    pairs = np.concatenate([pairs, np.tile(pairs[:1], (128 - len(pairs) % 128, 1))])
    assert (np.abs(pairs[pairs != 0]) < np.finfo(F32).tiny).sum() >= 40
    got = probe_lib.run(build, "atan2_bf", pairs)
    kept = np.arctan2(pairs[:, 0].astype(np.float64), pairs[:, 1].astype(np.float64))
    fl = R.flush_subnormals(pairs).astype(np.float64)
    flushed = np.arctan2(fl[:, 0], fl[:, 1])
    err = np.minimum(np.abs(got - kept), np.abs(got - flushed))
    bad = ~np.isfinite(got)
    report("atan2_bf[subnormal]", build, np.inf if bad.any() else err.max(), ATAN2_BOUND, len(pairs))
    assert not bad.any(), pairs[bad][:8]
    assert err.max() <= ATAN2_BOUND, pairs[np.argmax(err)]


def test_map_pi(build):
    a = gen_map_pi()
    got = probe_lib.run(build, "map_pi", a)
    assert (np.abs(got) <= R.PI_F).all()
    # the source comment: "exact (k = 0) for |a| < 2 pi" -- the result is a itself, or a -+ 2 pi_f in float32
    small = np.abs(a) < F32(2 * np.pi)
    two_pi = F32(2) * R.PI_F
    exact = np.where(a >= R.PI_F, a - two_pi, np.where(a < -R.PI_F, a + two_pi, a)).astype(F32)
    assert small.sum() > 50000 and np.array_equal(got[small], exact[small])
    a64 = a.astype(np.float64)
    over = R.circ(got, R.map_pi_def(a64)) - np.spacing(np.abs(a)).astype(np.float64)
    report("map_pi", build, over.max(), 2.4e-7, len(a))       # the error beyond one ulp of |a|
    assert over.max() <= 2.4e-7, a[np.argmax(over)]


def floor_check(name, build, got, ref64, floor32, buckets, angle=True):
    """per bucket: HIP max error <= 2 x (max error of the same formula in float32) + 4.2e-7; returns the worst margin"""
    dist = R.circ if angle else (lambda a, b: np.abs(np.asarray(a, dtype=np.float64) - b))
    e_dev = dist(got, ref64).reshape(len(got), -1).max(axis=1)
    e_f32 = dist(floor32, ref64).reshape(len(got), -1).max(axis=1)
    assert np.isfinite(got).all()
    covered = np.zeros(len(got), dtype=bool)
    fails = []
    for bname, m in buckets.items():
        assert m.sum() >= R.MIN_BUCKET, (bname, int(m.sum()))
        covered |= m
        bound = FLOOR_FACTOR * e_f32[m].max() + FLOOR_SLACK
        report("%s[%s]" % (name, bname), build, e_dev[m].max(), bound, int(m.sum()))
        if not e_dev[m].max() <= bound:
            fails.append((bname, e_dev[m].max(), bound))
    assert covered.all(), "no input is dropped"
    assert not fails, fails


def test_asin_bf(build):
    x, buckets = gen_asin()
    got = probe_lib.run(build, "asin_bf", x)
    floor_check("asin_bf", build, got, np.arcsin(x.astype(np.float64)), np.arcsin(x), buckets)


def test_euler_from_quat(build):
    q, buckets = gen_euler()
    got = probe_lib.run(build, "euler_from_quat", q)
    floor_check("euler_from_quat", build, got, R.euler_def(q), R.euler_def(q, F32), buckets)
    # at the clamped ends the pitch is +-pi/2 itself
    m = buckets["clamped"]
    s = R.euler_sarg64(q[m])
    assert R.circ(got[m, 1], np.sign(s) * np.pi / 2).max() <= 2 * 4.4e-4     # float32 may see |sarg| just below 1: acos-like floor sqrt(2 x 1e-7)


def test_qheading(build):
    q, buckets = gen_heading()
    got = probe_lib.run(build, "qheading", q)
    floor_check("qheading", build, got, R.heading_def(q), R.heading_def(q, F32), buckets)


def test_q_norm_angle(build):
    q, buckets = gen_norm_angle()
    got = probe_lib.run(build, "q_norm_angle", q)
    floor_check("q_norm_angle", build, got, R.norm_angle_def(q), R.norm_angle_def(q, F32), buckets)


def test_q_to_mat_and_qrot(build):
    p, q, buckets = gen_quat_points()
    got = probe_lib.run(build, "q_to_mat", q)
    floor_check("q_to_mat", build, got, R.q_to_mat_def(q), R.q_to_mat_def(q, F32), buckets, angle=False)
    got = probe_lib.run(build, "qrot", np.concatenate([p, q], axis=1))
    floor_check("qrot", build, got, R.qrot_def(p, q), R.qrot_def(p, q, F32), buckets, angle=False)


SLERP_BOUND = 7.5e-7     # the float32 transliteration's 3.75e-7 + 3.6e-7 for the 1-ulp v_rsq (twice), v_rcp and v_sqrt on the path


def test_qslerp(build):
    x, buckets, dropped = gen_slerp()
    got = probe_lib.run(build, "qslerp", x)
    want, _ = R.slerp_def(x[:, 0:4], x[:, 4:8], x[:, 8])
    assert np.isfinite(got).all()
    err = np.abs(got - want).max(axis=1)
    fails = []
    for name, m in buckets.items():
        assert m.sum() >= R.MIN_BUCKET and (m & dropped).sum() < 0.01 * m.sum()
        e = err[m & ~dropped].max()
        report("qslerp[%s]" % name, build, e, SLERP_BOUND, int((m & ~dropped).sum()))
        if not e <= SLERP_BOUND:
            fails.append((name, e))
    assert not fails, fails
    # f = 0 and f = 1 give the normalised ends themselves
    for name, end in (("f=0", x[:, 0:4]), ("f=1", x[:, 4:8])):
        m = buckets[name]
        e64 = end[m].astype(np.float64)
        assert np.abs(got[m] - e64 / np.sqrt((e64 * e64).sum(axis=1, keepdims=True))).max() <= 2.5e-7    # 1 ulp of rsq + 1 of the product, at <= 1


# =====================================================================================================================
# C. Cholesky
# =====================================================================================================================
CHOL_BOUND = 32 * EPS24    # Higham's gamma_{3n+1}, n = 6: 19 units; six 1-ulp rsq pivots, each used twice, add the rest


def test_chol6_and_chol6_pk(build):
    rec, buckets = gen_chol()
    out = {}
    for name in ("chol6", "chol6_pk"):
        got = out[name] = probe_lib.run(build, name, rec)
        x, idg = got[:, :6], got[:, 6:]
        assert np.isfinite(got).all() and (idg > 0).all(), name
        be = R.chol_backward_error(rec, x)
        for bname, m in buckets.items():
            assert m.sum() >= R.MIN_BUCKET
            report("%s[%s]" % (name, bname), build, be[m].max(), CHOL_BOUND, int(m.sum()))
        assert be.max() <= CHOL_BOUND, name
    same = out["chol6"].view(np.uint32) == out["chol6_pk"].view(np.uint32)
    # do the two forms agree bit for bit?  Printed, not asserted (the source comment's claim, no contract); the line is
    # in profiles/device_primitives.txt with the others
    print("PRIMITIVE chol6_vs_chol6_pk %s bitwise_equal=%s differing_values=%d of %d max_diff=%.3e" % (
        build, same.all(), (~same).sum(), same.size, np.abs(out["chol6"] - out["chol6_pk"]).max()))


# =====================================================================================================================
# D. RNG and step limit
# =====================================================================================================================
@cached
def philox_reference():
    from tests import oracle_lib as ol
    L = ol.lib()
    s, r, e, b = R.gen_philox()
    want = np.empty((len(s), 4))
    for i in range(len(s)):
        for k in range(4):
            want[i, k] = L.orc_uniform(int(s[i]), int(r[i]), int(e[i]), 4 * int(b[i]) + k)
    return (s, r, e, b), want


def test_philox_block_matches_the_oracle(build):
    (s, r, e, b), want = philox_reference()
    got = probe_lib.run_philox(build, s, r, e, b)
    gi, wi = np.round(got.astype(np.float64) * 2 ** 24).astype(np.int64), np.round(want * 2 ** 24).astype(np.int64)
    assert np.array_equal(got.astype(np.float64), want) and np.array_equal(gi, wi)        # as 24-bit values
    assert len(np.unique(wi)) > 0.98 * wi.size       # the streams differ (75 k draws of 24 bits: a few hundred birthday collisions)
    report("philox_block", build, 0.0, 0.0, got.size)


@cached
def time_limit_reference():
    from tests import oracle_lib as ol
    L = ol.lib()
    cases = []
    for cur, steps, start, end in R.TIME_LIMIT_CONFIGS:
        cfg = _abi.OrrConfig()
        cfg.flags = _abi.FLAG_CURRICULUM if cur else 0
        cfg.curriculum_steps, cfg.ep_len_start, cfg.ep_len_end = steps, start, end
        tot = R.gen_time_limit_totals(steps, start, end)
        want = np.array([L.orc_time_limit(C.byref(cfg), int(t)) for t in tot], dtype=np.int32)
        cases.append((cfg, tot, want))
    return cases


def test_time_limit_matches_the_oracle(build):
    n = 0
    for cfg, tot, want in time_limit_reference():
        assert tot.max() >= 2 ** 40
        got = probe_lib.run_time_limit(build, cfg, tot)
        bad = got != want
        assert not bad.any(), (cfg.curriculum_steps, cfg.ep_len_start, cfg.ep_len_end, tot[bad][:5], got[bad][:5], want[bad][:5])
        n += len(tot)
    report("time_limit", build, 0.0, 0.0, n)
