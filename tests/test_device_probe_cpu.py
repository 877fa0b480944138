"""No GPU: the device-primitive probe compiles for gfx950 with both flag sets and the solver-stage probe with its three, the
vectorised references of tests/primitive_refs.py agree with brute-force definitions and with the oracle's own functions, and every
input generator of tests/test_gpu_device_primitives.py and tests/test_gpu_solver_primitives.py fills the buckets it names (none empty,
none below 1000 inputs, no input outside every bucket; the solver's buckets: rows on both sides of every bound)."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import primitive_refs as R
from tests import probe_lib
from tests import probe_solver_lib

F32 = np.float32


# ---- the probe builds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["one", "w2", "solver_one", "solver_w2", "solver_generic"])
def test_probe_compiles_for_gfx950(build):
    """A header change that breaks a probe shows here, on the CPU suite.  Not a forced compile: a library whose hash (probe source +
    _lib.DEPS + flags) still matches is taken as it is, so any change of those files compiles here and nothing else does.
    solver_*: the solver-stage probe (orr_probe_solver.hip) in its three builds, `generic` with -DORR_GENERIC_PGS."""
    if build.startswith("solver_"):
        mod, build, names = probe_solver_lib, build[len("solver_"):], list(probe_solver_lib.SPECS)
        assert ("-DORR_GENERIC_PGS" in mod.compile_command(build, "x")) == (build == "generic")
    else:
        mod, names = probe_lib, list(probe_lib.SPECS) + list(probe_lib.INT_ENTRIES)
    so = mod.build(build)
    assert os.path.exists(so) and not mod.needs_build(build)
    with open(so, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob
    for name in names:
        assert b"orrp_" + name.encode() in blob, name


def test_solver_probe_builds_differ_only_in_their_flags():
    from openroborl_amd import _lib
    B = probe_solver_lib.BUILDS
    assert B["one"][1] == list(_lib.HIPCC_FLAGS) and B["w2"][1] == list(_lib.HIPCC_FLAGS_W2)
    assert B["generic"][1] == list(_lib.HIPCC_FLAGS) + ["-DORR_GENERIC_PGS"]
    assert len({v[0] for v in B.values()}) == 3 and not {v[0] for v in B.values()} & {v[0] for v in probe_lib.BUILDS.values()}


def test_every_probe_build_has_one_command_shape_and_a_library_of_its_own():
    """All six builds go through one ProbeBuilds: the compiler, the build's flags, the two include paths, the output, the source."""
    from openroborl_amd import _lib
    from tests import probe_noise_lib
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    libs = []
    for mod in (probe_lib, probe_solver_lib):
        for b, (name, flags) in mod.BUILDS.items():
            assert mod.compile_command(b, "out.so") == [_lib.HIPCC] + list(flags) + ["-I", _lib.CSRC, "-I", include, "-o", "out.so", mod.SRC]
            libs.append(mod.lib_path(b))
    assert probe_noise_lib.compile_command("out.so") == (
        [_lib.HIPCC] + list(_lib.HIPCC_FLAGS) + ["-I", _lib.CSRC, "-I", include, "-o", "out.so", probe_noise_lib.SRC])
    libs.append(probe_noise_lib.LIB)
    assert all(os.path.dirname(p) == probe_lib.PROBE_DIR for p in libs)
    assert len(libs) == 6 and len({os.path.basename(p) for p in libs}) == 6


def test_probe_is_no_part_of_the_product_library():
    from openroborl_amd import _lib
    assert not any("device_probe" in d or "orr_probe" in d for d in _lib.DEPS)
    assert not any(os.path.samefile(os.path.dirname(d), probe_lib.PROBE_DIR) for d in _lib.DEPS)


# ---- A: the lane-movement references against per-lane loops ----------------------------------------------------------------
def test_suffix_sum_reference_is_the_per_lane_definition():
    x = R.wave_inputs(128, 2, 1)
    got = R.suffix_sum_ref(x)
    for i in range(128):
        base, lane = i & ~15, i & 15
        leg, part = lane & 3, lane >> 2
        v = lambda p: x[base + leg + 4 * p]   # noqa: E731
        want = [(v(0) + v(1)) + v(2), v(1) + v(2), v(2), v(3)][part]
        assert np.array_equal(got[i], want)


def test_first_moment_reference_is_the_per_lane_definition():
    rec = R.first_moment_inputs(128, 2, "random")
    got, scale = R.first_moment_ref64(rec)
    r = rec.astype(np.float64)
    for i in range(128):
        base, lane = i & ~15, i & 15
        leg, part = lane & 3, lane >> 2
        for k in range(3):
            h = lambda p: r[base + leg + 4 * p, 4 + k] if p <= 2 and part < 3 else 0.0   # noqa: E731
            own = r[i, 0] * r[i, 1 + k]
            want = (own + h(part + 1)) + h(part + 2)
            assert got[i, k] == want
            assert scale[i, k] >= abs(want) and scale[i, k] >= abs(own)
    # dyadic inputs are exact in float32: the float64 result is a float32 number, and so is every partial sum
    rec = R.first_moment_inputs(4096, 3, "dyadic")
    got, _ = R.first_moment_ref64(rec)
    assert np.array_equal(got.astype(F32).astype(np.float64), got)
    assert np.array_equal((rec[:, :1].astype(np.float64) * rec[:, 1:4]).astype(F32), rec[:, 4:7])


def test_triplet_reference_is_the_per_lane_definition():
    rec = R.wave_inputs(128, 21, 4)
    got, mag = R.triplet_ref64(rec)
    r = rec.astype(np.float64)
    for i in range(0, 128, 5):
        for g in range(4):
            src = r[(i & ~15) + 4 + g]
            rr, ck = src[0:3], src[3:12].reshape(3, 3)
            want = r[i, 15:18] + np.cross(r[i, 12:15], rr) + ck.T @ r[i, 18:21]
            assert np.allclose(got[i, 3 * g:3 * g + 3], want, rtol=1e-13, atol=1e-13)
            assert (mag[i, 3 * g:3 * g + 3] >= np.abs(want) - 1e-12).all()
    rec = R.wave_inputs(4096, 21, 5, "dyadic")
    got, _ = R.triplet_ref64(rec)
    assert np.array_equal(got.astype(F32).astype(np.float64), got)


def test_bcast_and_row_sum_references():
    x = R.wave_inputs(128, 1, 6)[:, 0]
    b = R.bcast_ref(x, range(16))
    s, sa = R.row_sum_ref64(x)
    for i in range(128):
        assert np.array_equal(b[i], x[(i & ~15):(i & ~15) + 16])
        assert s[i] == x[(i & ~15):(i & ~15) + 16].astype(np.float64).sum()
        assert sa[i] >= abs(s[i])


# ---- B: the math references against the oracle and the reference shim -----------------------------------------------------------
def _sample(x, k=300, seed=0):
    return x[np.random.RandomState(seed).choice(len(x), k, replace=False)]


def test_math_references_agree_with_the_oracle():
    L = ol.lib()
    dp = ol.dp
    L.orc_heading.argtypes = [dp]
    L.orc_euler_from_quat.argtypes = [dp, dp]
    L.orc_axis_angle.argtypes = [dp, dp, dp]
    q = _sample(R.gen_euler()[0]).astype(np.float64)
    want = np.empty((len(q), 3))
    for i in range(len(q)):
        L.orc_euler_from_quat(ol.P(q[i]), ol.P(want[i]))
    assert R.circ(R.euler_def(q), want).max() < 1e-12
    q = _sample(R.gen_heading()[0]).astype(np.float64)
    want = np.array([L.orc_heading(ol.P(q[i])) for i in range(len(q))])
    assert R.circ(R.heading_def(q), want).max() < 1e-12
    q = _sample(R.gen_norm_angle()[0]).astype(np.float64)
    want = np.empty(len(q))
    for i in range(len(q)):
        ax, ang = np.zeros(3), C.c_double()
        L.orc_axis_angle(ol.P(q[i]), ol.P(ax), C.byref(ang))
        want[i] = L.orc_normalize_angle(ang.value)
    assert R.circ(R.norm_angle_def(q), want).max() < 1e-12
    a = _sample(R.gen_map_pi()).astype(np.float64)
    assert np.abs(R.map_pi_def(a) - np.array([L.orc_map_pi(v) for v in a])).max() == 0
    x, _, dropped = R.gen_slerp()
    x = _sample(x[~dropped], 600).astype(np.float64)
    got, _ = R.slerp_def(x[:, 0:4], x[:, 4:8], x[:, 8])
    want = np.empty((len(x), 4))
    for i in range(len(x)):
        L.orc_slerp(ol.P(x[i, 0:4].copy()), ol.P(x[i, 4:8].copy()), float(x[i, 8]), ol.P(want[i]))
    assert np.abs(got - want).max() < 1e-9       # acos(d) at angles of 1e-7 amplifies the last bit of d


def test_math_references_agree_with_the_reference_shim():
    sys.path.insert(0, os.path.join(ol.GOLDEN, "_shims"))
    try:
        from pybullet_utils import transformations as T
    finally:
        sys.path.pop(0)
    x, _, dropped = R.gen_slerp()
    x = _sample(x[~dropped], 300, seed=1).astype(np.float64)
    got, _ = R.slerp_def(x[:, 0:4], x[:, 4:8], x[:, 8])
    want = np.array([T.quaternion_slerp(r[0:4], r[4:8], r[8]) for r in x])
    assert np.abs(got - want).max() < 1e-9
    p, q, _ = R.gen_quat_points()
    p, q = p[:200].astype(np.float64), q[:200].astype(np.float64)
    want = np.array([T.quaternion_multiply(T.quaternion_multiply(q[i], np.append(p[i], 0.0)), T.quaternion_inverse(q[i]))[:3]
                     for i in range(200)])
    assert np.abs(R.qrot_def(p, q) - want).max() < 1e-14
    # q_to_mat rotates like qrot
    assert np.abs(np.einsum("nij,nj->ni", R.q_to_mat_def(q).reshape(-1, 3, 3), p) - want).max() < 1e-13


def test_float32_floor_is_a_float32_evaluation():
    q = R.gen_euler()[0][:100]
    for f in (R.euler_def, R.heading_def, R.norm_angle_def, R.q_to_mat_def):
        assert f(q, F32).dtype == F32
    assert R.qrot_def(q[:, :3], q, F32).dtype == F32


# ---- B: the generators fill their buckets -----------------------------------------------------------------------------------
def _check_buckets(n, buckets):
    covered = np.zeros(n, dtype=bool)
    for name, m in buckets.items():
        assert m.shape == (n,) and m.sum() >= R.MIN_BUCKET, (name, int(m.sum()))
        assert not (covered & m).any(), name      # disjoint
        covered |= m
    assert covered.all()


def test_bucketed_generators_fill_every_bucket():
    for gen in (R.gen_atan2, R.gen_asin, R.gen_euler, R.gen_heading, R.gen_norm_angle):
        x, b = gen()
        assert len(x) <= 2 ** 20 and x.dtype == F32 and np.isfinite(x).all()
        _check_buckets(len(x), b)
    p, q, b = R.gen_quat_points()
    _check_buckets(len(q), b)
    rec, b = R.gen_chol()
    _check_buckets(len(rec), b)
    assert b["composite_inertia"].sum() == 4096


def test_euler_buckets_are_what_they_say():
    q, b = R.gen_euler()
    s = np.abs(R.euler_sarg64(q))
    edges = list(R.PITCH_EDGES) + [1.0]
    for (name, m), lo, hi in zip(b.items(), edges, edges[1:]):
        assert (s[m] >= lo).all() and (s[m] <= hi).all(), name
    assert (s[b["clamped"]] > 1.0).all()
    assert set(np.sign(R.euler_sarg64(q[b["clamped"]]))) == {-1.0, 1.0}
    x, b = R.gen_asin()
    assert (np.abs(x) <= 1).all() and (np.abs(x) == 1).sum() >= 2
    for (name, m), lo, hi in zip(b.items(), edges, edges[1:]):
        assert (np.abs(x[m]) >= F32(lo)).all() and (np.abs(x[m]) <= hi).all(), name


def test_heading_and_angle_buckets_are_what_they_say():
    q, b = R.gen_heading()
    h = R.heading_def(q)
    assert (np.abs(h[b["near_0"]]) < 1e-3).all() and (np.pi - np.abs(h[b["near_pi"]]) < 1e-3).all()
    assert set(np.sign(h[b["near_pi"]])) == {-1.0, 1.0} and set(np.sign(h[b["near_0"]])) >= {-1.0, 1.0}
    nrm = np.sqrt((q[b["unnormalised"]].astype(np.float64) ** 2).sum(axis=1))
    assert nrm.min() < 0.6 and nrm.max() > 1.8 and nrm.min() >= 0.5 - 1e-6 and nrm.max() <= 2 + 1e-6
    q, b = R.gen_norm_angle()
    w = q[:, 3]
    assert (w[b["near_0"]] > 0.99).all() and (w[b["near_2pi"]] < -0.99).all()
    assert (w[b["near_pi_w_pos"]] >= 0).all() and (w[b["near_pi_w_neg"]] < 0).all() and (np.abs(w[b["near_pi_w_pos"]]) < 1e-3).all()
    a = R.norm_angle_def(q)
    assert (np.abs(a[b["near_0"]]) < 1e-3).all() and (np.abs(a[b["near_2pi"]]) < 1e-3).all()
    assert (np.pi - np.abs(a[b["near_pi_w_pos"]]) < 1e-3).all() and (np.pi - np.abs(a[b["near_pi_w_neg"]]) < 1e-3).all()


def test_atan2_inputs_cover_what_the_test_names():
    x, b = R.gen_atan2()
    y, xx = x[:, 0], x[:, 1]
    tiny = np.finfo(F32).tiny
    nz = x[x != 0]
    assert np.abs(nz).min() >= 4 * tiny * (1 - 1e-6) and np.abs(nz).min() < 5 * tiny and np.abs(x).max() > 0.9e30     # no subnormals here
    for sy in (False, True):
        for sx in (False, True):
            for name in ("log_grid", "log_random", "angles", "diagonal", "switch", "axes"):
                assert ((np.signbit(y) == sy) & (np.signbit(xx) == sx) & b[name]).sum() > 100, (name, sy, sx)
    assert (np.abs(y[b["diagonal"]]) == np.abs(xx[b["diagonal"]])).all()
    assert ((y == 0) & b["axes"]).sum() >= 1000 and ((xx == 0) & b["axes"]).sum() >= 1000
    r = np.hypot(y[b["angles"]].astype(np.float64), xx[b["angles"]])
    assert r.min() < 2e-3 and r.max() > 5e2
    # the switch point of the polynomial branches: t = min / max takes each of the 17 floats around tan(pi / 8)
    s = x[b["switch"]].astype(np.float64)
    t = (np.abs(s).min(axis=1) / np.abs(s).max(axis=1)).astype(F32)
    assert set(t) == set(R.next_floats(0.41421356237, 8))
    assert (t > F32(0.41421356237)).sum() > 100 and (t <= F32(0.41421356237)).sum() > 100
    sub = np.array(R.ATAN2_SUBNORMAL, dtype=F32)
    assert ((np.abs(sub) < tiny) & (sub != 0)).any(axis=1).all()
    for pair in ((0.0, 1e-40), (1e-40, 1e-40), (1.0, 1e-40)):
        assert pair in R.ATAN2_SUBNORMAL


def test_sincos_and_map_pi_inputs_cover_what_the_test_names():
    a = R.gen_sincos()
    assert len(a) <= 2 ** 20 and np.abs(a).max() <= 101 and np.abs(a).max() >= 100
    have = set(a.tolist())
    for k in range(-64, 65):
        assert set(R.next_floats(k * math.pi / 2, 4).tolist()) <= have
    assert F32(1e-30) in a and np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()
    assert np.diff(np.sort(a[np.abs(a) <= 100])).max() < 1e-3      # dense
    a = R.gen_map_pi()
    assert len(a) <= 2 ** 20 and np.abs(a).max() <= 1000 and np.abs(a).max() > 999
    have = set(a.tolist())
    for c in (math.pi, -math.pi, 2 * math.pi, -2 * math.pi, 100 * math.pi, -318 * math.pi, 317 * math.pi):
        assert set(R.next_floats(c, 4).tolist()) <= have, c


def test_slerp_inputs_cover_what_the_test_names():
    x, b, dropped = R.gen_slerp()
    _check_buckets(len(x), b)
    a, bb, f = x[:, 0:4].astype(np.float64), x[:, 4:8].astype(np.float64), x[:, 8]
    d = (a * bb).sum(axis=1) / np.sqrt((a * a).sum(axis=1) * (bb * bb).sum(axis=1))
    ang = 2 * np.arctan2(np.sqrt(((R._unit(bb) - R._unit(a)) ** 2).sum(axis=1)), np.sqrt(((R._unit(bb) + R._unit(a)) ** 2).sum(axis=1)))
    for name, (lo, hi) in R.SLERP_ANGLES.items():
        m = b[name]
        assert (ang[m] > lo * 0.5).all() and (ang[m] < hi + 1e-6).all(), name
        assert ang[m].min() < lo * 1.5 + 1e-3 and ang[m].max() > hi * 0.7, name
        assert (dropped & m).sum() < 0.01 * m.sum()
    assert (d[b["pi/2..pi-1e-3"]] < 1e-3).all() and (d[b["antipodal"]] < -0.999999).all()
    assert (np.abs(d[b["identical"]]) > 1 - 1e-12).all() and (d[b["identical"]] < 0).sum() > 1000
    assert (f[b["f=0"]] == 0).all() and (f[b["f=1"]] == 1).all()
    assert dropped.sum() > 0 and (np.abs(d[dropped]) < 1e-3).all() and not dropped[b["f=0"] | b["f=1"]].any()
    na = np.sqrt((a[b["unnormalised"]] ** 2).sum(axis=1))
    assert na.min() < 0.6 and na.max() > 1.8


# ---- C, D ------------------------------------------------------------------------------------------------------------------
def test_cholesky_inputs_are_spd_with_the_named_conditioning():
    rec, b = R.gen_chol()
    A = rec[:, :36].reshape(-1, 6, 6).astype(np.float64)
    assert np.array_equal(A, np.transpose(A, (0, 2, 1)))
    ev = np.linalg.eigvalsh(A)
    assert (ev[:, 0] > 0).all()
    cond = ev[:, -1] / ev[:, 0]
    assert cond[b["random_spd"]].max() > 0.9e5 and cond[b["random_spd"]].max() < 1.2e5 and cond[b["random_spd"]].min() < 2
    m = A[b["composite_inertia"], 3, 3]            # total mass of 13 bodies of 0.25 .. 13 kg
    assert m.min() > 13 + 12 * 0.25 and m.max() < 13 * 13
    # the backward-error formula: an exact solve has none, a perturbed one has the perturbation's size
    x = np.linalg.solve(A, rec[:, 36:, None].astype(np.float64))[:, :, 0]
    assert R.chol_backward_error(rec, x).max() < 1e-14
    be = R.chol_backward_error(rec, x * (1 + 1e-3))       # residual 1e-3 |b|: at most 1e-3, less where |A| |x| exceeds |b|
    assert be.max() <= 1e-3 and 1e-5 < np.median(be[b["composite_inertia"]]) < 1e-3


def test_philox_and_time_limit_inputs_cover_what_the_test_names():
    s, r, e, b = R.gen_philox()
    for v in (2 ** 32 - 1, 2 ** 32, 0xDEADBEEF12345678, 2 ** 64 - 1):
        assert (s == np.uint64(v)).any()
    for v in (2 ** 31, 2 ** 32 - 1):
        assert (r == v).any() and (e == v).any() and ((r == v) & (e == v)).any()
    assert set(b.tolist()) == set(range(64))
    L = ol.lib()
    from openroborl_amd import _abi
    for cur, steps, start, end in R.TIME_LIMIT_CONFIGS:
        tot = R.gen_time_limit_totals(steps, start, end)
        assert tot.max() >= 2 ** 40 and tot.min() < 0 and len(tot) < 20000
        if cur and steps > 0 and abs(end - start) <= 2000 and 3 * abs(end - start) < steps:     # the ramp's slope is below one limit per step
            cfg = _abi.OrrConfig()
            cfg.flags, cfg.curriculum_steps, cfg.ep_len_start, cfg.ep_len_end = _abi.FLAG_CURRICULUM, steps, start, end
            lim = {L.orc_time_limit(C.byref(cfg), int(t)) for t in tot}
            assert lim == set(range(min(start, end), max(start, end) + 1)), (steps, start, end)     # every boundary is crossed


# ---- E: the solver stages' references and generators ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solver_bucket(name):
    P = R.gen_solver_bucket(name)
    return P, R.pgs_ref64(R.scaled_system64(P, True), P, R.SOLVER_ITERS + 1)


def test_solver_jacobians_are_the_row_setup_ones():
    """contact rows: ((rr x dir, dir), dir . ck[k]) on the base and on the joints of the row's own leg only; knee rows e_knee; limit
    rows +-e_joint"""
    P, _ = solver_bucket("limits")
    J = R.solver_jacobians(P)
    rr, ck = P["rr"].astype(np.float64), P["ck"].astype(np.float64)
    for i in (0, 5, 1023):
        for r in range(28):
            want = np.zeros(18)
            if r < 4:
                want[6 + 3 * r + 2] = 1.0
            elif r < 16:
                want[6 + r - 4] = P["sgn"][i, r - 4]
            else:
                leg = r - 16 if r < 20 else (r - 20) // 2
                d = np.eye(3)[2 if r < 20 else (r - 20) % 2]
                want[0:3], want[3:6] = np.cross(rr[i, leg], d), d
                for k in range(3):
                    want[6 + 3 * leg + k] = d @ ck[i, leg, k]
            assert np.array_equal(J[i, r], want), (i, r)
    assert set(np.unique(P["sgn"])) == {-1.0, 1.0}
    # W = M^-1 J^T, rounded to float32: M^-1 recovered from the eighteen independent columns is symmetric positive definite with its
    # eigenvalues 2.5 decades apart
    W = P["W"].astype(np.float64)
    for i in (0, 7):
        Minv = np.linalg.lstsq(J[i], W[i], rcond=None)[0]
        assert np.abs(Minv - Minv.T).max() < 1e-5 * np.abs(Minv).max()
        ev = np.linalg.eigvalsh((Minv + Minv.T) / 2)
        assert ev[0] > 0 and abs(np.log10(ev[-1] / ev[0]) - 2.5) < 0.01


def test_solver_references_are_the_per_robot_loops():
    for name, has_b in (("limits", True), ("limits", False), ("missing_legs", False), ("soft", True)):
        P, _ = solver_bucket(name)
        A, mag = R.delassus_ref64(P, has_b)
        S = R.scaled_system64(P, has_b, A)
        L = R.pgs_ref64(S, P, 4)
        for i in (0, 3, 514):
            Ab, magb = R.delassus_ref64_brute(P, has_b, i)
            assert np.abs(A[i] - Ab).max() <= 1e-13 * max(np.abs(Ab).max(), 1) and np.abs(mag[i] - magb).max() <= 1e-13 * magb.max()
            assert (mag[i] >= np.abs(A[i]) * (1 - 1e-12)).all()
            Lb = R.pgs_ref64_brute(S["y0"][i], S["Ac"][i], S["lam0"][i], P["lo_c"][i].astype(np.float64), P["hi_c"][i].astype(np.float64),
                                   P["mu"][i].astype(np.float64), S["swept"][i], 4)
            assert np.abs(L[:, i] - Lb).max() <= 1e-12, (name, has_b, i)
        v = R.visited_columns(P, has_b)
        assert (A[~np.broadcast_to(v[:, None, :], A.shape)] == 0).all() and (S["lam0"][~v] == 0).all()
        assert not v[:, 4:16].any() if not has_b else v[:, 4:16].any() == (name == "limits")


def test_solver_ref64_is_the_oracle_row_update():
    """pgs_ref64 is stated with scaled inputs; here the oracle's own statement, unscaled, on one robot:
    lam_r <- clamp(lam_r + (rhs_r - A_r . lam - cfm_r lam_r) / (A_rr + cfm_r)) with the exact reciprocal"""
    P, _ = solver_bucket("soft")
    A, _ = R.delassus_ref64(P, True)
    for i in (1, 2, 600):
        act = P["active"][i]
        D = A[i].diagonal() + P["cfm"][i]
        jdi = np.where(act, 1.0 / np.where(act, D, 1.0), 0.0)
        rhs = np.where(act, P["rhs"][i].astype(np.float64) / np.where(act, P["jdi"][i], 1.0), 0.0)       # unscaled
        lam = P["lam"][i].astype(np.float64)
        for _ in range(3):
            for r in range(28):
                if not act[r]:
                    continue
                v = lam[r] + (rhs[r] - A[i, r] @ lam - P["cfm"][i, r] * lam[r]) * jdi[r]
                hi = P["mu"][i, r] * lam[R.NRM_SLOT[r]] if R.NRM_SLOT[r] >= 0 else float(P["hi_c"][i, r])
                lo = -hi if R.NRM_SLOT[r] >= 0 else float(P["lo_c"][i, r])
                lam[r] = min(max(v, lo), hi)
        # the scaled form takes the float32 jdi for 1 / (A_rr + cfm): they differ by its rounding, 2^-24 relative, per row
        S = R.scaled_system64(P, True, A)
        got = R.pgs_ref64({k: (x[i:i + 1] if k != "swept" else x[i:i + 1]) for k, x in S.items()}, {k: P[k][i:i + 1] for k in ("lo_c", "hi_c", "mu")}, 3)[3, 0]
        assert np.abs(got - lam).max() <= 2e-6 * np.abs(lam).max(), i


def test_solver_yform_in_float64_is_pgs_ref64():
    for name in R.SOLVER_BUCKETS:
        for has_b in (False, True):
            if name == "limits" and not has_b:
                continue
            P, _ = solver_bucket(name)
            I = R.solver_lane_inputs(P, has_b, np.float64)
            Y = R.pgs_yform(I, has_b, R.SOLVER_ITERS)
            L = R.pgs_ref64(R.scaled_system64(P, has_b), P, R.SOLVER_ITERS)
            assert Y.dtype == np.float64 and np.abs(Y - L).max() <= 1e-12, (name, has_b, np.abs(Y - L).max())
    I = R.solver_lane_inputs(P, True)
    assert R.pgs_yform(I, True, 1).dtype == F32 and all(I[k].dtype == F32 for k in I if k != "swept")


def test_solver_buckets_are_what_they_say():
    frac = {}
    for name in R.SOLVER_BUCKETS:
        P, L = solver_bucket(name)
        n = len(P["rr"])
        assert n >= R.MIN_BUCKET and n % 4 == 0 and P["W"].dtype == F32 and all(np.isfinite(v).all() for k, v in P.items() if k != "name")
        act, st = P["active"], R.solver_bucket_stats(P, L)
        frac[name] = st
        print("SOLVER_BUCKET", name, " ".join("%s=%.3g" % kv for kv in st.items()))
        warm = (P["lam"] != 0).any(axis=1)
        if name == "idle":
            assert not act.any() and P["mask"].max() == 0 and (L == 0).all() and not warm.any()
            assert (P["jdi"] == 0).all() and (P["rhs"] == 0).all() and np.abs(P["W"]).min(axis=(1, 2)).max() > 0     # responses stay
            continue
        assert 0.4 < warm.mean() < 0.6 and (P["lam"][~act] == 0).all() and (P["jdi"][~act] == 0).all() and (P["hi_c"][~act] == 0).all()
        assert (P["lam"][:, 4:20] >= 0).all() and (np.abs(P["lam"][:, 0:4]) <= P["hi_c"][:, 0:4]).all()
        assert (P["lo_c"][:, 0:4] == -P["hi_c"][:, 0:4]).all() and (P["mu"][:, :20] == 0).all()
        assert np.array_equal(act[:, 20:28], np.repeat(act[:, 16:20], 2, axis=1))
        assert (act[:, 4:16].any()) == (name == "limits") and ((P["cfm"] > 0).any()) == (name == "soft")
        for key in ("friction_on_cone", "friction_inside", "normal_zero", "normal_positive", "knee_on_bound", "knee_inside"):
            assert st[key] >= 0.10, (name, key, st[key])
        mu = P["mu"][:, 20:28][act[:, 20:28]]
        lo, hi = (0.2, 0.5) if name == "sliding" else (0.5, 1.0)
        assert mu.min() >= F32(lo) and mu.max() <= F32(hi) and mu.max() - mu.min() > 0.9 * (hi - lo)
    P, _ = solver_bucket("standing")
    assert P["active"][:, 16:].all()
    assert frac["standing"]["last_sweep_change"] > 1e-6 and frac["limits"]["last_sweep_change"] > 1e-6
    # sliding: higher tangential right-hand sides against lower friction than standing
    Ps, _ = solver_bucket("sliding")
    tang = lambda Q: np.abs(Q["rhs"][:, 20:28][Q["active"][:, 20:28]] / Q["jdi"][:, 20:28][Q["active"][:, 20:28]]).mean()   # noqa: E731
    assert tang(Ps) > 1.5 * tang(P) and frac["sliding"]["friction_on_cone"] > 1.5 * frac["standing"]["friction_on_cone"]
    P, L = solver_bucket("limits")
    st = frac["limits"]
    assert st["limit_zero"] >= 0.10 and st["limit_positive"] >= 0.10
    assert 0.2 < P["active"][:, 4:16].mean() < 0.3
    bits = ((np.repeat(P["mask"], 4)[:, None] >> np.arange(4, 16, dtype=np.uint32)[None, :]) & 1).astype(bool)
    assert (bits | ~P["active"][:, 4:16]).all() and (bits & ~P["active"][:, 4:16]).mean() > 0.2     # bits of rows the robot lacks
    P, _ = solver_bucket("missing_legs")
    legs = (P["mask"] >> np.uint32(16)) & np.uint32(0xF)
    assert (legs != 0xF).all() and len(set(legs.tolist())) > 4
    P, _ = solver_bucket("soft")
    assert ((P["cfm"][:, 16:20] > 0) == P["active"][:, 16:20]).all() and (P["cfm"][:, :16] == 0).all() and (P["cfm"][:, 20:] == 0).all()


def test_solver_records_carry_the_problem():
    P, _ = solver_bucket("limits")
    rec = R.delassus_records(P).reshape(-1, 16, probe_solver_lib.DEL_IN)
    assert rec.dtype == F32
    for lane in range(16):
        r = R.LANE_SLOT_A[lane]
        assert np.array_equal(rec[:, lane, 0], P["active"][:, r].astype(F32)) and np.array_equal(rec[:, lane, 7], P["jdi"][:, r])
        assert (rec[:, lane, 1] == R.SLOT_LEG[r]).all() and (rec[:, lane, 2] == R.NRM_SLOT[r]).all()
        assert np.array_equal(rec[:, lane, 13:31], P["W"][:, r])
        if lane >= 4:
            assert np.array_equal(rec[:, lane, 31 + 8], P["lam"][:, lane]) and np.array_equal(rec[:, lane, 31 + 13:62], P["W"][:, lane])
            assert np.array_equal(rec[:, lane, 31 + 3 + (lane - 4) % 3], P["sgn"][:, lane - 4])
        else:
            assert (rec[:, lane, 31:62] == np.array([0, 0, -1] + [0] * 28, dtype=F32)).all()
        if 4 <= lane < 8:
            assert np.array_equal(rec[:, lane, 62:65], P["rr"][:, lane - 4]) and np.array_equal(rec[:, lane, 65:68], P["ck"][:, lane - 4, 0])
    assert np.array_equal(rec[:, :, 74].view(np.uint32), np.repeat(np.repeat(P["mask"], 4)[:, None], 16, axis=1))
    assert np.array_equal(rec[0::4, 0, 74].view(np.uint32), R.wave_masks(P["active"]))
    # the mask's layout: bit = slot below 16, the bank-A lanes 4..15 above
    a = np.zeros((4, 28), dtype=bool)
    a[1, 2] = a[3, 9] = a[0, 17] = a[2, 26] = True
    assert R.wave_masks(a)[0] == (1 << 2) | (1 << 9) | (1 << 17) | (1 << 26)
    I = R.solver_lane_inputs(P, True)
    rec = R.pgs_records(P, I).reshape(-1, 16, probe_solver_lib.PGS_IN)
    assert np.array_equal(rec[:, 5, 76:104], I["lam"]) and np.array_equal(rec[:, 9, 20:48], I["AcA"][:, 9]) and np.array_equal(rec[:, 9, 48:76], I["AcB"][:, 9])
    assert (I["AcA"][:, np.arange(16), R.LANE_SLOT_A] == 0).all() and (I["AcB"][:, np.arange(16), np.arange(16)] == 0).all()
    assert np.array_equal(rec[:, 10, 8], I["lam"][:, 17]) and (rec[:, 10, 9] == 17).all()          # slot 22: friction of toe 1
    Q = R.select_robots(P, np.arange(8)[::-1])
    assert np.array_equal(Q["W"][0], P["W"][7]) and len(Q["mask"]) == 2
