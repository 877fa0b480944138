"""The constraint solver's two register stages on the GPU, with inputs the test chooses (through the test-only probe
tests/probe_solver_lib.py, tests/device_probe/orr_probe_solver.hip): delassus_columns<HAS_B> and pgs_sweeps<HAS_B> of
csrc/orr_physics.h, compared with a plain float64 projected Gauss-Seidel in the oracle's form (tests/primitive_refs.py, section E).

Three probe builds: `one` and `w2` carry the hand-scheduled sweeps (pgs_sweeps_bank_a / _bank_ab) under the flags of the two env units,
`generic` the readable C++ form behind ORR_GENERIC_PGS.  Inputs: six named buckets of 1024 robots (standing, sliding, limits,
missing_legs, soft, idle; tests/test_device_probe_cpu.py checks that rows end on both sides of every bound).  Each test prints
`PRIMITIVE <name> <build> max_err=... bound=... n=...` lines in the format of tests/test_gpu_device_primitives.py (run with -s; the
lines of one MI355X run are in profiles/device_primitives.txt beside the leaves': per entry and build the line nearest its bound).

Bounds.  Exact tests compare bit patterns (values where the sign of a zero is free: med3(y, -0, +0) and max(-0, 0) may give either).
Columns: (chained roundings on the entry's path + 1) x 2^-24 of the sum of its terms' magnitudes, counted at COLUMN_ROUNDINGS.
Sweeps: per bucket and sweep count, max error against float64 <= FLOOR_FACTOR x (max error of the generic sweeps restated in numpy
float32 on the same inputs) + 2^-22 of the bucket's largest impulse; the assembly builds also stay that close to the `generic` build.
"""
import functools

import numpy as np
import pytest

from tests import primitive_refs as R
from tests import probe_solver_lib as PS

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS24 = 2.0 ** -24
FLOOR_FACTOR, SLACK_REL = 2.0, 2.0 ** -22
SWEEP_ITERS = (1, 2, 3, 4, 5, 9, 10)
DELASSUS_ITERS = (0, 1, 9, 10)
# Chained roundings between the float32 inputs and an output of delassus_columns:
#   knee / joint-limit column  a = wq[.] (x -+1: exact), Ac = -a jdi: 1
#   contact column             dpp_contact_triplet: v_mul, v_fmac, v_add, three v_fmac = 6, then -a jdi: 7
#   w                          cfm lam (1), then per visited column a product and a sum (2 if not fused) behind each other, 16 columns
#                              without the joint-limit bank and 28 with it, and the triplet's 6 inside a contact column's a
COLUMN_ROUNDINGS = {"knee": 1, "limit": 1, "contact": 7, "w_a": 1 + 2 * 16 + 6, "w_ab": 1 + 2 * 28 + 6}
cached = functools.lru_cache(maxsize=None)


@pytest.fixture(scope="module", params=["one", "w2", "generic"])
def build(request):
    PS.lib(request.param)
    return request.param


def report(name, build, err, bound, n):
    print("PRIMITIVE %s %s max_err=%.3e bound=%.3e n=%d" % (name, build, err, bound, n))


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def same_bits_but_zero_sign(a, b):
    """equal values everywhere (so +0 == -0, NaN never), equal bit patterns wherever the value is not zero"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    return bool((a == b).all() and np.array_equal(bits(a)[a != 0], bits(b)[a != 0]))


def per_robot(out, what="lam"):
    """[R * 16, k] -> [R, k], after checking that the 16 lanes of every robot hold the same bits"""
    o = bits(out).reshape(-1, 16, out.shape[1])
    assert (o == o[:, :1]).all(), "%s differs between the lanes of a robot" % what
    return np.ascontiguousarray(out.reshape(-1, 16, out.shape[1])[:, 0])


bucket = cached(R.gen_solver_bucket)


@cached
def lane_inputs(name, has_b):
    return R.solver_lane_inputs(bucket(name), has_b)


@cached
def pgs_recs(name, has_b):
    return R.pgs_records(bucket(name), lane_inputs(name, has_b))


@cached
def delassus_recs(name):
    return R.delassus_records(bucket(name))


@cached
def sweeps_reference(name, has_b, columns):
    """-> (float64 impulses after 0..10 sweeps, the float32 floor's).  columns False: the sweeps alone, reference and floor on the same
    float32 columns; True: columns + sweeps, reference on delassus_ref64's float64 columns, floor on their float32 roundings"""
    P, I = bucket(name), lane_inputs(name, has_b)
    S = R.scaled_system64(P, has_b) if columns else R.system_from_lane_inputs(I)
    return R.pgs_ref64(S, P, R.SOLVER_ITERS), R.pgs_yform(I, has_b, R.SOLVER_ITERS)


def entry(kind, has_b):
    return kind + ("_ab" if has_b else "_a")


def cases():
    """(bucket, HAS_B): the instantiation without the joint-limit bank never sees a wave with joint-limit rows"""
    return [(name, has_b) for name in R.SOLVER_BUCKETS for has_b in (False, True) if has_b or name != "limits"]


def run_sweeps(build, name, has_b, columns, iters):
    """lam[R, 28] after `iters` sweeps from the probe (lanes checked)"""
    if columns:
        out = PS.run(build, entry("delassus_pgs", has_b), delassus_recs(name), iters)
        return per_robot(out[:, 87:115])
    return per_robot(PS.run(build, entry("pgs", has_b), pgs_recs(name, has_b), iters))


generic_sweeps = cached(functools.partial(run_sweeps, "generic"))


# =====================================================================================================================
# exact
# =====================================================================================================================
def test_no_sweep_returns_the_warm_start(build):
    """iters = 0: the `it <= 0` exits of the assembly forms, the empty loop of the generic one"""
    for name, has_b in cases():
        I = lane_inputs(name, has_b)
        got = run_sweeps(build, name, has_b, False, 0)
        assert np.array_equal(bits(got), bits(I["lam"])), (name, has_b)
        got = run_sweeps(build, name, has_b, True, 0)
        assert np.array_equal(bits(got), bits(I["lam"])), (name, has_b)
    report("pgs[iters=0]", build, 0.0, 0.0, 2 * len(cases()) * got.size)


@cached
def decoupled_inputs():
    """256 robots with every column zero and everything on a dyadic grid (impulses, right-hand sides and bounds multiples of 2^-6 below 16,
    friction coefficients k / 8, jdi a power of two): the rows do not talk to each other, y never moves, every operation is exact, and
    the result is lam[r] = clamp(y_r) whatever the number of sweeps >= 1 -- with each friction bound mu x its toe's normal impulse."""
    rng = np.random.RandomState(77)
    n = 256
    dy = lambda *s: (rng.randint(-1023, 1024, size=s) / 64.0).astype(F32)      # noqa: E731
    I = {"AcA": np.zeros((n, 16, 28), dtype=F32), "AcB": np.zeros((n, 16, 28), dtype=F32)}
    for b in "AB":
        I["lam" + b], I["rhs" + b], I["w" + b] = dy(n, 16), dy(n, 16), dy(n, 16)
        I["jdi" + b] = (2.0 ** rng.randint(-3, 1, size=(n, 16))).astype(F32)
        I["cfm" + b] = np.zeros((n, 16), dtype=F32)
    kinds = np.array(["knee"] * 4 + ["normal"] * 4 + ["friction"] * 8)
    hi = np.abs(dy(n, 16))
    I["hiA"] = np.where(kinds == "knee", hi, np.where(kinds == "normal", R.BIG, F32(0))).astype(F32)
    I["loA"] = np.where(kinds == "knee", -hi, F32(0)).astype(F32)
    I["muA"] = np.where(kinds == "friction", rng.randint(1, 9, size=(n, 16)) / 8.0, 0.0).astype(F32)
    I["hiB"], I["loB"], I["muB"] = np.full((n, 16), R.BIG), np.zeros((n, 16), dtype=F32), np.zeros((n, 16), dtype=F32)
    I["lamA"][:, 4:8] = np.abs(I["lamA"][:, 4:8])
    I["lamB"] = np.abs(I["lamB"])
    for k in ("lamB", "rhsB", "wB", "jdiB", "hiB"):
        I[k] = I[k].astype(F32)
        I[k][:, :4] = 0
    lam = np.zeros((n, 28), dtype=F32)
    lam[:, R.LANE_SLOT_A], lam[:, 4:16] = I["lamA"], I["lamB"][:, 4:]
    I["lam"] = lam
    I["lam_nA"] = np.where(R.NRM_SLOT[R.LANE_SLOT_A][None, :] >= 0, lam[:, np.maximum(R.NRM_SLOT[R.LANE_SLOT_A], 0)], 0).astype(F32)
    I["lam_nB"] = np.zeros((n, 16), dtype=F32)
    mask = (rng.randint(0, 1 << 12, size=n // 4).astype(np.uint32) << np.uint32(4)) | np.uint32(0xFFF000F)
    mask[:4] = np.array([0xFFF000F, 0xFFFFFFF, 0xFFF001F, 0xFFF800F], dtype=np.uint32)      # none, all, the first, the last
    P = {"mask": mask}
    y = np.zeros((n, 28))
    y[:, R.LANE_SLOT_A] = I["lamA"].astype(np.float64) + (I["rhsA"].astype(np.float64) - I["wA"].astype(np.float64) * I["jdiA"])
    y[:, 4:16] = (I["lamB"].astype(np.float64) + (I["rhsB"].astype(np.float64) - I["wB"].astype(np.float64) * I["jdiB"]))[:, 4:]
    assert np.array_equal(y.astype(F32).astype(np.float64), y)
    return P, I, y


def test_decoupled_rows_are_their_clamps(build):
    P, I, y = decoupled_inputs()
    rec = R.pgs_records(P, I)
    hi_k = I["hiA"][:, :4].astype(np.float64)
    mu = np.zeros((len(y), 28))
    mu[:, 20:28] = I["muA"][:, 8:16]
    want = {}
    for has_b in (False, True):
        w = I["lam"].astype(np.float64).copy()
        w[:, 0:4] = np.clip(y[:, 0:4], -hi_k, hi_k)
        w[:, 16:20] = np.maximum(y[:, 16:20], 0)
        b = mu[:, 20:28] * w[:, R.NRM_SLOT[20:28]]                          # each friction bound follows ITS toe's normal impulse
        w[:, 20:28] = np.clip(y[:, 20:28], -b, b)
        if has_b:
            on = ((np.repeat(P["mask"], 4)[:, None] >> np.arange(4, 16, dtype=np.uint32)[None, :]) & 1).astype(bool)
            w[:, 4:16] = np.where(on, np.maximum(y[:, 4:16], 0), w[:, 4:16])
        want[has_b] = w.astype(F32)
        assert np.array_equal(want[has_b].astype(np.float64), w)
    # the inputs exercise what the test names: both sides of every clamp, bounds that differ between the toes of a robot
    w = want[True]
    assert (np.abs(w[:, 0:4]) == hi_k).mean() > 0.1 and (np.abs(w[:, 0:4]) < hi_k).mean() > 0.1
    assert (w[:, 16:20] == 0).mean() > 0.1 and (w[:, 16:20] > 0).mean() > 0.1 and (w[:, 4:16] != I["lam"][:, 4:16]).mean() > 0.1
    b = mu[:, 20:28] * w[:, R.NRM_SLOT[20:28]]
    assert ((np.abs(w[:, 20:28]) == b) & (b > 0)).mean() > 0.1 and (np.abs(w[:, 20:28]) < b).mean() > 0.1
    assert (np.ptp(b, axis=1) > 0).mean() > 0.9
    for iters in range(0, 11):                                              # residues 0, 1, 2 behind the three-sweep loop
        for has_b in (False, True):
            got = per_robot(PS.run(build, entry("pgs", has_b), rec, iters))
            exp = want[has_b] if iters > 0 else I["lam"]
            assert same_bits_but_zero_sign(got, exp), (iters, has_b, np.argwhere(got != exp)[:5])
    report("pgs[decoupled, iters 0..10]", build, 0.0, 0.0, 22 * w.size)


def test_idle_robots_return_zeros(build):
    for has_b in (False, True):
        for iters in (1, 10):
            assert (run_sweeps(build, "idle", has_b, False, iters) == 0).all()
            out = PS.run(build, entry("delassus_pgs", has_b), delassus_recs("idle"), iters)
            assert (out == 0).all()                                          # columns, warm start, w, impulses
    report("pgs[idle]", build, 0.0, 0.0, out.size)


def test_a_robot_does_not_depend_on_its_place_in_the_wave(build):
    """Shuffled over the batch, every robot lands in another lane group next to three other robots (and under another wave mask, which may
    now carry bits of rows the robot lacks: no-ops).  Its impulses stay the same."""
    for name, has_b in (("limits", True), ("missing_legs", False), ("missing_legs", True), ("soft", False)):
        P = bucket(name)
        n = len(P["rr"])
        perm = np.random.RandomState(5).permutation(n)
        assert ((perm & 3) != (np.arange(n) & 3)).mean() > 0.5
        Q = R.select_robots(P, perm)
        assert name == "soft" or (Q["mask"] != P["mask"]).mean() > 0.5      # soft: nearly every wave has every knee and leg anyway
        for columns in (False, True):
            base = run_sweeps(build, name, has_b, columns, 10)
            rec = R.delassus_records(Q) if columns else R.pgs_records(Q, R.solver_lane_inputs(Q, has_b))
            out = PS.run(build, entry("delassus_pgs" if columns else "pgs", has_b), rec, 10)
            got = per_robot(out[:, 87:115] if columns else out)
            assert same_bits_but_zero_sign(got, base[perm]), (name, has_b, columns)
    report("pgs[place in the wave]", build, 0.0, 0.0, got.size)


def test_a_limit_bit_of_an_inactive_row_changes_nothing(build):
    lim = np.uint32(0xFFF0)
    for name in ("standing", "limits", "soft"):
        P = dict(bucket(name))
        base_s, base_c = run_sweeps(build, name, True, False, 10), run_sweeps(build, name, True, True, 10)
        rng = np.random.RandomState(9)
        for extra in (np.full(len(P["mask"]), lim), (rng.randint(0, 1 << 12, size=len(P["mask"])).astype(np.uint32) << np.uint32(4))):
            P["mask"] = bucket(name)["mask"] | extra
            assert (P["mask"] != bucket(name)["mask"]).mean() > 0.5
            # the sweeps alone: the same columns (those of the true mask), the wider mask
            rec = pgs_recs(name, True).copy()
            rec[:, 104] = np.repeat(P["mask"], 64).view(F32)
            assert same_bits_but_zero_sign(per_robot(PS.run(build, "pgs_ab", rec, 10)), base_s), name
            # columns + sweeps: the columns of the extra rows are computed too (J = -+e_joint of a row that is pinned to zero)
            out = PS.run(build, "delassus_pgs_ab", R.delassus_records(P), 10)
            assert same_bits_but_zero_sign(per_robot(out[:, 87:115]), base_c), name
    report("pgs_ab[extra limit bits]", build, 0.0, 0.0, base_c.size)


@pytest.mark.parametrize("build", PS.ASM_BUILDS)
def test_bank_ab_without_limit_rows_is_bank_a(build):
    """the two blocks of assembly do the same arithmetic on the knee and contact rows (the generic form is one piece of code for both)"""
    keep = np.r_[0:4, 16:28]
    for name in R.SOLVER_BUCKETS:
        if name == "limits":
            continue
        for columns in (False, True):
            for iters in (1, 3, 10):
                a, ab = run_sweeps(build, name, False, columns, iters), run_sweeps(build, name, True, columns, iters)
                assert np.array_equal(bits(a[:, keep]), bits(ab[:, keep])), (name, columns, iters)
                assert (ab[:, 4:16] == 0).all()
    report("pgs_ab == pgs_a", build, 0.0, 0.0, a.size)


# =====================================================================================================================
# columns
# =====================================================================================================================
def test_delassus_columns(build):
    kind_of = np.array(["knee"] * 4 + ["limit"] * 12 + ["contact"] * 12)
    units = np.array([COLUMN_ROUNDINGS[k] + 1 for k in kind_of], dtype=np.float64)
    for name, has_b in cases():
        P = bucket(name)
        n = len(P["rr"])
        out = PS.run(build, entry("delassus_pgs", has_b), delassus_recs(name), 0).reshape(n, 16, PS.DEL_OUT)
        AcA, AcB, lam0, wA, wB, lam_n = out[:, :, 0:28], out[:, :, 28:56], out[:, :, 56:84], out[:, :, 84], out[:, :, 85], out[:, :, 86]
        A, mag = R.delassus_ref64(P, has_b)
        S = R.scaled_system64(P, has_b, A)
        v = R.visited_columns(P, has_b)
        jdi, la = P["jdi"].astype(np.float64), R.LANE_SLOT_A
        # the warm start, in every lane; 0 in the slots that are skipped
        want0 = np.where(v, P["lam"], F32(0))
        assert np.array_equal(bits(lam0), bits(np.repeat(want0[:, None, :], 16, axis=1))), (name, has_b)
        nrm = R.NRM_SLOT[la]
        assert np.array_equal(bits(lam_n[:, nrm >= 0]), bits(want0[:, nrm[nrm >= 0]]))
        # skipped slots read 0, and so does the diagonal entry
        vv = np.broadcast_to(v[:, None, :], AcA.shape)
        assert (AcA[~vv] == 0).all() and (AcB[~vv] == 0).all()
        assert (AcA[:, np.arange(16), la] == 0).all() and (AcB[:, np.arange(16), np.arange(16)] == 0).all()
        worst = {}

        def check(what, got, ref, scale, u):
            ok = scale > 0
            assert (got[~ok] == 0).all(), (name, has_b, what)
            rel = np.abs(got[ok] - ref[ok]) / scale[ok]
            worst[what] = max(worst.get(what, 0.0), float((rel / (u[ok] * EPS24)).max()) if ok.any() else 0.0)
            return rel
        offd = np.ones((16, 28), dtype=bool)
        offd[np.arange(16), la] = False
        U = np.broadcast_to(units[None, None, :], AcA.shape)
        for kind in ("knee", "limit", "contact"):
            sel = np.broadcast_to((kind_of == kind)[None, None, :] & offd[None], AcA.shape)
            ref, scale = S["Ac"][:, la, :], mag[:, la, :] * np.abs(jdi[:, la, None])
            rel = check("AcA[%s]" % kind, AcA[sel], ref[sel], scale[sel], U[sel])
            report("delassus%s.AcA[%s,%s]" % ("_ab" if has_b else "_a", kind, name), build, rel.max() if rel.size else 0.0,
                   (COLUMN_ROUNDINGS[kind] + 1) * EPS24, int(sel.sum()))
        wu = COLUMN_ROUNDINGS["w_ab" if has_b else "w_a"] + 1
        wmag = np.abs(P["cfm"].astype(np.float64) * P["lam"]) + np.einsum("nrc,nc->nr", mag, np.abs(S["lam0"]))
        rel = check("A.w", wA, S["w"][:, la], wmag[:, la], np.full(wA.shape, float(wu)))
        report("delassus%s.w[%s]" % ("_ab" if has_b else "_a", name), build, rel.max() if rel.size else 0.0, wu * EPS24, wA.size)
        if has_b:
            offb = np.ones((16, 28), dtype=bool)
            offb[np.arange(16), np.arange(16)] = False
            offb[:4] = False
            for kind in ("knee", "limit", "contact"):
                sel = np.broadcast_to((kind_of == kind)[None, None, :] & offb[None], AcB.shape)
                ref, scale = S["Ac"][:, :16, :], mag[:, :16, :] * np.abs(jdi[:, :16, None])
                check("AcB[%s]" % kind, AcB[sel], ref[sel], scale[sel], U[sel])
            check("B.w", wB[:, 4:], S["w"][:, 4:16], wmag[:, 4:16], np.full(wB[:, 4:].shape, float(wu)))
            assert (AcB[:, :4] == 0).all() and (wB[:, :4] == 0).all()
        else:
            assert (AcB == 0).all()
        assert all(x <= 1.0 for x in worst.values()), (name, has_b, worst)       # in units of each entry's own bound


# =====================================================================================================================
# sweeps, and columns + sweeps, against float64
# =====================================================================================================================
@pytest.mark.parametrize("columns", [False, True], ids=["pgs", "delassus_pgs"])
def test_sweeps_against_float64(build, columns):
    fails = []
    for name, has_b in cases():
        if name == "idle":
            continue
        ref, floor = sweeps_reference(name, has_b, columns)
        slack = SLACK_REL * np.abs(ref).max()
        for iters in (DELASSUS_ITERS[1:] if columns else SWEEP_ITERS):
            got = run_sweeps(build, name, has_b, columns, iters).astype(np.float64)
            assert np.isfinite(got).all()
            bound = FLOOR_FACTOR * np.abs(floor[iters] - ref[iters]).max() + slack
            err = np.abs(got - ref[iters]).max()
            tag = "%s[%s,iters=%d]" % (entry("delassus_pgs" if columns else "pgs", has_b), name, iters)
            report(tag, build, err, bound, got.size)
            if not err <= bound:
                fails.append((tag, err, bound))
            if build in PS.ASM_BUILDS:                                       # ... and the assembly stays that close to the C++ form
                err = np.abs(got - generic_sweeps(name, has_b, columns, iters)).max()
                report(tag + " vs generic", build, err, bound, got.size)
                if not err <= bound:
                    fails.append((tag + " vs generic", err, bound))
    assert not fails, fails
