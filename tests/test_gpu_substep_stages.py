"""The first half of a physics sub-step on the GPU, stage by stage: leg_dynamics -> row_setup_bank_a / row_setup_limit -> row_response
(csrc/orr_physics.h), read through the -DORR_STAGE_DUMP build (orr_stage_dump_kernel, csrc/orr_env_kernels.h; tools/dev_build.py
STAGE_DUMP, built by __graft_entry__.build) and compared with float64 (tests/stage_refs.py: the oracle's orc_dynamics_probe /
orc_rows_probe, tests/phys_ref.py, tools/crba_proto.py).

One child process (tests/stage_dump_child.py: ORR_LIB_PATH must be set before the library loads) dumps every bucket of stage_refs for
both step units (w1: the main unit's flags and forms, w2: ORR_TU_STEP_W2's) and both friction-anchor forms into one .npz; the tests
compare in this process: every bucket in both forms (the `anchor` bucket's models carry the anchor, it has no plain form), 64 cases per
unit.  The child takes about 11 s with the prebuilt library (12 s of 22 s for the whole module on one MI355X, before the references of
the second anchor form were added; they are CPU work of this process, about 1.5 s per case).

Exact checks (bit patterns; the sign of a zero is free): stage_refs.check_exact, and the batch-size / place-in-the-wave / padding tests.
Short paths (lc, Jb, jl, ContactGeom, unscaled rhs, bounds, cfm, limit margin): every entry within (chained roundings + 1) x 2^-24 x
the sum of its terms' magnitudes; the counts are listed at stage_refs.RW_UNITS.
Long chains (u*, T, H^-1, A0, wa / wq, jdi, scaled rhs): per bucket and group, max error against float64 <= FLOOR_FACTOR (2.0, the
solver probe's) x the max error of the numpy-float32 restatement on the same inputs + 2^-22 of the group's largest magnitude
(stage_refs.compare_long).  One factor moved, that of the contact normals' scaled right-hand side (rhs.normal): 3.57 = the measured
ratio 2.853 x 1.25.  Its error is dist / dt, i.e. ulps of the foot height x 1000; in `random`, mini-cheetah ONE open normal row decides
the group's maximum, the restatement is 1.0 ulp off there (2.702e-06), the device 2.8 ulp (7.709e-06, both units), inside the
kinematic chain's counted roundings (lc, ContactGeom and the unscaled rhs of the same dump pass their short-path bounds), and the floor
itself moves by a factor of 4 between two float32 orderings of the same sums (stage_refs.LONG_FACTORS has the figures).
Every test prints `PRIMITIVE <name> <unit> max_err=... bound=... n=...` lines, one per group: the case nearest its bound (run with -s;
profiles/device_primitives.txt).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import stage_refs as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("w1", "w2")
CHILD_TIMEOUT = 90            # s: eight times the measured run of the child; a rebuild inside it (minutes) would not fit
CRASH_CODES = (-6, -11, 134, 139, 124, 137)
cached = functools.lru_cache(maxsize=None)


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("stage") / "dumps.npz")
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stage_dump_child.py"), path], capture_output=True, text=True, timeout=CHILD_TIMEOUT,
                             env={k: v for k, v in os.environ.items() if not k.startswith("ORR_")})
    except subprocess.TimeoutExpired as e:
        pytest.fail("the stage dump child ran into its time limit: nothing more is launched\n%s" % ((e.stdout or b"")[-2000:],))
    if out.returncode in CRASH_CODES:
        pytest.fail("the stage dump child ended with %d (abort / fault / time limit): nothing more is launched\n%s" % (out.returncode, out.stderr[-3000:]))
    assert out.returncode == 0 and "STAGE DUMP OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    return dict(np.load(path))


def report(name, unit, err, bound, n):
    print("PRIMITIVE %s %s max_err=%.3e bound=%.3e n=%d" % (name, unit, err, bound, n))


class Worst(object):
    """One PRIMITIVE line per group instead of one per group and bucket: the case that comes closest to its bound (or misses it by most),
    over n values in all cases; every case that misses its bound gets a line of its own"""

    def __init__(self, unit, suffix=""):
        self.unit, self.suffix, self.w, self.n, self.fails = unit, suffix, {}, {}, []

    def add(self, group, case, err, bound, n):
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
        self.n[group] = self.n.get(group, 0) + n
        if group not in self.w or ratio > self.w[group][0]:
            self.w[group] = (ratio, case, err, bound)
        if not err <= bound:
            self.fails.append((group,) + case + (err, bound))
            report("%s%s MISSES ITS BOUND" % (tag(group, *case), self.suffix), self.unit, err, bound, n)

    def done(self):
        for group in sorted(self.w):
            _, case, err, bound = self.w[group]
            report("%s%s worst of %d cases" % (tag(group, *case), self.suffix, len(compared())), self.unit, err, bound, self.n[group])
        assert not self.fails, self.fails


@cached
def ref(bucket, robot, anchor):
    return SR.reference(SR.inputs(bucket, robot), anchor)


@cached
def floor(bucket, robot, anchor):
    return SR.restate(SR.inputs(bucket, robot), anchor=anchor)


def compared():
    """(bucket, robot, anchor form): every bucket in both forms"""
    return [(b, r, a) for b, r in SR.cases() for a in (False, True) if a or b != "anchor"]


def get(dumps, bucket, robot, unit, anchor):
    return SR.from_dump(dumps["%s/%s/%s/a%d" % (bucket, robot, unit, anchor)])


def tag(group, bucket, robot, anchor=False):
    return "stage.%s[%s,%s%s]" % (group, bucket, robot, ",anchor" if anchor else "")


@pytest.mark.parametrize("unit", UNITS)
def test_discrete_outcomes_and_exact_relations(dumps, unit):
    W = Worst(unit)
    for b, r, a in compared():
        D = get(dumps, b, r, unit, a)
        assert np.isfinite(dumps["%s/%s/%s/a%d" % (b, r, unit, a)]).all(), (b, r, a)
        bad = SR.check_exact(D, ref(b, r, a), SR.inputs(b, r))
        assert not bad, (b, r, a, bad)
        W.add("exact", (b, r, a), 0.0, 0.0, D["rows"].size)
    W.done()


@pytest.mark.parametrize("unit", UNITS)
def test_short_paths(dumps, unit):
    W = Worst(unit, " (units of its bound)")
    for b, r, a in compared():
        for name, ratio, one, n in SR.compare_short(get(dumps, b, r, unit, a), ref(b, r, a), SR.inputs(b, r), a):
            W.add(name, (b, r, a), ratio, one, n)
    W.done()


@pytest.mark.parametrize("unit", UNITS)
def test_long_chains_against_float64(dumps, unit):
    W = Worst(unit)
    for b, r, a in compared():
        for name, err, bound, n, ferr in SR.compare_long(get(dumps, b, r, unit, a), ref(b, r, a), floor(b, r, a), SR.inputs(b, r).keep):
            W.add(name, (b, r, a), err, bound, n)
    W.done()


def test_the_two_units_agree(dumps):
    """w1 against w2: the long chains and the short paths within the bounds each has against float64, the discrete outcomes equal"""
    W, fails, equal = Worst("w1", " w1 vs w2"), [], 0
    for b, r, a in compared():
        inp = SR.inputs(b, r)
        D1, D2 = get(dumps, b, r, "w1", a), get(dumps, b, r, "w2", a)
        equal += np.array_equal(SR.bits(dumps["%s/%s/w1/a%d" % (b, r, a)]), SR.bits(dumps["%s/%s/w2/a%d" % (b, r, a)]))
        other = dict(ref(b, r, a), **{k: D2[k] for k in ("ustar", "T", "Hi", "A0", "MinvJT", "jdi", "rhs")})      # w2 in the reference's place
        apart = dict((g[0], g[1]) for g in SR.compare_long(D1, other, floor(b, r, a), inp.keep))
        for name, err, bound, n, _ in SR.compare_long(D1, ref(b, r, a), floor(b, r, a), inp.keep):
            W.add(name, (b, r, a), apart[name], bound, n)
        for name, ratio, one, n in SR.compare_short(D1, ref(b, r, a), inp, a, other=D2):
            W.add(name + " (units of its bound)", (b, r, a), ratio, one, n)
        for k in ("active", "lo", "hi", "mu", "cfm", "lam"):
            if not np.array_equal(np.asarray(D1[k])[inp.keep], np.asarray(D2[k])[inp.keep]):
                fails.append((b, r, a, k))
    print("units bit-equal in %d of %d dumps" % (equal, len(compared())))      # printed, not asserted
    assert not fails, fails
    W.done()


@pytest.mark.parametrize("unit", UNITS)
def test_anchor_form_without_cached_points_keeps_what_the_anchor_has_no_say_in(dumps, unit):
    """Every bucket in the ANCHOR form (the models carry the anchor, the records no cached point): dynamics, knee and joint-limit rows
    are the plain form's bit for bit, the same rows are active"""
    for b, r in SR.cases():
        if b == "anchor":
            continue
        P, A = get(dumps, b, r, unit, False), get(dumps, b, r, unit, True)
        for k in ("ustar", "lc", "T", "Hi", "bf", "margin"):
            assert np.array_equal(SR.bits(P[k]), SR.bits(A[k])), (b, r, k)
        assert np.array_equal(SR.bits(P["rows"][:, :16]), SR.bits(A["rows"][:, :16])), (b, r)
        keep = SR.inputs(b, r).keep
        assert np.array_equal(P["active"][keep], A["active"][keep]), (b, r)
    report("stage.anchor form, no cached point", unit, 0.0, 0.0, len(SR.cases()) - 2)


@pytest.mark.parametrize("unit", UNITS)
def test_a_robot_does_not_depend_on_batch_size_or_place(dumps, unit):
    """7 robots (a wave with an empty place), 1 robot, and one record in all four places of a wave give the 64-robot batch's bits; no
    word of a padding lane group (or behind the batch) is written"""
    for key in dumps:
        kind, _, rest = key.partition("/")
        if kind not in ("seven", "one", "places") or not key.endswith(unit):
            continue
        b, r = rest.split("/")[:2]
        full = dumps["%s/%s/%s/a0" % (b, r, unit)]
        got = dumps[key]
        if kind == "seven":
            assert np.array_equal(SR.bits(got[:7]), SR.bits(full[:7])), key
            assert np.isnan(got[7:]).all(), key
        elif kind == "one":
            assert np.array_equal(SR.bits(got[0]), SR.bits(full[5])), key
            assert np.isnan(got[1:]).all(), key
        else:
            assert (SR.bits(got) == SR.bits(full[9])[None]).all(), key
    report("stage.batch size and place", unit, 0.0, 0.0, 6)
