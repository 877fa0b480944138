"""CPU checks behind tests/test_gpu_substep_stages.py: the oracle is unchanged by the row-construction refactor (a digest of 50 env steps),
its row probe agrees with an independent point Jacobian, the buckets of tests/stage_refs.py are what their names say, the comparison
functions accept the clean float32 restatement of the kernel's formulation and reject it with one seeded defect each, the restatement
evaluated in float64 is the reference itself (so its float32 error is rounding alone), the host mirror
of the dump's layout matches the kernel's, and the development build compiles for gfx950 with both step units' flags."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from openroborl_amd import _lib
from tests import oracle_lib as ol
from tests import phys_ref as pr
from tests import stage_refs as SR

# float64 oracle, 64 robots, 50 env steps, taken BEFORE build_rows was split off physics_substep (tests/stage_refs.py: oracle_digest)
ORACLE_DIGEST = {"laikago": "e950be4b6e09694500cedf629b6192fe7d5474f54310971fc1a7b1106ac0443d",
                 "mini_cheetah": "3793abee32cbe515d5d630022f9ad3f5aec0ef0002f1f29a55e46bc582b52dbd"}


@pytest.mark.parametrize("robot", SR.ROBOTS)
def test_oracle_is_bit_identical_to_the_one_before_the_row_probe(robot):
    digest, touched = SR.oracle_digest(robot)
    assert touched > 4000                       # contacts all along
    assert digest == ORACLE_DIGEST[robot]


@pytest.mark.parametrize("robot", SR.ROBOTS)
def test_row_probes_contact_jacobians_match_an_independent_point_jacobian(robot):
    """orc_rows_probe's contact rows against J = d . (v_com + w x (P - com)) of the lower leg from tests/phys_ref.py's body Jacobians"""
    inp = SR.inputs("random", robot)
    lay = ol.layout()
    orc = SR.oracle_env(inp.names, inp.models(), inp.cfg)
    orc.state[:] = inp.st
    m = SR.dec_model(inp.models()[inp.types[0]])
    worst, n = 0.0, 0
    dirs = {0: np.array([0.0, 0, 1]), 1: np.array([1.0, 0, 0]), 2: np.array([0.0, 1, 0])}
    for i in range(len(inp.st)):
        rows, _, legs = SR.oracle_rows(orc, i, inp.tau[i])
        s = inp.st[i]
        bodies, axes = pr.kinematics(m, s[lay.sl("POS")], s[lay.sl("QUAT")], s[lay.sl("Q")])
        Js = pr.body_jacobians(bodies, axes)
        for slot in range(16, 28):
            if rows[slot, 0] == 0:
                continue
            leg = SR.SLOT_LEG[slot]
            b = 1 + 3 * leg + 2
            P = np.array([legs[leg, 0], legs[leg, 1], legs[leg, 2]])
            r = P - bodies[b]["cw"]
            Jp = Js[b][3:6] - np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) @ Js[b][0:3]
            worst = max(worst, np.abs(dirs[SR.SLOT_DIR[slot]] @ Jp - rows[slot, 1:19]).max())
            n += 1
    orc.close()
    print("contact rows %d, largest deviation %.3e" % (n, worst))
    assert n >= 30 and worst < 1e-9


def test_float32_oracle_gives_the_same_probe_in_float32():
    inp = SR.inputs("stance", "laikago")
    o64, o32 = SR.oracle_env(inp.names, inp.models(), inp.cfg), SR.oracle_env(inp.names, inp.models(), inp.cfg, f32="parity")
    o64.state[:] = inp.st
    o32.state[:] = inp.st.astype(np.float32)
    a, b = SR.oracle_rows(o64, 3, inp.tau[3])[0], SR.oracle_rows(o32, 3, inp.tau[3])[0]
    o64.close(); o32.close()
    assert b.dtype == np.float32 and np.array_equal(a[:, 0], b[:, 0]) and a[:, 0].sum() == 16
    assert np.abs(a[:, 1:19] - b[:, 1:19]).max() < 1e-5 and np.abs(a[:, 43] - b[:, 43]).max() < 1e-4 * np.abs(a[:, 43]).max()


def test_buckets_are_what_their_names_say():
    cfg = SR.base_cfg()
    margin, act = ol.dec32(cfg.contact_margin), ol.dec32(cfg.limit_activation)
    for bucket, robot in SR.cases():
        inp = SR.inputs(bucket, robot)
        f = SR.facts(inp)
        lay = ol.layout()
        down = f["dist"] < margin
        pen = f["pen"].min(axis=2)
        assert len(inp.st) == SR.N and len(inp.names) == SR.N
        if bucket == "random":                    # drawn: robots nearer than CLOSE to a discrete choice are left out, few of them
            assert (~inp.keep).mean() <= SR.CLOSE_CAP, (~inp.keep).sum()
            assert (SR.choice_distance(inp)[inp.keep] >= SR.CLOSE).all()
        else:                                     # crafted (`shank`: drawn, then moved off the choices): nobody is that near
            assert inp.keep.all() and SR.choice_distance(inp).min() > SR.CLOSE
        if bucket == "stance":
            assert down.all()
        if bucket == "flight":
            assert not down.any()
        if bucket == "missing_legs":
            assert not down[:4, 1].any() and down[:4, [0, 2, 3]].all() and (down.sum(axis=1) < 4).mean() > 0.5 and down.any(axis=0).all()
        if bucket == "open_in_margin":
            assert ((f["dist"] > 0) & down).all()
        if bucket == "penetrating":
            assert (f["dist"] < 0).all()
        if bucket == "shank":
            assert f["shank"].all() and down.any(axis=1).all()
        if bucket == "soft":
            assert all(m is None or m["contact_stiffness"] > 0 for m in inp.models()) and (f["dist"] < 0).any() and ((f["dist"] > 0) & down).any()
        if bucket == "knee_off":
            assert (inp.st[:, lay.sl("KNEE_FRICTION")] == 0).all()
        if bucket == "knee_on":
            assert (inp.st[:, lay.sl("KNEE_FRICTION")] > 0).all()
        if bucket == "limit_inside":
            on = (f["pen"] < act) & (f["pen"] > 0)
            assert on.any(axis=(1, 2)).all() and not (f["pen"] < 0).any()
            assert on[:, :, 0].any() and on[:, :, 1].any() and on[:, 10].any() and on[:, 11].any()
        if bucket == "limit_beyond":
            on = f["pen"] < 0
            assert on.any(axis=(1, 2)).all() and on[:, :, 0].any() and on[:, :, 1].any() and on[:, 10].any() and on[:, 11].any()
        if bucket == "randomised":
            assert (inp.st[:, lay.sl("MASS_RATIO")] != 1).all() and (inp.st[:, lay.sl("INERTIA_RATIO")] != 1).all() and (inp.st[:, lay.sl("BASE_DAMPING")] > 0).all()
        if bucket == "fast":
            assert np.abs(inp.st[:, lay.sl("QD")]).max() > 25 and np.abs(inp.st[:, lay.sl("ANGVEL")]).max() > 8
        if bucket == "warm":
            lam = inp.st[:, lay.sl("LAMBDA")].reshape(-1, 4, 3)
            assert (lam != 0).all() and (~down).any() and down.any()
        if bucket == "mixed":
            assert all(len(set(inp.names[4 * w:4 * w + 4])) == 2 for w in range(SR.N // 4))
        if bucket == "anchor":
            ref = SR.reference(inp, True)
            before, after = inp.st[:, lay.sl("ANCHOR_VALID")], ref["anchor"][:, :, 6]
            moved = np.abs(ref["anchor"][:, :, :3] - inp.st[:, lay.sl("ANCHOR")].reshape(-1, 4, 6)[:, :, :3]).max(axis=2) > 0
            assert ((before == 1) & (after == 1) & ~moved).any(), "kept"
            assert ((before == 1) & (after == 1) & moved).any(), "replaced"
            assert ((before == 1) & (after == 0)).any(), "dropped"
            assert ((before == 0) & (after == 1)).any(), "new"
            assert ((before == 1) & SR.facts(inp, True)["shank"] & (after == 0)).sum() >= 8, "a cached point on a leg that lies on its shank"
        if bucket not in ("limit_inside", "limit_beyond", "random", "shank", "anchor"):
            assert (pen > act).all(), bucket


DEFECT_BUCKET = {"knee_product": "fast", "inertia_product": "stance", "no_damping": "randomised", "erp_open": "open_in_margin",
                 "jl_neighbour": "missing_legs", "warm_slot": "warm", "no_cfm": "soft"}


def verdict(dev, ref, flo, inp, anchor=False):
    """what the GPU tests assert, on stage dicts: -> list of what is out of bounds"""
    bad = [("long", g[0], g[1], g[2]) for g in SR.compare_long(dev, ref, flo, inp.keep) if not g[1] <= g[2]]
    bad += [("short", g[0], g[1]) for g in SR.compare_short(dev, ref, inp, anchor) if not g[1] <= g[2]]
    bad += [("exact", x) for x in SR.check_stage_relations(dev, ref, inp)]      # the part of check_exact that needs no raw dump
    return bad


@pytest.mark.parametrize("robot", SR.ROBOTS)
@pytest.mark.parametrize("defect", SR.DEFECTS)
def test_a_seeded_defect_is_rejected_and_the_clean_restatement_passes(defect, robot):
    inp = SR.inputs(DEFECT_BUCKET[defect], robot)
    ref, clean = SR.reference(inp), SR.restate(inp)
    assert verdict(clean, ref, clean, inp) == []
    bad = verdict(SR.restate(inp, defect=defect), ref, clean, inp)
    print(defect, robot, bad[:4])
    assert bad, defect


@pytest.mark.parametrize("bucket,robot,anchor", [("randomised", "laikago", False), ("fast", "mini_cheetah", True), ("anchor", "laikago", True),
                                                 ("soft", "mini_cheetah", False), ("limit_beyond", "laikago", False)])
def test_restatement_in_float64_is_the_reference(bucket, robot, anchor):
    """The floor is only as good as the restatement: evaluated in float64 (with the decimal constants the oracle recovers) it must BE the
    reference, to 1e-11 of each quantity's largest magnitude - a wrong or missing term in restate() would otherwise widen every
    long-chain bound of the GPU tests unseen.  What is left in float32 is then rounding alone."""
    inp = SR.inputs(bucket, robot)
    ref, f64 = SR.reference(inp, anchor), SR.restate(inp, f=np.float64, anchor=anchor)
    assert np.array_equal(ref["active"], f64["active"])
    for k in ("ustar", "lc", "T", "Hi", "A0", "J", "MinvJT", "jdi", "rhs", "rhs0", "lo", "hi", "mu", "cfm", "lam", "w", "geom", "margin"):
        e = np.abs(np.asarray(f64[k], dtype=np.float64) - ref[k])
        if k in ("J", "MinvJT"):
            e = e * ref["active"][:, :, None]
        elif e.shape == ref["active"].shape:
            e = e * ref["active"]
        assert e.max() <= 1e-11 * max(1.0, np.abs(ref[k]).max()), (k, e.max())
    assert np.abs(f64["anchor"][:, :, :6] - ref["anchor"][:, :, :6]).max() <= 1e-11


def test_clean_restatement_passes_with_anchors_and_mixed_robots():
    for bucket, robot, anchor in (("anchor", "laikago", True), ("mixed", "mixed", False), ("limit_beyond", "mini_cheetah", False)):
        inp = SR.inputs(bucket, robot)
        ref, clean = SR.reference(inp, anchor), SR.restate(inp, anchor=anchor)
        assert np.array_equal(ref["active"], clean["active"])
        assert verdict(clean, ref, clean, inp, anchor) == []
        assert np.array_equal(clean["anchor"][:, :, 6], ref["anchor"][:, :, 6])


def test_host_layout_matches_the_kernels():
    """orr_debug_stage_words() returns kStageWords; the constants of csrc/orr_env_kernels.h give stage_refs' offsets"""
    src = open(os.path.join(_lib.CSRC, "orr_env_kernels.h")).read()
    body = src[src.index("constexpr int kStageUstar"):src.index("template <bool ANCHOR, int WPE>")]
    env = {"kLanes": 16, "kMaxRows": 28}
    for name, expr in re.findall(r"(kStage\w+) = ([^,;]+)[,;]", body):
        env[name] = eval(expr, {}, env)
    assert (env["kStageUstar"], env["kStageLc"], env["kStageLeg"], env["kStageBf"], env["kStageRow"], env["kStageGeom"], env["kStageW"], env["kStageWords"],
            env["kStageRowWords"]) == (SR.USTAR, SR.LC, SR.LEG, SR.BF, SR.ROW, SR.GEOM, SR.WOFF, SR.WORDS, SR.ROW_WORDS)
    assert "int32_t orr_debug_stage_words(void) { return kStageWords; }" in open(_lib.SRC).read()


@pytest.mark.parametrize("unit", [0, 1])
def test_stage_dump_build_compiles_for_gfx950_with_both_units_flags(unit):
    name, src, flags, _ = _lib.UNITS[unit]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, name + ".s")
        flags = [f for f in flags if f not in ("-shared", "-fPIC")] + ["-DORR_STAGE_DUMP"]
        subprocess.check_call([_lib.HIPCC] + flags + ["-S", "--cuda-device-only", "-o", out, src], stderr=subprocess.DEVNULL)
        text = open(out).read()
    kernels = re.findall(r"^(_Z21orr_stage_dump_kernelILb[01]ELi%d\w+):" % (unit + 1), text, re.M)
    assert len(set(kernels)) == 2, kernels                 # both ANCHOR forms, this unit's WPE
