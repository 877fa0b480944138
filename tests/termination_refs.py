"""The termination block of the env step (csrc/orr_env_kernels.h: _terminal_condition + time limit + non-finite guard) and the fall
proxies of a physics sub-step (csrc/orr_physics.h: physics_substep, want_fall), restated in plain float64 numpy, with the case grids
that tests/test_termination_refs_cpu.py (oracle, float32 mimic) and tests/test_gpu_termination.py (device) both run.

reason64            the DONE_REASON word and the signed margin of every test to its threshold, from ONE robot's record after the step
pos_bound/ang_bound what float32 may do to `pe` and `ang` (derived below, from the device's operations - not from what it returns)
proxy_clearance64   every fall proxy's distance to the contact threshold, through tests/phys_ref.py's kinematics
mimic_reason32, mimic_fall_wave32   float32 restatements of the two device blocks with seeded defects; the comparison of the GPU tests
                    must pass the clean mimic and reject every defect (tests/test_termination_refs_cpu.py)

The gate `STEP_COUNTER > 0 && fall` (imitation_task.py:536: no contact termination in the step that follows a reset of the robot's
own step counter) cannot close in a step: the kernel increments the counter at the end of robot_step, IN FRONT of the termination block
(orr_env_kernels.h, `seti(S, O(STEP_COUNTER), geti(S, O(STEP_COUNTER)) + 1);` under "end of robot_step"), and so does the oracle
(orr_oracle.c step_robot: `seti(s, ORR_OFF_STEP_COUNTER, geti(s, ORR_OFF_STEP_COUNTER) + 1);` in the last sub-step).  Every reset writes
0 and nothing decrements it, so the test reads a counter >= 1.  There is no device case for the closed gate; reason64 and the mimic
honour it, and the CPU test shows the dropped gate on a synthetic record (counter 0) that no step can produce.

Float32 bounds.  u = 2^-24 (one rounding to nearest).
  pe = sum_k (rp_k - p_k)^2:  d_k = fl(rp_k - p_k) carries u |d_k|, so d_k^2 carries 2u; the three products and the adds (plain or
    fused) add at most 3u to a sum of non-negative terms: |pe32 - pe| <= 5u pe, taken as 6u pe.  The threshold thr * thr is rounded
    once: u thr^2.  `pe > thr^2` can differ from float64 only while |pe - thr^2| <= 7u thr^2, i.e. (pe - thr^2 = (dist - thr)(dist +
    thr) ~ 2 thr (dist - thr)) while |thr - dist| <= 3.5u thr, taken as 4u thr: 2.4e-7 m at thr = 1 m.
  ang = q_norm_angle(rp_q (x) conj(q)):  qconj is exact.  A component of qmul is four products and three adds of terms whose
    absolute sum is <= |rp_q| |q| = 1 (Cauchy-Schwarz): 4u each.  n = sqrt(x^2 + y^2 + z^2): the components' errors move it by at
    most sqrt(3) 4u; the sum of squares carries 3u relative, halved by the root (1.5u n), and the hardware square root (v_sqrt_f32, 1 ulp)
    2u n: dn <= (6.93 + 3.5)u with n <= 1, dw <= 4u.  atan2 turns (dn, dw) into at most sqrt(dn^2 + dw^2) / |dq| = 11.2u = 6.7e-7 rad, and
    atan2_bf adds its documented 4.2e-7 (orr_device.h; ATAN2_BOUND of tests/test_gpu_device_primitives.py).  Doubled (the factor 2 is
    exact): 2.17e-6.  The wrap beyond pi subtracts float32(2 pi) (off by 1.75e-7) and rounds a result below pi once (2^-23 = 1.2e-7).
    Total 2.47e-6 rad, taken as 2.5e-6.  fabsf and the comparison with the float32 threshold are exact.
A near case sits at least 16 bounds from its threshold, so a correct float32 evaluation decides it as float64 does.
"""
import numpy as np

from openroborl_amd import _abi
from tests import oracle_lib as ol
from tests import phys_ref as pr

F32 = np.float32
U = 2.0 ** -24
ATAN2_BOUND = 4.2e-7          # tests/test_gpu_device_primitives.py: ATAN2_BOUND
DELTA = 1e-3                  # the fall proxies' distance from the contact threshold, either side (m)
WORDS = 37                    # POS QUAT LINVEL ANGVEL Q QD
CONTACT_FALL, ROOT_POS, ROOT_ROT = _abi.DONE_CONTACT_FALL, _abi.DONE_ROOT_POS, _abi.DONE_ROOT_ROT
TIME_LIMIT, NAN, MOTION_OVER = _abi.DONE_TIME_LIMIT, _abi.DONE_NAN, _abi.DONE_MOTION_OVER
ALL_BITS = CONTACT_FALL | ROOT_POS | ROOT_ROT | TIME_LIMIT | NAN | MOTION_OVER
NEAR_MAX = 1e-4               # a near case is at most this far from its threshold (m, rad)
NEAR_POS, NEAR_ROT = 5e-5, 7e-5
FAR = 0.5
OTHER_DIST_THRESHOLD = 0.75   # exact in float32 and thr^2 != thr: the configuration of the second position grid
MODEL_GROUP = (0, 2, 4, 6)    # the chassis's upper corners: the proxies of the isolating table's grid
BIT_NAMES = ((CONTACT_FALL, "contact_fall"), (ROOT_POS, "root_pos"), (ROOT_ROT, "root_rot"), (TIME_LIMIT, "time_limit"), (NAN, "non_finite"),
             (MOTION_OVER, "motion_over"))


def pos_bound(thr):
    """float32's reach around `pe > thr^2`, as a distance (m): see the module docstring"""
    return 4.0 * U * float(thr)


def ang_bound():
    """float32's reach around `|ang| > thr` (rad): see the module docstring"""
    dn, dw = (np.sqrt(3.0) * 4.0 + 1.5 + 2.0) * U, 4.0 * U
    b = 2.0 * (np.hypot(dn, dw) + ATAN2_BOUND) + abs(float(F32(2.0 * np.pi)) - 2.0 * np.pi) + 2.0 ** -23
    assert 2.4e-6 < b < 2.5e-6
    return 2.5e-6


def thresholds(cfg):
    """(distance, rotation) thresholds as the oracle recovers them from the float32 configuration; the shipped ones are the float32 values"""
    return float(ol.dec32(cfg.dist_fail_threshold)), float(ol.dec32(cfg.rot_fail_threshold))


def root_errors64(ref_pose, pos, quat):
    """pe = |REF_POSE[0:3] - POS|^2 and the normalised angle of REF_POSE[3:7] (x) conj(QUAT), wrapped to (-pi, pi] as q_norm_angle does"""
    with np.errstate(all="ignore"):
        d = np.asarray(ref_pose[0:3], dtype=np.float64) - np.asarray(pos, dtype=np.float64)
        pe = float(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        dq = pr.qmul(np.asarray(ref_pose[3:7], dtype=np.float64), pr.qconj(np.asarray(quat, dtype=np.float64)))
        n = np.sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2])
        ang = float(2.0 * np.arctan2(n, dq[3]))          # in [0, 2 pi]
        if ang > np.pi:
            ang = (ang - 2.0 * np.pi if ang >= 2.0 * np.pi else ang) - 2.0 * np.pi
    return pe, ang


def motion_time64(record, cfg):
    lay = ol.layout()
    t = record[lay.sl("STATE_ACTION_COUNTER")][0] * float(ol.dec32(cfg.sim_dt)) + record[lay.sl("TIME_OFFSET")][0]
    if int(record[lay.sl("WARMUP")][0]):
        t -= float(ol.dec32(cfg.warmup_time))
    return float(t)


def reason64(record, cfg, clip, fall, ep_step_before=None):
    """(bits, margins) of one robot from its float64 record AFTER the step (auto_reset off: the record of the step that ended).
    ep_step_before: EP_STEP ahead of the step (the record's own EP_STEP - 1 when None).  margins: pos (m), rot (rad): threshold - value;
    time (steps): MAX_EP_STEPS - (EP_STEP_before + 1), <= 0 = the limit; motion (s): duration - motion time, None for a clip that wraps."""
    lay = ol.layout()
    g = lambda name: record[lay.sl(name)]
    thr_d, thr_r = thresholds(cfg)
    pe, ang = root_errors64(g("REF_POSE"), g("POS"), g("QUAT"))
    bits = 0
    with np.errstate(all="ignore"):
        if int(g("STEP_COUNTER")[0]) > 0 and fall:
            bits |= CONTACT_FALL
        if pe > thr_d * thr_d:
            bits |= ROOT_POS
        if abs(ang) > thr_r:
            bits |= ROOT_ROT
        motion = None
        if not (clip.flags & _abi.CLIP_WRAP):
            motion = float(clip.duration) - motion_time64(record, cfg)
            if motion <= 0.0:
                bits |= MOTION_OVER
        words = record[lay.sl("POS").start:lay.sl("POS").start + WORDS]
        assert lay.sl("QD").stop == lay.sl("POS").start + WORDS
        if not bool((np.abs(words) < 1e30).all()):
            bits |= NAN
        ep = (int(g("EP_STEP")[0]) - 1 if ep_step_before is None else int(ep_step_before)) + 1
        time = int(g("MAX_EP_STEPS")[0]) - ep
        if time <= 0:
            bits |= TIME_LIMIT
        margins = dict(pos=thr_d - float(np.sqrt(pe)), rot=thr_r - abs(ang), time=time, motion=motion)
    return bits, margins


# ---------------------------------------------------------------------------------------------------------------------------
# fall proxies
# ---------------------------------------------------------------------------------------------------------------------------
def proxy_clearance64(model, pos, quat, q, margin):
    """(o_b + R_b fall_pos)[2] - fall_radius - contact_margin of every fall proxy: negative = the proxy touches"""
    bodies, _ = pr.kinematics(model, pos, quat, q)
    out = np.zeros(int(model["num_fall_proxies"]))
    for k in range(len(out)):
        b = bodies[int(model["fall_body"][k])]
        out[k] = (b["o"] + b["R"] @ np.asarray(model["fall_pos"][k], dtype=np.float64))[2] - float(model["fall_radius"][k]) - margin
    return out


def proxy_clearance_batch(model, pos, quat, q, margin):
    """proxy_clearance64 for [n] poses at once (the pose searches): the same chain, written on arrays; checked against it on the CPU"""
    pos, quat, q = (np.asarray(x, dtype=np.float64) for x in (pos, quat, q))
    n = len(pos)
    dirj, offj, _ = pr.joint_maps(model)
    a = dirj * (q - offj)
    iq = np.asarray(model["init_quat"], dtype=np.float64)
    x1, y1, z1, w1 = quat.T
    x0, y0, z0, w0 = -iq[0], -iq[1], -iq[2], iq[3]
    rel = np.stack([x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0, -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0,
                    x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0, -x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0], axis=1)
    rel /= np.linalg.norm(rel, axis=1, keepdims=True)
    x, y, z, w = rel.T
    Rb = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                   np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                   np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    R, o = [Rb], [pos]
    for j in range(12):
        par = 0 if j % 3 == 0 else j
        ax = np.asarray(model["joint_axis"][j], dtype=np.float64)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        rod = np.eye(3)[None] + np.sin(a[:, j])[:, None, None] * K[None] + (1 - np.cos(a[:, j]))[:, None, None] * (K @ K)[None]
        o.append(o[par] + R[par] @ np.asarray(model["joint_pos"][j], dtype=np.float64))
        R.append(R[par] @ rod)
    out = np.zeros((n, int(model["num_fall_proxies"])))
    for k in range(out.shape[1]):
        b = int(model["fall_body"][k])
        out[:, k] = (o[b] + R[b] @ np.asarray(model["fall_pos"][k], dtype=np.float64))[:, 2] - float(model["fall_radius"][k]) - margin
    return out


def random_poses(model, rng, n):
    """n tumbled poses: uniform orientations, joint angles uniform between the limits (within +-pi where a joint has none) -> (quat, q)"""
    quat = rng.randn(n, 4)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    dirj, offj, _ = pr.joint_maps(model)
    lo, hi = np.maximum(model["joint_lo"], -np.pi), np.minimum(model["joint_hi"], np.pi)
    ang = rng.uniform(lo, hi, (n, 12))
    return quat, ang * dirj + offj


def f32r(x):
    """a float64 array of float32 values: what a record holds"""
    return np.asarray(x, dtype=np.float64).astype(F32).astype(np.float64)


def isolated_proxy_cases(model, margin, only=None, seed=0, n_search=20000):
    """For every proxy i (of `only`) that some pose of the search (n_search tumbled poses, seed) makes the lowest by more than 2 DELTA:
    a pair of cases - i DELTA inside the contact threshold and every other proxy at least DELTA clear (flag 1), the same pose 2 DELTA higher
    (flag 0).  -> ({i: [hit case, clear case]}, [proxies no pose isolated]); a case = dict(proxy, flag, pos, quat, q, clearance),
    positions and angles float32 values, the clearance that of those values, every claim asserted."""
    rng = np.random.RandomState(seed)
    quat, q = random_poses(model, rng, n_search)
    c0 = proxy_clearance_batch(model, np.zeros((n_search, 3)), quat, q, margin)
    order = np.sort(c0, axis=1)
    gap, low = order[:, 1] - order[:, 0], np.argmin(c0, axis=1)
    found, missing = {}, []
    for i in (range(c0.shape[1]) if only is None else only):
        cand = np.nonzero((low == i) & (gap > 2.5 * DELTA))[0]
        if len(cand) == 0:
            missing.append(i)
            continue
        p = cand[np.argmax(gap[cand])]
        pair = []
        for flag, lift in ((1, 0.0), (0, 2.0 * DELTA)):
            pos = f32r([rng.uniform(-1, 1), rng.uniform(-1, 1), -c0[p, i] - DELTA + lift])
            qt, qq = f32r(quat[p]), f32r(q[p])
            cl = proxy_clearance64(model, pos, qt, qq, margin)
            others = np.delete(cl, i)
            assert abs(cl[i] - (lift - DELTA)) < 2e-6 and (others >= DELTA).all(), (i, flag, cl)
            assert int((cl < 0).any()) == flag
            pair.append(dict(proxy=i, flag=flag, pos=pos, quat=qt, q=qq, clearance=cl))
        found[i] = pair
    return found, missing


def isolating_model(model, proxies):
    """The table in which the given proxies can be isolated by pose: every OTHER proxy's fall_radius at -1 m (1 m clearer than
    shipped); all 16 entries stay, the given ones as shipped -> the fall_radius array of a model override"""
    r = np.array(model["fall_radius"], dtype=np.float64)
    r[[k for k in range(len(r)) if k not in proxies]] = -1.0
    return r


def airborne_case(model, margin, rng):
    """a padding robot: level, 1 m up, flag 0"""
    dirj, offj, _ = pr.joint_maps(model)
    ang = np.zeros(12)
    for mot in range(12):
        ang[int(model["joint_of_motor"][mot])] = model["init_motor_angles"][mot]
    pos, quat, q = f32r([rng.uniform(-1, 1), rng.uniform(-1, 1), 1.0]), f32r(model["init_quat"]), f32r(ang * dirj + offj)
    cl = proxy_clearance64(model, pos, quat, q, margin)
    assert cl.min() > 0.3
    return dict(proxy=-1, flag=0, pos=pos, quat=quat, q=q, clearance=cl)


def mixed_launches(pairs, pad, launches=4):
    """The launches of the isolated-proxy test: each holds every pair, ordered so that consecutive waves of four alternate between
    (hit, clear, hit, clear) and (clear, hit, clear, hit), behind k padding robots in launch k and in front of launches - 1 - k: every
    launch has 2 len(pairs) + launches - 1 robots (a partial last wave), and over the launches a proxy's hit robot sits in every slot."""
    out = []
    for k in range(launches):
        body = []
        for w, i in enumerate(sorted(pairs)):
            hit, clear = pairs[i]
            body += [hit, clear] if (w // 2) % 2 == 0 else [clear, hit]
        out.append([pad] * k + body + [pad] * (launches - 1 - k))
    n = len(out[0])
    assert all(len(l) == n for l in out) and n % 4 != 0
    slots = {}
    for l in out:
        for r, c in enumerate(l):
            if c["flag"]:
                slots.setdefault(c["proxy"], set()).add(r % 4)
    assert all(s == {0, 1, 2, 3} for s in slots.values()), slots
    for l in out:      # every full wave mixes hit and clear robots
        for w in range(len(l) // 4):
            assert len({c["flag"] for c in l[4 * w:4 * w + 4]}) == 2 or all(c["proxy"] < 0 for c in l[4 * w:4 * w + 4])
    return out


def tumbled_cases(model, margin, seed, n=256, band=0.05):
    """n tumbled poses with heights in +-band around first touch -> (cases, decided [n] bool: min |clearance| >= DELTA)"""
    rng = np.random.RandomState(seed)
    quat, q = random_poses(model, rng, n)
    c0 = proxy_clearance_batch(model, np.zeros((n, 3)), quat, q, margin)
    cases = []
    for p in range(n):
        pos = f32r([rng.uniform(-1, 1), rng.uniform(-1, 1), -c0[p].min() + rng.uniform(-band, band)])
        qt, qq = f32r(quat[p]), f32r(q[p])
        cl = proxy_clearance64(model, pos, qt, qq, margin)
        cases.append(dict(proxy=int(np.argmin(cl)), flag=int((cl < 0).any()), pos=pos, quat=qt, q=qq, clearance=cl))
    decided = np.array([np.abs(c["clearance"]).min() >= DELTA for c in cases])
    return cases, decided


def pose_records(base_row, cases):
    """float64 records: base_row with each case's pose, at rest"""
    lay = ol.layout()
    rec = np.repeat(np.asarray(base_row, dtype=np.float64)[None], len(cases), axis=0)
    for i, c in enumerate(cases):
        rec[i, lay.sl("POS")], rec[i, lay.sl("QUAT")], rec[i, lay.sl("Q")] = c["pos"], c["quat"], c["q"]
    for name in ("LINVEL", "ANGVEL", "QD", "LAMBDA"):
        rec[:, lay.sl(name)] = 0.0
    return rec


FALL_DEFECTS = ("body_off_by_one", "no_radius", "lane_xor_1", "ballot_unmasked")


def mimic_fall_wave32(model, margin, wave, pad, defect=None):
    """The device's proxy check for one wave: wave = up to four cases (dicts with pos, quat, q), pad = the case whose pose a padding
    lane group computes (robot 0 of the batch).  One lane per proxy, link poses from the float64 kinematics rounded to float32 (the
    check is mimicked, not the kinematics), the 3-term dot product and the comparison in float32, the robot's flag from the wave's
    ballot shifted by its slot.  Defects: body_off_by_one (the proxy's body index + 1), no_radius, lane_xor_1 (lane i takes its
    radius from lane i ^ 1: a whole row taken from the neighbour only permutes the lanes under the any(), and in the shipped tables
    proxies 2k and 2k + 1 have the same radius, so only the grids on isolating_model's table can see it), ballot_unmasked (the
    shifted ballot not cut to the robot's 16 lanes)."""
    assert 1 <= len(wave) <= 4
    nf = int(model["num_fall_proxies"])
    hit = np.zeros(64, dtype=bool)
    for s in range(4):
        c = wave[s] if s < len(wave) else pad
        bodies, _ = pr.kinematics(model, c["pos"], c["quat"], c["q"])
        for lane in range(16):
            if lane >= nf:
                continue
            b = int(model["fall_body"][lane])
            if defect == "body_off_by_one":
                b = (b + 1) % 13
            Rw, oz = bodies[b]["R"].astype(F32), F32(bodies[b]["o"][2])
            fp = np.asarray(model["fall_pos"][lane], dtype=F32)
            r = F32(0.0) if defect == "no_radius" else F32(model["fall_radius"][lane ^ 1 if defect == "lane_xor_1" else lane])
            wz = Rw[2, 0] * fp[0] + Rw[2, 1] * fp[1] + Rw[2, 2] * fp[2]
            hit[16 * s + lane] = (oz + wz - r) < F32(margin)
    ballot = sum(1 << k for k in range(64) if hit[k])
    mask = (1 << 64) - 1 if defect == "ballot_unmasked" else 0xFFFF
    return [int(((ballot >> (16 * s)) & mask) != 0) for s in range(len(wave))]


def mimic_fall32(model, margin, launch, defect=None):
    out = []
    for w in range(0, len(launch), 4):
        out += mimic_fall_wave32(model, margin, launch[w:w + 4], launch[0], defect)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the termination block: float32 mimic
# ---------------------------------------------------------------------------------------------------------------------------
REASON_DEFECTS = ("pe_without_z", "threshold_not_squared", "ang_without_fabs", "ang_without_wrap", "time_gt_for_ge", "ep_step_without_plus_1",
                  "fall_gate_dropped", "nan_sweep_32_words")


def mimic_reason32(record, cfg, clip, fall, ep_step_before=None, defect=None):
    """The device's block in float32 numpy, from the record after the step (rounded to float32 first); the reward's own non-finite test is
    not part of it (a non-finite state word makes the reward non-finite or leaves it alone, never the other way round)"""
    lay = ol.layout()
    g = lambda name: record[lay.sl(name)]
    rp, p, q = g("REF_POSE").astype(F32), g("POS").astype(F32), g("QUAT").astype(F32)
    thr_d, thr_r = F32(cfg.dist_fail_threshold), F32(cfg.rot_fail_threshold)
    bits = 0
    with np.errstate(all="ignore"):
        pe = F32(0.0)
        for k in range(2 if defect == "pe_without_z" else 3):
            d = rp[k] - p[k]
            pe = pe + d * d
        x1, y1, z1, w1 = rp[3:7]
        x0, y0, z0, w0 = -q[0], -q[1], -q[2], q[3]
        dq = (x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0, -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0,
              x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0, -x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0)
        n = np.sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2])
        ang = F32(2.0) * np.arctan2(n, dq[3])
        two_pi = F32(2.0 * np.pi)
        if defect != "ang_without_wrap" and ang > F32(np.pi):
            ang = (ang - two_pi if ang >= two_pi else ang) - two_pi
        assert all(isinstance(v, F32) for v in (pe, n, ang))
        if (defect == "fall_gate_dropped" or int(g("STEP_COUNTER")[0]) > 0) and fall:
            bits |= CONTACT_FALL
        if pe > (thr_d if defect == "threshold_not_squared" else thr_d * thr_d):
            bits |= ROOT_POS
        if (ang if defect == "ang_without_fabs" else np.abs(ang)) > thr_r:
            bits |= ROOT_ROT
        if not (clip.flags & _abi.CLIP_WRAP) and motion_time64(record, cfg) >= float(clip.duration):     # float64 on the device too (DevClip)
            bits |= MOTION_OVER
        words = record[lay.sl("POS").start:lay.sl("POS").start + (32 if defect == "nan_sweep_32_words" else WORDS)].astype(F32)
        if not bool((np.abs(words) < F32(1e30)).all()):
            bits |= NAN
        before = int(g("EP_STEP")[0]) - 1 if ep_step_before is None else int(ep_step_before)
        ep = before if defect == "ep_step_without_plus_1" else before + 1
        limit = int(g("MAX_EP_STEPS")[0])
        if (ep > limit) if defect == "time_gt_for_ge" else (ep >= limit):
            bits |= TIME_LIMIT
    return bits


# ---------------------------------------------------------------------------------------------------------------------------
# the replay-step grid: one robot per case
# ---------------------------------------------------------------------------------------------------------------------------
INJECTED = (float("nan"), float("inf"), float("-inf"), 2e30)
FINITE_LARGE_WORDS = (1, 8, 20, 31, 36)        # 0.9e30: finite, not a NaN case


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def replay_cases(cfg, seed=11, only_pos=False):
    """The grid of the issue's part 3 for a clip that wraps, in a seeded order that mixes the kinds within waves.  A case: name, pos =
    (unit direction, margin) / rot = (unit axis, relative angle) or None = on the reference, neg_quat, neg_ref, fall, ep = EP_STEP before the
    step relative to MAX_EP_STEPS, inject = (word, value), bits = what the case claims, mask = the bits compared, kind = near / far /
    None per tested quantity."""
    rng = np.random.RandomState(seed)
    thr_d, thr_r = thresholds(cfg)
    cases = []

    def add(name, **kw):
        c = dict(name=name, pos=None, rot=None, neg_quat=False, neg_ref=False, fall=0, ep=None, inject=None, mask=ALL_BITS, near_pos=None, near_rot=None)
        c.update(kw)
        cases.append(c)
    rand_axis = _unit(rng.randn(3))
    # position
    for dname, d in (("x", [1, 0, 0]), ("y", [0, 1, 0]), ("z", [0, 0, 1]), ("diag", [1, 1, 1]), ("unequal", [0.2, -0.55, 0.81])):
        for side in (1, -1):
            add("pos %s %s" % (dname, "inside" if side > 0 else "outside"), pos=(_unit(d), side * NEAR_POS), near_pos=True)
    for side in (1, -1):
        add("pos far %s" % ("inside" if side > 0 else "outside"), pos=(_unit(rng.randn(3)), side * FAR), near_pos=False)
    # rotation
    for aname, ax in (("x", [1, 0, 0]), ("y", [0, 1, 0]), ("z", [0, 0, 1]), ("random", rand_axis)):
        for side in (1, -1):
            for variant in ("", " quat negated", " ref negated"):
                add("rot %s %s%s" % (aname, "inside" if side > 0 else "outside", variant), rot=(_unit(ax), thr_r - side * NEAR_ROT), near_rot=True,
                    neg_quat=variant == " quat negated", neg_ref=variant == " ref negated")
    for side in (1, -1):
        add("rot far %s" % ("inside" if side > 0 else "outside"), rot=(_unit(rng.randn(3)), thr_r - side * FAR), near_rot=False)
    add("rot pi - 0.01", rot=(_unit(rng.randn(3)), np.pi - 0.01), near_rot=False)
    add("rot pi + 0.01 (beyond the wrap)", rot=(_unit(rng.randn(3)), np.pi + 0.01), near_rot=False)
    # fall flag, time limit
    add("fall 1", fall=1)
    add("fall 0", fall=0)
    for k in (-2, -1, 0):
        add("ep_step = max %+d" % k, ep=k)
    # non-finite state: one case per word, the four values rotated over the words
    for w in range(WORDS):
        add("word %d = %r" % (w, INJECTED[w % 4]), inject=(w, INJECTED[w % 4]))
    for w in FINITE_LARGE_WORDS:
        add("word %d = 0.9e30 (finite)" % w, inject=(w, 0.9e30))
    # combinations
    add("pos + rot", pos=(_unit(rng.randn(3)), -FAR), rot=(_unit(rng.randn(3)), thr_r + FAR), near_pos=False, near_rot=False)
    add("fall + time", fall=1, ep=-1)
    add("pos + rot + fall + time", pos=(_unit(rng.randn(3)), -FAR), rot=(_unit(rng.randn(3)), thr_r + FAR), near_pos=False, near_rot=False, fall=1, ep=-1)
    add("nan + time", inject=(17, float("nan")), ep=-1)
    for _ in range(6):
        add("nothing")
    if only_pos:      # the position cases alone, for a configuration whose distance threshold is not 1 (thr^2 != thr)
        cases = [c for c in cases if c["name"].startswith("pos ") or c["name"] == "nothing"][:-1]
    for c in cases:
        c["bits"], c["mask"] = claimed_bits(c, cfg)
    # two robots with an injected word per wave, in slots (w, w + 2) mod 4, until they run out; everybody else in a seeded order
    a = [cases[i] for i in rng.permutation(len(cases)) if cases[i]["inject"] is not None]
    b = [cases[i] for i in rng.permutation(len(cases)) if cases[i]["inject"] is None]
    cases = []
    while a or b:
        w, s = divmod(len(cases), 4)
        cases.append(a.pop() if a and (s in (w % 4, (w + 2) % 4) or not b) else b.pop())
    inj =[i for i, c in enumerate(cases) if c["inject"] is not None and not abs(c["inject"][1]) < 1e30]
    assert only_pos or {i % 4 for i in inj} == {0, 1, 2, 3}
    for i in inj:     # a wave-mate without an injection in every such wave
        assert any(cases[j]["inject"] is None for j in range(4 * (i // 4), min(4 * (i // 4) + 4, len(cases))) if j != i), i
    assert (only_pos or 64 <= len(cases) <= 128) and len(cases) % 4 != 0
    return cases


def motion_over_cases(cfg):
    """The second env's cases, on a clip without wrap: the motion time after the step 1 ms on either side of the clip's duration"""
    out = []
    for name, dt in (("motion 1 ms short", -1e-3), ("motion 1 ms over", 1e-3), ("motion 1 ms short + fall", -1e-3), ("motion 1 ms over + fall", 1e-3),
                     ("motion 1 ms over + time", 1e-3), ("motion 1 ms short ", -1e-3)):
        c = dict(name=name, pos=None, rot=None, neg_quat=False, neg_ref=False, fall=int("fall" in name), ep=-1 if "time" in name else None, inject=None,
                 near_pos=None, near_rot=None, motion=dt)
        c["bits"], c["mask"] = claimed_bits(c, cfg)
        out.append(c)
    return out


def claimed_bits(c, cfg):
    """(bits the case claims, mask of the bits compared).  A non-finite or overflowing word in QUAT leaves the rotation test without a
    margin (float64 gives NaN or an angle that float32 cannot form: 2e30^2 overflows it): ROOT_ROT is left out of the comparison for
    those four words.  In POS every injected value decides `pe > thr^2` alike in both formats: NaN never, +-Inf, 2e30 and 0.9e30 always."""
    thr_d, thr_r = thresholds(cfg)
    bits, mask = 0, ALL_BITS
    if c["fall"]:
        bits |= CONTACT_FALL
    if c["pos"] is not None and c["pos"][1] < 0:
        bits |= ROOT_POS
    if c["rot"] is not None:
        th = c["rot"][1]
        if (th if th <= np.pi else 2.0 * np.pi - th) > thr_r:
            bits |= ROOT_ROT
    if c["ep"] is not None and c["ep"] + 1 >= 0:
        bits |= TIME_LIMIT
    if c.get("motion") is not None and c["motion"] >= 0:
        bits |= MOTION_OVER
    if c["inject"] is not None:
        w, v = c["inject"]
        if not abs(v) < 1e30:
            bits |= NAN
        if w < 3 and not np.isnan(v):
            bits |= ROOT_POS
        if 3 <= w < 7:
            mask &= ~ROOT_ROT
    return bits, mask


def prepare_records(cases, rec, cfg, clip):
    """What a case changes in the record ahead of the step (and of the scouting step, which must see it): EP_STEP, the reference's
    quaternion negated through ORIGIN_ROT (the reference pose is ORIGIN_ROT (x) the clip's; positions rotate the same under -q), the
    motion time through TIME_OFFSET"""
    lay = ol.layout()
    rec = rec.copy()
    for i, c in enumerate(cases):
        if c["ep"] is not None:
            rec[i, lay.sl("EP_STEP")] = rec[i, lay.sl("MAX_EP_STEPS")] + c["ep"]
        if c["neg_ref"]:
            rec[i, lay.sl("ORIGIN_ROT")] = -rec[i, lay.sl("ORIGIN_ROT")]
        if c.get("motion") is not None:
            after = (rec[i, lay.sl("STATE_ACTION_COUNTER")][0] + cfg.action_repeat) * float(ol.dec32(cfg.sim_dt))
            warm = float(ol.dec32(cfg.warmup_time)) if int(rec[i, lay.sl("WARMUP")][0]) else 0.0
            rec[i, lay.sl("TIME_OFFSET")] = f32r(float(clip.duration) + c["motion"] - after + warm)
    return rec


def hold_rows(rec):
    lay = ol.layout()
    return rec[:, lay.sl("POS").start:lay.sl("POS").start + WORDS].copy()


def last_rows(cases, rec, ref_after, cfg):
    """The last row of every robot's traj: the record's own rigid state with POS and QUAT placed relative to ref_after (the REF_POSE of the
    step's end, from the scouting step), rounded to float32, then the injected word"""
    thr_d, _ = thresholds(cfg)
    rows = hold_rows(rec)
    for i, c in enumerate(cases):
        rp = ref_after[i]
        pos, quat = rp[0:3].copy(), rp[3:7].copy()
        if c["pos"] is not None:
            pos = rp[0:3] + c["pos"][0] * (thr_d - c["pos"][1])
        if c["rot"] is not None:
            ax, th = c["rot"]
            dq = np.concatenate([ax * np.sin(0.5 * th), [np.cos(0.5 * th)]])
            quat = pr.qmul(pr.qconj(dq), rp[3:7])          # REF (x) conj(quat) = dq
        if c["neg_quat"]:
            quat = -quat
        rows[i, 0:3], rows[i, 3:7] = pos, quat
    rows = f32r(rows)
    for i, c in enumerate(cases):
        if c["inject"] is not None:
            rows[i, c["inject"][0]] = c["inject"][1]
    return rows


def run_replay_grid(backend, cases, cfg, clip, inject=True):
    """reset records -> the cases' records -> scouting step (the robots held in place) -> the same records again -> the step under test.
    backend: records() -> float64 [n, stride]; set_records(rec); replay_step(traj [n, repeat, 37] float64, fall [n]) -> (done, reward)"""
    lay = ol.layout()
    if not inject:
        cases = [dict(c, inject=None) for c in cases]
    start = prepare_records(cases, backend.records(), cfg, clip)
    hold = np.repeat(hold_rows(start)[:, None, :], cfg.action_repeat, axis=1)
    fall = np.array([c["fall"] for c in cases], dtype=np.uint8)
    backend.set_records(start)
    backend.replay_step(hold, np.zeros_like(fall))
    scout = backend.records()
    if clip.flags & _abi.CLIP_WRAP:     # no phase wrap inside the step: the reference pose does not depend on where the robot is
        assert (scout[:, lay.sl("PREV_PHASE")] > start[:, lay.sl("PREV_PHASE")]).all()
    ref_after = scout[:, lay.sl("REF_POSE")]
    neg = np.array([c["neg_ref"] for c in cases])
    dots = (ref_after[:, 3:7] * start[:, lay.sl("REF_POSE")][:, 3:7]).sum(axis=1)
    assert (dots[neg] < -0.99).all() and (dots[~neg] > 0.99).all(), dots      # the negated reference quaternions are negated, the others not
    traj = hold.copy()
    traj[:, -1, :] = last_rows(cases, start, ref_after, cfg)
    backend.set_records(start)
    done, reward = backend.replay_step(traj, fall)
    return dict(cases=cases, start=start, after=backend.records(), done=np.asarray(done).astype(bool), reward=np.asarray(reward, dtype=np.float64),
                traj=traj, fall=fall, ref_after=ref_after)


def expected_of_grid(run, cfg, clip):
    """reason64 on every robot's record after the step -> (bits [n], mask [n], nearest margin used, cases with a bit left out); asserts
    that every case is what it claims to be: its bits, and its margins in the band of a near or a far case"""
    lay = ol.layout()
    bound_p, bound_r = pos_bound(thresholds(cfg)[0]), ang_bound()
    bits, masks, nearest = [], [], np.inf
    for i, c in enumerate(run["cases"]):
        rec = run["after"][i].copy()
        rec[lay.sl("POS").start:lay.sl("POS").start + WORDS] = run["traj"][i, -1]     # POS and QUAT are the inputs, bit for bit
        b, m = reason64(rec, cfg, clip, int(run["fall"][i]), ep_step_before=int(run["start"][i, lay.sl("EP_STEP")][0]))
        assert (b & c["mask"]) == (c["bits"] & c["mask"]), (c["name"], b, c["bits"], m)
        if c["inject"] is None or c["inject"][0] >= 7:
            for key, near, bound, target in (("pos", c["near_pos"], bound_p, NEAR_POS), ("rot", c["near_rot"], bound_r, NEAR_ROT)):
                if near is True:
                    assert 16.0 * bound <= abs(m[key]) <= NEAR_MAX, (c["name"], key, m[key])
                    nearest = min(nearest, abs(m[key]))
                elif near is False:
                    assert abs(m[key]) >= 0.3, (c["name"], key, m[key])
                else:
                    assert m[key] >= 0.3, (c["name"], key, m[key])       # an untested quantity is on its reference
        if c.get("motion") is not None:
            assert 0.9e-3 < abs(m["motion"]) < 1.1e-3 and (m["motion"] <= 0) == (c["motion"] >= 0)
        bits.append(b)
        masks.append(c["mask"])
    left_out = sum(1 for c in run["cases"] if c["mask"] != ALL_BITS)
    return np.array(bits), np.array(masks), float(nearest), left_out


def histogram(bits):
    return {name: int(((np.asarray(bits) & bit) != 0).sum()) for bit, name in BIT_NAMES}


def report(group, cases, nearest, bound, left_out):
    """the line every GPU test prints (kept in profiles/termination.txt)"""
    line = "TERMINATION %s cases=%d nearest=%.3g bound=%.3g left_out=%d" % (group, cases, nearest, bound, left_out)
    print("\n" + line)
    return line


class OracleReplay(object):
    """run_replay_grid's backend on the float64 oracle (orc_set_replay, one robot at a time, as tests/test_oracle_golden_task.py drives it)"""

    def __init__(self, cfg, models, clip, n, robot_type, uniforms):
        import ctypes as C
        self.C = C
        self.orc = ol.OracleEnv(cfg, models, [clip], n, robot_type=robot_type, clip_id=0)
        L = self.L = self.orc.L
        L.orc_set_replay.argtypes = [C.c_void_p, C.c_int, ol.dp, ol.dp, ol.dp, ol.dp, C.c_int, ol.dp]
        L.orc_set_margins_out.argtypes = [C.c_void_p, ol.dp]
        self.n = n
        self.margins = np.zeros((n, 3))
        for i in range(n):
            uni = np.ascontiguousarray(uniforms[i], dtype=np.float64)
            L.orc_set_replay(self.orc.h, 1, None, None, None, None, 0, ol.P(uni))
            L.orc_reset(self.orc.h, ol.P(self.orc.state[i:i + 1]), 1, None, None)
        L.orc_set_replay(self.orc.h, 0, None, None, None, None, 0, None)

    def records(self):
        return self.orc.state.copy()

    def set_records(self, rec):
        self.orc.state[:] = rec

    def replay_step(self, traj, fall):
        C, L, orc = self.C, self.L, self.orc
        done, rew = np.zeros(self.n, dtype=np.uint8), np.zeros(self.n)
        act, obs, tau = np.zeros((1, 12)), np.zeros((1, _abi.OBS_DIM)), np.zeros((orc.cfg.action_repeat, 12))
        for i in range(self.n):
            tr = np.ascontiguousarray(traj[i], dtype=np.float64)
            one = np.zeros(3)
            L.orc_set_margins_out(orc.h, ol.P(one))
            L.orc_set_replay(orc.h, 1, ol.P(tr), ol.P(tau), None, None, int(fall[i]), None)
            L.orc_step(orc.h, ol.P(orc.state[i:i + 1]), 1, ol.P(act), ol.P(obs), ol.P(rew[i:i + 1]), done[i:i + 1].ctypes.data_as(C.c_void_p), None)
            self.margins[i] = one
        L.orc_set_replay(orc.h, 0, None, None, None, None, 0, None)
        L.orc_set_margins_out(orc.h, None)
        return done.astype(bool), rew

    def close(self):
        self.orc.close()


def replay_uniforms(n, seed=3):
    """The draws of the replay reset: reference state initialisation for everybody (draw 26 = 0), the time offset (draw 27) between 0.1
    and 0.6 of the clip: no phase wrap within a step"""
    rng = np.random.RandomState(seed)
    uni = rng.uniform(0.0, 1.0, (n, 28)).astype(F32)
    uni[:, 26] = 0.0
    uni[:, 27] = rng.uniform(0.1, 0.6, n).astype(F32)
    return uni
