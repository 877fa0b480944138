"""Float64 reference of ONE orr_shaped_reward call (include/openroborl_hip.h), the counted float32 error bound of every output, the
comparison the GPU tests and the CPU tests share, a float32 numpy mimic of the kernel with seeded defects, and the edge grid's inputs.

A call's inputs, `inp`, a dict of numpy arrays as the device holds them (float32 unless noted):
  act [N, 12, 4] | None (no actuator outputs bound), contact [N, 4, 4] | None, actions [N, 12], prev [N, 24], reward [N], done [N] uint8,
  ep_step, last_len, reason [N] int32 (the record's EP_STEP, LAST_EP_LEN, DONE_REASON), ep [N, 8], tot [N, 8] (the two sum buffers before
  the call), w [6], floor, inv_nsub, inv_dt (float32 scalars, the host's 1 / action_repeat and 1 / sim_dt).
Its outputs, `out`: row [N, 8], ep [N, 8], tot [N, 8], prev [N, 24], reward [N].

The bounds, EPS = 2^-24 (one float32 rounding is a relative error of at most EPS), first order with the slack the counts carry:
  a sum of n non-negative values with at most one scaling (torque, work, impact): n - 1 adds and one multiply, (n + 2) EPS value
  action_rate: every element is one subtraction and one square, 3 EPS of it, then the 12-element sum: (12 + 2 + 3) EPS value
  action_accel: d = a - 2 a1 + a2 cancels, so its error is absolute: |dd| <= 2 EPS (|a| + 2 |a1| + |a2|) =: e (2 a1 is exact, two adds);
      the square then is off by 2 |d| e + e^2, its own rounding and the sum add (12 + 2 + 1) EPS sum (|d| + e)^2
  failure and column 7 are selects: exact
  pen: six fused multiply-adds, 7 EPS sum |w p| with p at its upper bound, plus the terms' own bounds times w
  shaped = fmax(r - pen, floor): fmax is 1-Lipschitz, so pen's bound plus the subtraction's EPS |r - pen|
  an episode row that is added to: the step row's bound plus EPS |new value|; the totals likewise from the episode row's
Nothing here is tuned on device output."""
import numpy as np

EPS = 2.0 ** -24
NAMES = ("torque", "work", "action_rate", "action_accel", "impact", "failure")
CONTACT_FALL, ROOT_POS, ROOT_ROT, TIME_LIMIT, NAN, MOTION_OVER = 1, 2, 4, 8, 16, 32
FAIL_BITS = CONTACT_FALL | ROOT_POS | ROOT_ROT | NAN
# the edge grid: the step's number within its episode x done x the done reason (every bit alone, a time limit together with a fall)
GRID_STEPS = (0, 1, 2, 3, 17)
GRID_REASONS = (CONTACT_FALL, ROOT_POS, ROOT_ROT, TIME_LIMIT, NAN, MOTION_OVER, TIME_LIMIT | CONTACT_FALL)
GRID = [(s, d, r) for s in GRID_STEPS for d in (0, 1) for r in GRID_REASONS]
WEIGHTS = (1e-5, 0.05, 0.01, 0.005, 0.002, 0.7)          # penalties of the order of the reward with the magnitudes edge_inputs draws
DEFECTS = ("n_step_from_ep_step", "time_limit_fails", "work_signed", "prev_not_shifted", "floor_ignored", "nan_not_zeroed", "ep_added_at_1")


def host_scales(action_repeat=33, sim_dt=0.001):
    """(inv_nsub, inv_dt) as the C side forms them: float32 divisions of 1 by the float32 values"""
    return np.float32(1.0) / np.float32(action_repeat), np.float32(1.0) / np.float32(sim_dt)


def rounds(n):
    """how many calls of n robots walk the whole grid"""
    return -(-len(GRID) // n)


def edge_inputs(n, rnd, seed=0, action_repeat=33, sim_dt=0.001, bound=(True, True)):
    """The inputs of call `rnd` of the edge grid for n robots: robot i takes grid cell (rnd n + i) mod |GRID|; every buffer is filled
    from a seeded generator (the sum buffers and prev with values that a wrong overwrite / add / shift shows against), a NaN step has
    non-zero buffers and non-finite actions, the work column has both signs, and the floor lies a quarter above (even calls) or below
    (odd calls) robot 0's unfloored shaped reward, so that across robots and calls it cuts on both sides."""
    rng = np.random.default_rng([seed, n, rnd])
    f32 = np.float32
    cell = [GRID[(rnd * n + i) % len(GRID)] for i in range(n)]
    n_step = np.array([c[0] for c in cell], dtype=np.int32)
    done = np.array([c[1] for c in cell], dtype=np.uint8)
    reason = np.array([c[2] for c in cell], dtype=np.int32)
    decoy = np.where(n_step >= 2, 0, 5).astype(np.int32)          # what the OTHER counter holds: on the other side of every threshold
    act = np.zeros((n, 12, 4), dtype=f32)
    act[:, :, 0] = rng.normal(0.0, 60.0, (n, 12))
    act[:, :, 1] = rng.uniform(0.0, 30.0, (n, 12))
    act[:, :, 2] = rng.uniform(0.0, 3.0e4, (n, 12))
    act[:, :, 3] = rng.normal(0.0, 0.5, (n, 12))
    contact = rng.uniform(0.0, 0.6, (n, 4, 4)).astype(f32)
    contact[:, :, 3] = rng.uniform(0.0, 0.08, (n, 4))
    contact[rng.random((n, 4)) < 0.3] = 0.0                        # legs in the air
    actions = rng.uniform(-2 * np.pi, 2 * np.pi, (n, 12)).astype(f32)
    prev = (np.tile(actions, (1, 2)) + rng.normal(0.0, 0.3, (n, 24))).astype(f32)
    nan_rows = np.nonzero(reason & NAN)[0]
    for k, i in enumerate(nan_rows):
        actions[i, k % 12] = (np.nan, np.inf, -np.inf)[k % 3]
    inv_nsub, inv_dt = host_scales(action_repeat, sim_dt)
    inp = dict(act=act if bound[0] else None, contact=contact if bound[1] else None, actions=actions, prev=prev,
               reward=rng.uniform(0.0, 1.0, n).astype(f32), done=done, ep_step=np.where(done != 0, decoy, n_step).astype(np.int32),
               last_len=np.where(done != 0, n_step, decoy).astype(np.int32), reason=reason,
               ep=rng.uniform(1.0, 50.0, (n, 8)).astype(f32), tot=rng.uniform(100.0, 900.0, (n, 8)).astype(f32),
               w=np.array(WEIGHTS, dtype=f32), floor=f32(-np.inf), inv_nsub=inv_nsub, inv_dt=inv_dt)
    free = reference(inp)["row"][0, 6]
    inp["floor"] = f32(free + (0.25 if rnd % 2 == 0 else -0.25))
    return inp


def _n_step(inp):
    return np.where(inp["done"] != 0, inp["last_len"], inp["ep_step"]).astype(np.int64)


def reference(inp):
    """-> dict of float64 arrays: row, ep, tot, reward and their bounds row_b, ep_b, tot_b, reward_b; prev (float32, exact);
    pen, pen_b [N]"""
    n = len(inp["reward"])
    a = inp["actions"].astype(np.float64)
    a1, a2 = inp["prev"][:, :12].astype(np.float64), inp["prev"][:, 12:].astype(np.float64)
    d = inp["done"] != 0
    reason = inp["reason"].astype(np.int64)
    n_step = _n_step(inp)
    nan_step = (reason & NAN) != 0
    p = np.zeros((n, 8))
    b = np.zeros((n, 8))
    if inp["act"] is not None:
        A = inp["act"].astype(np.float64)
        p[:, 0] = A[:, :, 2].sum(1) * float(inp["inv_nsub"])
        b[:, 0] = (12 + 2) * EPS * np.abs(A[:, :, 2]).sum(1) * float(inp["inv_nsub"])
        p[:, 1] = np.abs(A[:, :, 3]).sum(1)
        b[:, 1] = (12 + 2) * EPS * p[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        d1 = a - a1
        p[:, 2] = np.where(n_step >= 2, (d1 * d1).sum(1), 0.0)
        b[:, 2] = (12 + 2 + 3) * EPS * p[:, 2]
        d2 = a - 2.0 * a1 + a2
        e = 2.0 * EPS * (np.abs(a) + 2.0 * np.abs(a1) + np.abs(a2))
        p[:, 3] = np.where(n_step >= 3, (d2 * d2).sum(1), 0.0)
        b[:, 3] = np.where(n_step >= 3, (2.0 * np.abs(d2) * e + e * e).sum(1) + (12 + 2 + 1) * EPS * ((np.abs(d2) + e) ** 2).sum(1), 0.0)
    if inp["contact"] is not None:
        C = inp["contact"].astype(np.float64)
        p[:, 4] = C[:, :, 3].sum(1) * float(inp["inv_dt"])
        b[:, 4] = (4 + 2) * EPS * np.abs(C[:, :, 3]).sum(1) * float(inp["inv_dt"])
    p[nan_step, :5] = 0.0
    b[nan_step, :5] = 0.0
    p[:, 5] = (d & ((reason & FAIL_BITS) != 0)).astype(np.float64)
    w = inp["w"].astype(np.float64)
    pen = (p[:, :6] * w).sum(1)
    pen_b = 7.0 * EPS * ((np.abs(p[:, :6]) + b[:, :6]) * w).sum(1) + (b[:, :6] * w).sum(1)
    r = inp["reward"].astype(np.float64)
    p[:, 6] = np.maximum(r - pen, float(inp["floor"]))
    b[:, 6] = pen_b + EPS * (np.abs(r - pen) + pen_b)
    p[:, 7] = 1.0
    over = (n_step <= 1)[:, None]
    ep = np.where(over, p, inp["ep"].astype(np.float64) + p)
    ep_b = np.where(over, b, b + EPS * (np.abs(ep) + b))
    tot_old = inp["tot"].astype(np.float64)
    tot = np.where(d[:, None], tot_old + ep, tot_old)
    tot_b = np.where(d[:, None], ep_b + EPS * (np.abs(tot) + ep_b), 0.0)
    prev = np.concatenate([inp["actions"], inp["prev"][:, :12]], axis=1).astype(np.float32)
    return dict(row=p, row_b=b, ep=ep, ep_b=ep_b, tot=tot, tot_b=tot_b, prev=prev, reward=p[:, 6].copy(), reward_b=b[:, 6].copy(), pen=pen, pen_b=pen_b)


def _fma(x, y, z):
    """float32 fused multiply-add: the product of two float32 is exact in float64, one float64 add, one rounding to float32 (a double
    rounding in rare ties: the mimic is held to the bounds, not to the device's bits)"""
    return np.float32(np.float64(x) * np.float64(y) + np.float64(z))


def mimic(inp, defect=None):
    """The kernel in float32 numpy, robot by robot, with one of DEFECTS seeded in (None: clean) -> out"""
    assert defect is None or defect in DEFECTS, defect
    f32 = np.float32
    n = len(inp["reward"])
    out = dict(row=np.zeros((n, 8), f32), ep=inp["ep"].copy(), tot=inp["tot"].copy(), prev=np.zeros((n, 24), f32), reward=np.zeros(n, f32))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            d = inp["done"][i] != 0
            reason = int(inp["reason"][i])
            n_step = int(inp["last_len"][i] if d and defect != "n_step_from_ep_step" else inp["ep_step"][i])
            nan_step = bool(reason & NAN) and defect != "nan_not_zeroed"
            a, a1, a2 = inp["actions"][i], inp["prev"][i, :12], inp["prev"][i, 12:]
            s_tau = s_work = s_rate = s_accel = s_peak = f32(0.0)
            for m in range(12):
                if inp["act"] is not None:
                    s_tau = f32(s_tau + inp["act"][i, m, 2])
                    s_work = f32(s_work + (inp["act"][i, m, 3] if defect == "work_signed" else abs(inp["act"][i, m, 3])))
                d1 = f32(a[m] - a1[m])
                d2 = f32(f32(a[m] - f32(2.0) * a1[m]) + a2[m])
                s_rate = f32(s_rate + f32(d1 * d1))
                s_accel = f32(s_accel + f32(d2 * d2))
            if inp["contact"] is not None:
                for leg in range(4):
                    s_peak = f32(s_peak + inp["contact"][i, leg, 3])
            fail_bits = FAIL_BITS | (TIME_LIMIT if defect == "time_limit_fails" else 0)
            p = [f32(0.0) if nan_step else f32(s_tau * inp["inv_nsub"]), f32(0.0) if nan_step else s_work,
                 f32(0.0) if nan_step or n_step < 2 else s_rate, f32(0.0) if nan_step or n_step < 3 else s_accel,
                 f32(0.0) if nan_step else f32(s_peak * inp["inv_dt"]), f32(1.0) if d and reason & fail_bits else f32(0.0)]
            pen = f32(0.0)
            for k in range(6):
                pen = _fma(inp["w"][k], p[k], pen)
            shaped = f32(inp["reward"][i] - pen)
            if defect != "floor_ignored":
                shaped = max(shaped, f32(inp["floor"]))
            row = np.array(p + [shaped, f32(1.0)], dtype=f32)
            out["row"][i] = row
            out["ep"][i] = row if n_step <= (0 if defect == "ep_added_at_1" else 1) else inp["ep"][i] + row
            if d:
                out["tot"][i] = inp["tot"][i] + out["ep"][i]
            out["prev"][i] = np.concatenate([a, a2 if defect == "prev_not_shifted" else a1])
            out["reward"][i] = shaped
    return out


def _within(got, want, bound):
    """elementwise |got - want| <= bound, False for anything non-finite in got"""
    with np.errstate(invalid="ignore"):
        return np.abs(got.astype(np.float64) - want) <= bound


def check(inp, out, ref=None, what=""):
    """The comparison of one call: every output within its counted bound of the float64 reference, and bit for bit what is a copy, a
    select or one float32 add of stored values.  AssertionError names the first output that misses; -> {output: largest error / bound}."""
    ref = ref or reference(inp)
    f32 = np.float32
    worst = {}
    for key in ("row", "ep", "tot", "reward"):
        ok = _within(out[key], ref[key], ref[key + "_b"])
        if not ok.all():
            i = tuple(np.argwhere(~ok)[0])
            raise AssertionError("%s%s%s: got %r, float64 %r, bound %.3g" % (what, key, list(i), out[key][i], ref[key][i], ref[key + "_b"][i]))
        err, bnd = np.abs(out[key].astype(np.float64) - ref[key]), ref[key + "_b"]
        worst[key] = float(np.max(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), 0.0)))
    # copies and selects
    assert out["prev"].tobytes() == ref["prev"].tobytes(), what + "prev is not {a, a1} bit for bit"
    assert out["row"][:, 5].tobytes() == ref["row"][:, 5].astype(f32).tobytes(), what + "the failure term"
    assert out["row"][:, 7].tobytes() == np.ones(len(out["row"]), f32).tobytes(), what + "column 7 is not 1.0"
    assert out["reward"].tobytes() == out["row"][:, 6].tobytes(), what + "reward_out is not the stored shaped reward"
    # the shaped reward from the very term values stored
    row64, w = out["row"].astype(np.float64), inp["w"].astype(np.float64)
    pen = (row64[:, :6] * w).sum(1)
    diff = inp["reward"].astype(np.float64) - pen
    ok = _within(out["row"][:, 6], np.maximum(diff, float(inp["floor"])), EPS * np.abs(diff) + 7.0 * EPS * (np.abs(row64[:, :6]) * w).sum(1))
    assert ok.all(), what + "shaped reward of robot %d is not fmax(r - sum w p, floor) of the stored terms" % int(np.argwhere(~ok)[0, 0])
    # overwrite versus add of the episode row, and the totals, in float32 from the stored rows
    over = (_n_step(inp) <= 1)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        ep_want = np.where(over, out["row"], inp["ep"] + out["row"]).astype(f32)
        tot_want = np.where((inp["done"] != 0)[:, None], inp["tot"] + out["ep"], inp["tot"]).astype(f32)
    assert out["ep"].tobytes() == ep_want.tobytes(), what + "the episode row is not the stored row (n_step <= 1) / one add of it"
    assert out["tot"].tobytes() == tot_want.tobytes(), what + "the totals are not one add of the new episode row where done, untouched elsewhere"
    return worst
