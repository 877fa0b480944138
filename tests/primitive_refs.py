"""References and input generators of the device-primitive tests (test infrastructure).

tests/test_gpu_device_primitives.py runs every device helper of the env kernels through the probe (tests/probe_lib.py) and compares
it with the definitions below; tests/test_device_probe_cpu.py checks, without a GPU, that the vectorised references agree with
brute-force per-lane definitions and the oracle's own functions, and that every input generator fills the buckets it names.

Lane layout of the cross-lane helpers: record i sits in lane i & 15 of robot i >> 4; inside a robot lane = leg + 4 * part.
Generators are deterministic (fixed seeds) and return float32 arrays; "buckets" are {name: boolean mask over the records}.
"""
import numpy as np

F32 = np.float32
PI_F = F32(np.pi)
EPS24 = 2.0 ** -24
MIN_BUCKET = 1000


def next_floats(x, k):
    """The 2 k + 1 float32 values around x: x and its k neighbours on each side."""
    x = F32(x)
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo = np.nextafter(lo, F32(-np.inf), dtype=F32)
        hi = np.nextafter(hi, F32(np.inf), dtype=F32)
        out += [lo, hi]
    return np.array(sorted(out), dtype=F32)


def circ(a, b):
    """circular distance of two angles"""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


# =====================================================================================================================
# A. lane movement
# =====================================================================================================================
def lanes(x):
    """[n, ...] -> [robots, part, leg, ...]"""
    x = np.asarray(x)
    return x.reshape((-1, 4, 4) + x.shape[1:])


def wave_inputs(n, width, seed, kind="random"):
    """[n, width] float32, different in every lane and robot.  kind: "random" (normal, scales over three decades), "dyadic"
    (multiples of 2^-6, |.| < 16, i.e. 10-bit integers / 64: a product has 20 bits and a sum of six products 23, so every product and
    sum of the helpers is exact in float32; the same on a 2^-8 grid would need 26 bits for a sum of three products), "int" (small
    integers)."""
    rng = np.random.RandomState(seed)
    if kind == "int":
        x = rng.randint(-512, 513, size=(n, width)).astype(F32)
    elif kind == "dyadic":
        x = (rng.randint(-1023, 1024, size=(n, width)) / 64.0).astype(F32)
    else:
        x = (rng.standard_normal((n, width)) * 10.0 ** rng.uniform(-2, 1, size=(n, 1))).astype(F32)
    return x


def row_sum_ref64(x):
    """float64 sum over each robot's 16 lanes, in every lane; and the sum of |x|"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 16)
    s = np.repeat(x.sum(axis=1), 16)
    sa = np.repeat(np.abs(x).sum(axis=1), 16)
    return s, sa


def bcast_ref(x, lanes_r):
    """out[i, j] = x in lane lanes_r[j] of record i's robot"""
    x = np.asarray(x).reshape(-1, 16)
    return np.repeat(x[:, list(lanes_r)], 16, axis=0)


def suffix_sum_ref(x):
    """part_suffix_sum in float32: part 0 = (x0 + x1) + x2, part 1 = x1 + x2, part 2 = x2, part 3 = x3 (x[n] or x[n, k])"""
    X = lanes(np.asarray(x, dtype=F32))
    out = np.empty_like(X)
    out[:, 0] = (X[:, 0] + X[:, 1]) + X[:, 2]
    out[:, 1] = X[:, 1] + X[:, 2]
    out[:, 2] = X[:, 2]
    out[:, 3] = X[:, 3]
    return out.reshape(np.asarray(x).shape)


def first_moment_inputs(n, seed, kind):
    """records (m, c[3], h[3]) with h = the lane's own rounded m c"""
    v = wave_inputs(n, 4, seed, kind)
    if kind == "random":
        v[:, 0] = np.abs(v[:, 0]) + F32(0.01)     # a mass
    h = (v[:, :1] * v[:, 1:4]).astype(F32)
    return np.concatenate([v, h], axis=1)


def first_moment_ref64(rec):
    """t = m c + h[part + 1] + h[part + 2] in float64 (the other lanes' ROUNDED h; parts beyond 2 are no source), and the largest
    partial sum's magnitude"""
    R = lanes(np.asarray(rec, dtype=np.float64))
    own = R[..., 0:1] * R[..., 1:4]
    h = R[..., 4:7]
    z = np.zeros_like(h[:, 0])
    h1 = np.stack([h[:, 1], h[:, 2], z, z], axis=1)
    h2 = np.stack([h[:, 2], z, z, z], axis=1)
    p1 = own + h1
    t = p1 + h2
    scale = np.max(np.abs(np.stack([own, h1, h2, p1, t])), axis=0)
    return t.reshape(-1, 3), scale.reshape(-1, 3)


def triplet_ref64(rec):
    """dpp_contact_triplet<4 + g>, g = 0..3 -> [n, 12] and the sum of the terms' magnitudes: t = wa_lin + wa_ang x rr + sum_k ck[k] wq[k],
    rr / ck from lane 4 + g of the robot, wa / wq from the own lane"""
    r = np.asarray(rec, dtype=np.float64)
    n = len(r)
    R = r.reshape(-1, 16, 21)
    wa, wq = r[:, 12:18], r[:, 18:21]
    out, mag = np.empty((n, 12)), np.empty((n, 12))
    for g in range(4):
        src = np.repeat(R[:, 4 + g], 16, axis=0)
        rr, ck = src[:, 0:3], src[:, 3:12].reshape(n, 3, 3)       # ck[k] = (c_k0, c_k1, c_k2)
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            terms = np.stack([wa[:, 3 + i], wa[:, j] * rr[:, k], -wa[:, k] * rr[:, j],
                              ck[:, 0, i] * wq[:, 0], ck[:, 1, i] * wq[:, 1], ck[:, 2, i] * wq[:, 2]])
            out[:, 3 * g + i] = terms.sum(axis=0)
            mag[:, 3 * g + i] = np.abs(terms).sum(axis=0)
    return out, mag


# =====================================================================================================================
# B. math: float64 definitions (ref64_*) and the same formulas in float32 (the floor)
# =====================================================================================================================
def _qmul(a, b):
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x0, y0, z0, w0 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([x1 * w0 + y1 * z0 - z1 * y0 + w1 * x0, -x1 * z0 + y1 * w0 + z1 * x0 + w1 * y0,
                     x1 * y0 - y1 * x0 + z1 * w0 + w1 * z0, -x1 * x0 - y1 * y0 - z1 * z0 + w1 * w0], axis=-1)


def qrot_def(p, q, dt=np.float64):
    """pose3d.QuaternionRotatePoint: q [p, 0] q^-1, q^-1 = conjugate / |q|^2"""
    p, q = np.asarray(p, dtype=dt), np.asarray(q, dtype=dt)
    qp = np.concatenate([p, np.zeros_like(p[..., :1])], axis=-1)
    qi = q * np.array([-1, -1, -1, 1], dtype=dt) / (q * q).sum(axis=-1, keepdims=True)
    return _qmul(_qmul(q, qp), qi)[..., :3]


def heading_def(q, dt=np.float64):
    q = np.asarray(q, dtype=dt)
    x = np.zeros(q.shape[:-1] + (3,), dtype=dt)
    x[..., 0] = 1
    r = qrot_def(x, q, dt)
    return np.arctan2(r[..., 1], r[..., 0])


def euler_def(q, dt=np.float64):
    """pybullet.getEulerFromQuaternion (the oracle's orc_euler_from_quat)"""
    q = np.asarray(q, dtype=dt)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    sqx, sqy, sqz, sqw = x * x, y * y, z * z, w * w
    sarg = dt(-2.0) * (x * z - w * y)
    roll = np.arctan2(dt(2) * (y * z + w * x), -sqx - sqy + sqz + sqw)
    pitch = np.arcsin(np.clip(sarg, dt(-1), dt(1)))
    yaw = np.arctan2(dt(2) * (x * y + w * z), sqx - sqy - sqz + sqw)
    return np.stack([roll, pitch, yaw], axis=-1)


def euler_sarg64(q):
    q = np.asarray(q, dtype=np.float64)
    return -2.0 * (q[..., 0] * q[..., 2] - q[..., 3] * q[..., 1])


def norm_angle_def(q, dt=np.float64):
    """QuaternionToAxisAngle's angle + normalize_rotation_angle (orc_axis_angle, orc_normalize_angle)"""
    q = np.asarray(q, dtype=dt)
    n = np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2])
    t = dt(2.0) * np.arctan2(n, q[..., 3])
    pi = dt(np.pi)
    m = np.fmod(t, dt(2) * pi)
    m = np.where(m >= 0, m - dt(2) * pi, m + dt(2) * pi)
    return np.where(np.abs(t) > pi, m, t)


def map_pi_def(a):
    """orc_map_pi"""
    a = np.asarray(a, dtype=np.float64)
    m = np.fmod(a, 2 * np.pi)
    return np.where(m >= np.pi, m - 2 * np.pi, np.where(m < -np.pi, m + 2 * np.pi, m))


def q_to_mat_def(q, dt=np.float64):
    q = np.asarray(q, dtype=dt)
    q = q / np.sqrt((q * q).sum(axis=-1, keepdims=True))
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two = dt(2)
    return np.stack([1 - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w),
                     two * (x * y + z * w), 1 - two * (x * x + z * z), two * (y * z - x * w),
                     two * (x * z - y * w), two * (y * z + x * w), 1 - two * (x * x + y * y)], axis=-1)


def slerp_def(a, b, f):
    """transformations.quaternion_slerp (shortest path), float64, vectorised; also returns the dot product of the unit ends"""
    eps = np.finfo(float).eps * 4.0
    a, b, f = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(f, dtype=np.float64)
    q0 = a / np.sqrt((a * a).sum(axis=-1, keepdims=True))
    q1 = b / np.sqrt((b * b).sum(axis=-1, keepdims=True))
    d = (q0 * q1).sum(axis=-1)
    same = np.abs(np.abs(d) - 1.0) < eps
    sg = np.where(d < 0, -1.0, 1.0)
    ang = np.arccos(np.minimum(np.abs(d), 1.0))
    same |= np.abs(ang) < eps
    with np.errstate(divide="ignore", invalid="ignore"):
        isin = 1.0 / np.sin(ang)
        s0 = np.sin((1.0 - f) * ang) * isin
        s1 = np.sin(f * ang) * isin * sg
    s0 = np.where(f == 0, 1.0, np.where(f == 1, 0.0, np.where(same, 1.0, s0)))
    s1 = np.where(f == 0, 0.0, np.where(f == 1, 1.0, np.where(same, 0.0, s1)))
    return q0 * s0[..., None] + q1 * s1[..., None], d


# ---- input generators -----------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def quat_from_euler64(r, p, y):
    """pybullet.getQuaternionFromEuler"""
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy], axis=-1)


PITCH_EDGES = (0.0, 0.9, 0.999, 0.99999)


def pitch_buckets(s):
    """buckets of |sin pitch| (or of |x| for asin)"""
    s = np.abs(np.asarray(s, dtype=np.float64))
    return {"[0,0.9)": s < 0.9, "[0.9,0.999)": (s >= 0.9) & (s < 0.999), "[0.999,0.99999)": (s >= 0.999) & (s < 0.99999),
            "[0.99999,1]": (s >= 0.99999) & (s <= 1.0), "clamped": s > 1.0}


def gen_sincos():
    grid = np.linspace(-100.0, 100.0, 400001).astype(F32)
    edges = np.concatenate([next_floats(k * (np.pi / 2), 4) for k in range(-64, 65)])
    return np.concatenate([grid, edges, np.array([0.0, -0.0, 1e-30, -1e-30], dtype=F32)])


def gen_atan2():
    """(y, x) pairs and {bucket: mask}"""
    rng = np.random.RandomState(11)
    parts, names = [], []

    def add(name, y, x):
        parts.append(np.stack([np.asarray(y, dtype=F32), np.asarray(x, dtype=F32)], axis=1))
        names.append(name)
    lo, hi = np.log(4 * 2.0 ** -126), np.log(1e30)
    mags = np.exp(np.linspace(lo, hi, 48))
    gy, gx = np.meshgrid(mags, mags, indexing="ij")
    for sy in (1, -1):
        for sx in (1, -1):
            add("log_grid", sy * gy.ravel(), sx * gx.ravel())
    m = 100000
    add("log_random", np.exp(rng.uniform(lo, hi, m)) * rng.choice([-1, 1], m), np.exp(rng.uniform(lo, hi, m)) * rng.choice([-1, 1], m))
    th = rng.uniform(-np.pi, np.pi, 300000)
    r = 10.0 ** rng.uniform(-3, 3, len(th))
    add("angles", r * np.sin(th), r * np.cos(th))
    ax = np.exp(np.linspace(lo, hi, 500))
    z = np.zeros_like(ax)
    add("axes", np.concatenate([z, -z, ax, -ax, z, -z]), np.concatenate([ax, ax, z, -z, -ax, -ax]))
    dg = np.exp(rng.uniform(lo, hi, 2000)).astype(F32)
    add("diagonal", np.concatenate([dg, dg, -dg, -dg]), np.concatenate([dg, -dg, dg, -dg]))
    t = next_floats(0.41421356237, 8)
    ys, xs = [], []
    for scale in [2.0 ** k for k in (-40, -20, -10, -3, 0, 1, 7, 20, 40)]:   # powers of two: t = mn / mx stays the same float
        for sy in (1, -1):
            for sx in (1, -1):
                ys += [sy * t * F32(scale), sx * np.full_like(t, scale)]
                xs += [sx * np.full_like(t, scale), sy * t * F32(scale)]
    add("switch", np.concatenate(ys), np.concatenate(xs))
    x = np.concatenate(parts)
    masks, at = {}, 0
    for name, p in zip(names, parts):
        mk = np.zeros(len(x), dtype=bool)
        mk[at:at + len(p)] = True
        masks[name] = masks.get(name, np.zeros(len(x), dtype=bool)) | mk
        at += len(p)
    return x, masks


ATAN2_EXACT = [((0.0, -0.0), np.pi), ((-0.0, -1.0), -np.pi), ((0.0, 0.0), 0.0)]
ATAN2_SUBNORMAL = [(0.0, 1e-40), (1e-40, 1e-40), (1.0, 1e-40), (1e-40, 1.0), (-1e-40, 3e-39), (2e-39, -1e-40), (0.0, -1e-40),
                   (1e-45, 1e-45), (-1.0, -1e-40), (1e-40, 0.0)]


def flush_subnormals(x):
    x = np.asarray(x, dtype=F32)
    return np.where(np.abs(x) < np.finfo(F32).tiny, np.copysign(F32(0), x), x).astype(F32)


def gen_map_pi():
    rng = np.random.RandomState(12)
    u = rng.uniform(-1000.0, 1000.0, 400000).astype(F32)
    near = np.concatenate([next_floats(s * k * 2 * np.pi, 4) for k in range(0, 160) for s in (1, -1)] +
                          [next_floats(s * (2 * k + 1) * np.pi, 4) for k in range(0, 159) for s in (1, -1)])
    small = rng.uniform(-2 * np.pi, 2 * np.pi, 50000).astype(F32)
    x = np.concatenate([u, near, small])
    return x[np.abs(x) <= 1000.0]


def gen_asin():
    rng = np.random.RandomState(13)
    m = 20000
    parts = [rng.uniform(-0.9, 0.9, m), rng.choice([-1, 1], m) * rng.uniform(0.9, 0.999, m),
             rng.choice([-1, 1], m) * rng.uniform(0.999, 0.99999, m), rng.choice([-1, 1], m) * (1 - 10.0 ** rng.uniform(-9, -5, m)),
             np.concatenate([next_floats(1.0, 8), next_floats(-1.0, 8), [0.0, -0.0]])]
    x = np.clip(np.concatenate(parts).astype(F32), F32(-1), F32(1))
    b = pitch_buckets(x)
    b.pop("clamped")
    return x, b


def gen_euler():
    """quaternions with |sin pitch| in every bucket up to gimbal lock; the last group sits AT +-90 degrees with a norm a hair above 1,
    so that -2 (xz - wy) exceeds 1 by rounding (the clamped ends)"""
    rng = np.random.RandomState(14)
    m = 20000

    def q(sp):
        return quat_from_euler64(rng.uniform(-np.pi, np.pi, len(sp)), np.arcsin(sp), rng.uniform(-np.pi, np.pi, len(sp)))
    sg = lambda: rng.choice([-1.0, 1.0], m)   # noqa: E731
    parts = [q(rng.uniform(-0.9, 0.9, m)), q(sg() * rng.uniform(0.9, 0.999, m)), q(sg() * rng.uniform(0.999, 0.99999, m)),
             q(sg() * (1 - 10.0 ** rng.uniform(-9, -5, m))),
             q(sg()) * (1.0 + rng.uniform(2e-7, 1e-6, (m, 1)))]
    x = np.concatenate(parts).astype(F32)
    return x, pitch_buckets(euler_sarg64(x))


def gen_heading():
    """quaternions (roll, pitch moderate) with the heading anywhere, within 1e-3 of 0, within 1e-3 of +-pi, and unnormalised"""
    rng = np.random.RandomState(15)
    m = 20000

    def q(yaw):
        return quat_from_euler64(rng.uniform(-0.6, 0.6, len(yaw)), rng.uniform(-0.6, 0.6, len(yaw)), yaw)
    near = lambda: rng.uniform(-0.9e-3, 0.9e-3, m)   # noqa: E731
    parts = [q(rng.uniform(-np.pi, np.pi, m)), q(near()), q(np.pi * rng.choice([-1.0, 1.0], m) + near()),
             q(rng.uniform(-np.pi, np.pi, m)) * rng.uniform(0.5, 2.0, (m, 1))]
    x = np.concatenate(parts).astype(F32)
    h = heading_def(x)
    nrm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
    unit = np.abs(nrm - 1) < 1e-6
    b = {"general": unit & (np.abs(h) >= 1e-3) & (np.pi - np.abs(h) >= 1e-3), "near_0": unit & (np.abs(h) < 1e-3),
         "near_pi": unit & (np.pi - np.abs(h) < 1e-3), "unnormalised": ~unit}
    return x, b


def gen_norm_angle():
    """rotation angle anywhere, within 1e-3 of 0 (w = +1), of 2 pi (w = -1), of pi (w of both signs), and unnormalised"""
    rng = np.random.RandomState(16)
    m = 20000

    def q(ang):
        ax = _unit(rng.standard_normal((len(ang), 3)))
        return np.concatenate([ax * np.sin(ang / 2)[:, None], np.cos(ang / 2)[:, None]], axis=1)
    sm = lambda: 10.0 ** rng.uniform(-7, np.log10(0.9e-3), m)   # noqa: E731
    parts = [q(rng.uniform(0, 2 * np.pi, m)), q(sm()), q(2 * np.pi - sm()), q(np.pi - sm()), q(np.pi + sm()),
             q(rng.uniform(0, 2 * np.pi, m)) * rng.uniform(0.5, 2.0, (m, 1))]
    x = np.concatenate(parts).astype(F32)
    x64 = x.astype(np.float64)
    ang = 2 * np.arctan2(np.sqrt((x64[:, :3] ** 2).sum(axis=1)), x64[:, 3])     # in [0, 2 pi]
    unit = np.abs(np.sqrt((x64 ** 2).sum(axis=1)) - 1) < 1e-6
    w = x64[:, 3]
    b = {"general": unit & (ang >= 1e-3) & (np.abs(ang - np.pi) >= 1e-3) & (2 * np.pi - ang >= 1e-3),
         "near_0": unit & (ang < 1e-3), "near_2pi": unit & (2 * np.pi - ang < 1e-3),
         "near_pi_w_pos": unit & (np.abs(ang - np.pi) < 1e-3) & (w >= 0), "near_pi_w_neg": unit & (np.abs(ang - np.pi) < 1e-3) & (w < 0),
         "unnormalised": ~unit}
    return x, b


def gen_quat_points():
    """(p, q) records for qrot, q for q_to_mat: unit and unnormalised quaternions"""
    rng = np.random.RandomState(17)
    m = 30000
    q = _unit(rng.standard_normal((2 * m, 4)))
    q[m:] *= rng.uniform(0.5, 2.0, (m, 1))
    p = rng.uniform(-1.0, 1.0, (2 * m, 3))
    q = q.astype(F32)
    unit = np.abs(np.sqrt((q.astype(np.float64) ** 2).sum(axis=1)) - 1) < 1e-6
    return p.astype(F32), q, {"unit": unit, "unnormalised": ~unit}


SLERP_ANGLES = {"1e-7..1e-3": (1e-7, 1e-3), "1e-3..0.1": (1e-3, 0.1), "0.1..pi/2": (0.1, np.pi / 2), "pi/2..pi-1e-3": (np.pi / 2, np.pi - 1e-3)}


def gen_slerp():
    """records (a, b, f), {bucket: mask}, and the mask of the dropped pairs (|d| < 1e-3: the shortest-path sign is ambiguous)"""
    rng = np.random.RandomState(18)
    m = 20000

    def pair(ang):
        q0 = _unit(rng.standard_normal((len(ang), 4)))
        v = rng.standard_normal((len(ang), 4))
        v = _unit(v - (v * q0).sum(axis=1, keepdims=True) * q0)
        return q0, np.cos(ang)[:, None] * q0 + np.sin(ang)[:, None] * v
    parts, names = [], []

    def add(name, q0, q1, f):
        parts.append(np.concatenate([q0, q1, np.asarray(f, dtype=np.float64).reshape(-1, 1)], axis=1).astype(F32))
        names.append(name)
    for name, (lo, hi) in SLERP_ANGLES.items():
        ang = np.exp(rng.uniform(np.log(lo), np.log(hi), m)) if hi <= 0.1 else rng.uniform(lo, hi, m)
        add(name, *pair(ang), rng.uniform(0.0, 1.0, m))
    q0, q1 = pair(np.pi - 10.0 ** rng.uniform(-7, -3, m))
    add("antipodal", q0, q1, rng.uniform(0.0, 1.0, m))
    q0, _ = pair(np.zeros(m))
    q0 = q0.astype(F32).astype(np.float64)
    add("identical", q0, np.where(rng.uniform(size=(m, 1)) < 0.5, q0, -q0), rng.uniform(0.0, 1.0, m))
    ang = rng.uniform(1e-3, np.pi - 1e-3, m)
    ang[np.abs(ang - np.pi / 2) < 2e-3] = 1.0
    add("f=0", *pair(ang), np.zeros(m))
    add("f=1", *pair(ang), np.ones(m))
    q0, q1 = pair(ang)
    add("unnormalised", q0 * rng.uniform(0.5, 2.0, (m, 1)), q1 * rng.uniform(0.5, 2.0, (m, 1)), rng.uniform(0.0, 1.0, m))
    x = np.concatenate(parts)
    masks, at = {}, 0
    for name, p in zip(names, parts):
        masks[name] = np.zeros(len(x), dtype=bool)
        masks[name][at:at + len(p)] = True
        at += len(p)
    _, d = slerp_def(x[:, 0:4], x[:, 4:8], x[:, 8])
    dropped = (np.abs(d) < 1e-3) & (x[:, 8] != 0) & (x[:, 8] != 1)
    return x, masks, dropped


# =====================================================================================================================
# C. Cholesky
# =====================================================================================================================
def _skew(c):
    z = np.zeros(len(c))
    return np.stack([np.stack([z, -c[:, 2], c[:, 1]], axis=1), np.stack([c[:, 2], z, -c[:, 0]], axis=1),
                     np.stack([-c[:, 1], c[:, 0], z], axis=1)], axis=1)


def gen_chol(n_inertia=4096, n_random=2048):
    """records (A row-major, b) [n, 42] and {bucket: mask}: composite spatial inertias sum_k X_k^T I_k X_k of 13 bodies (0.25 .. 13 kg at
    leg-like offsets; [angular; linear] ordering about the base origin) and random SPD matrices with condition numbers log-spaced to 1e5"""
    rng = np.random.RandomState(19)
    A = np.zeros((n_inertia, 6, 6))
    for k in range(13):
        mass = 13.0 if k == 0 else np.exp(rng.uniform(np.log(0.25), np.log(3.0), n_inertia))
        c = rng.uniform(-1, 1, (n_inertia, 3)) * (np.array([0.03, 0.03, 0.03]) if k == 0 else np.array([0.3, 0.2, 0.5]))
        Q, _ = np.linalg.qr(rng.standard_normal((n_inertia, 3, 3)))
        pm = np.asarray(mass).reshape(-1, 1) * rng.uniform(0.02, 0.25, (n_inertia, 3)) ** 2      # principal moments m r^2
        Ic = np.einsum("nij,nj,nkj->nik", Q, pm, Q)
        S = _skew(c)
        mm = np.broadcast_to(np.asarray(mass, dtype=np.float64), (n_inertia,))[:, None, None]
        A[:, :3, :3] += Ic + mm * np.einsum("nij,nkj->nik", S, S)
        A[:, :3, 3:] += mm * S
        A[:, 3:, :3] += mm * np.transpose(S, (0, 2, 1))
        A[:, 3:, 3:] += mm * np.eye(3)
    Q, _ = np.linalg.qr(rng.standard_normal((n_random, 6, 6)))
    cond = 10.0 ** np.linspace(0, 5, n_random)
    lam = cond[:, None] ** (-np.sort(rng.uniform(0, 1, (n_random, 6)), axis=1))
    lam[:, 0], lam[:, -1] = 1.0, 1.0 / cond
    lam *= 10.0 ** rng.uniform(-1, 1, (n_random, 1))
    B = np.einsum("nij,nj,nkj->nik", Q, lam, Q)
    M = np.concatenate([A, B]).astype(F32)
    M = np.tril(M) + np.transpose(np.tril(M, -1), (0, 2, 1))       # exactly symmetric in float32
    b = (rng.standard_normal((len(M), 6)) * 10.0 ** rng.uniform(-1, 2, (len(M), 1))).astype(F32)
    rec = np.concatenate([M.reshape(len(M), 36), b], axis=1)
    kind = np.arange(len(M)) < n_inertia
    return rec, {"composite_inertia": kind, "random_spd": ~kind}


def chol_backward_error(rec, x):
    """normwise backward error |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), float64"""
    A = np.asarray(rec[:, :36], dtype=np.float64).reshape(-1, 6, 6)
    b = np.asarray(rec[:, 36:], dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    r = np.abs(b - np.einsum("nij,nj->ni", A, x)).max(axis=1)
    return r / (np.abs(A).sum(axis=2).max(axis=1) * np.abs(x).max(axis=1) + np.abs(b).max(axis=1))


# =====================================================================================================================
# D. RNG and step limit
# =====================================================================================================================
PHILOX_SEEDS = (0, 5, 2 ** 32 - 1, 2 ** 32, 0xDEADBEEF12345678, 2 ** 64 - 1)
PHILOX_INDICES = (0, 1, 63, 4095, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)


def gen_philox():
    """(seed, robot, episode, block) for every combination of the seeds, robot and episode indices above and blocks 0 .. 63"""
    s, r, e, b = np.meshgrid(np.array(PHILOX_SEEDS, dtype=np.uint64), np.array(PHILOX_INDICES, dtype=np.uint64),
                             np.array(PHILOX_INDICES, dtype=np.uint64), np.arange(64, dtype=np.uint64), indexing="ij")
    return s.ravel(), r.ravel().astype(np.uint32), e.ravel().astype(np.uint32), b.ravel().astype(np.uint32)


TIME_LIMIT_CONFIGS = ((True, 20_000_000, 50, 600), (True, 1000, 600, 50), (True, 3, 10, 1000), (True, 2 ** 36, 1, 30000),
                      (False, 20_000_000, 50, 600), (True, 0, 50, 600), (True, -5, 50, 600))


def gen_time_limit_totals(steps, start, end):
    """totals around every boundary of the curriculum t^3 ramp (where the integer limit changes), a coarse sweep, and powers of two to 2^40"""
    tot = [np.array([-2 ** 40, -1, 0, 1, 2, 3], dtype=np.float64), 2.0 ** np.arange(0, 41), 2.0 ** np.arange(1, 41) - 1]
    if steps > 0:
        tot.append(np.linspace(0, 1.25 * steps, 2001))
        if start != end:
            lim = np.arange(min(start, end), max(start, end) + 1)
            if len(lim) > 2000:
                lim = lim[:: len(lim) // 2000]
            t = np.cbrt((lim - start) / float(end - start)) * steps
            tot += [np.floor(t) + d for d in (-2, -1, 0, 1, 2)]
        tot.append(steps + np.arange(-3, 4.0))
    return np.unique(np.concatenate(tot).astype(np.int64))


# =====================================================================================================================
# E. the constraint solver's register stages: Delassus columns and projected Gauss-Seidel sweeps
# =====================================================================================================================
# A robot's problem is indexed by row SLOT (solve order): 0..3 knee friction motors, 4..15 joint limits (joint = slot - 4),
# 16..19 toe normals (leg = slot - 16), 20..27 friction (leg = (slot - 20) // 2, direction x / y).  Generalised velocities: 6 base
# (angular, linear) + 12 joints (3 per leg).  On the device lane l of a robot holds bank-A slot (l if l < 4 else l + 12) and, for
# l >= 4, bank-B slot l.  A batch of problems is a dict of arrays with the robots along axis 0 (see gen_solver_bucket).
N_SLOTS, N_DOF = 28, 18
SLOT_ORDER = tuple(range(N_SLOTS))
LANE_SLOT_A = np.array([l if l < 4 else l + 12 for l in range(16)])
NRM_SLOT = np.array([-1] * 20 + [16 + (r - 20) // 2 for r in range(20, 28)])        # friction row -> its toe's normal row
SLOT_LEG = np.array([r for r in range(4)] + [(r - 4) // 3 for r in range(4, 16)] + [r - 16 for r in range(16, 20)] +
                    [(r - 20) // 2 for r in range(20, 28)])
SLOT_DIR = np.array([-1] * 16 + [2] * 4 + [0, 1] * 4)                               # contact rows: z (normal), x, y
SOLVER_BUCKETS = ("standing", "sliding", "limits", "missing_legs", "soft", "idle")
SOLVER_ROBOTS = 1024                                                                 # per bucket: 16384 lanes, 256 waves
SOLVER_ITERS = 10
BIG = F32(1e30)                                                                      # "no upper bound" of the unilateral rows


def solver_jacobians(P):
    """J[R, 28, 18] in float64 from the float32 geometry, built as row_setup_bank_a / row_setup_limit build (Jb, jl): knee rows e_knee,
    limit rows sgn e_joint, contact rows ((rr x dir, dir), dir . ck[k] on the joints of their own leg)."""
    n = len(P["rr"])
    J = np.zeros((n, N_SLOTS, N_DOF))
    for r in range(4):
        J[:, r, 6 + 3 * r + 2] = 1.0
    for r in range(4, 16):
        J[:, r, 6 + r - 4] = P["sgn"][:, r - 4]
    rr, ck = P["rr"].astype(np.float64), P["ck"].astype(np.float64)
    for r in range(16, 28):
        g, d = SLOT_LEG[r], SLOT_DIR[r]
        dirv = np.zeros(3)
        dirv[d] = 1.0
        J[:, r, 0:3] = np.cross(rr[:, g], dirv)
        J[:, r, 3:6] = dirv
        J[:, r, 6 + 3 * g:9 + 3 * g] = ck[:, g, :, d]
    return J


def visited_columns(P, has_b):
    """[R, 28] bool: the columns delassus_columns<HAS_B> computes for the robot's WAVE mask (knee rows always, a joint-limit row by its
    bit, the three contact rows of a leg by the leg's normal bit); every other slot reads 0 and is not swept (joint limits) or is a
    no-op in the sweeps (contact rows of a leg that no robot of the wave has on the ground)."""
    m = np.repeat(np.asarray(P["mask"], dtype=np.uint32), 4)
    v = np.zeros((len(m), N_SLOTS), dtype=bool)
    v[:, 0:4] = True
    for r in range(4, 16):
        v[:, r] = has_b & (((m >> np.uint32(r)) & 1) == 1)
    for r in range(16, 28):
        v[:, r] = ((m >> np.uint32(16 + SLOT_LEG[r])) & 1) == 1
    return v


def delassus_ref64(P, has_b):
    """The expression the device evaluates, A[row][r] = J_r . W[row], in float64 from the float32 inputs (NOT J_row . W[r]: the W are
    rounded, the two differ in the last bits), and the sum of the terms' magnitudes; 0 where the column is not visited.
    -> (A[R, 28 row, 28 r], mag the same shape)"""
    J = solver_jacobians(P)
    W = P["W"].astype(np.float64)
    v = visited_columns(P, has_b)[:, None, :]
    A = np.einsum("nck,nrk->nrc", J, W)
    mag = np.einsum("nck,nrk->nrc", np.abs(J), np.abs(W))
    return np.where(v, A, 0.0), np.where(v, mag, 0.0)


def delassus_ref64_brute(P, has_b, i):
    """the same for robot i, by loops"""
    J = solver_jacobians(P)[i]
    W = P["W"][i].astype(np.float64)
    v = visited_columns(P, has_b)[i]
    A, mag = np.zeros((N_SLOTS, N_SLOTS)), np.zeros((N_SLOTS, N_SLOTS))
    for row in range(N_SLOTS):
        for r in range(N_SLOTS):
            if v[r]:
                for k in range(N_DOF):
                    A[row, r] += J[r, k] * W[row, k]
                    mag[row, r] += abs(J[r, k] * W[row, k])
    return A, mag


def scaled_system64(P, has_b, A=None):
    """What the sweeps work on, in float64: Ac[row][r] = -A[row][r] jdi_row off the diagonal (0 on it and in unvisited columns),
    w = cfm lam + (A lam) of the warm start over the visited columns, lam0 (0 in unvisited slots) and y0 = lam0 + rhs - w jdi."""
    if A is None:
        A, _ = delassus_ref64(P, has_b)
    v = visited_columns(P, has_b)
    jdi, cfm, rhs = P["jdi"].astype(np.float64), P["cfm"].astype(np.float64), P["rhs"].astype(np.float64)
    lam_row = P["lam"].astype(np.float64)
    lam0 = np.where(v, lam_row, 0.0)
    Ac = -A * jdi[:, :, None]
    Ac[:, np.arange(N_SLOTS), np.arange(N_SLOTS)] = 0.0
    w = cfm * lam_row + np.einsum("nrc,nc->nr", A, lam0)
    return {"Ac": Ac, "w": w, "lam0": lam0, "y0": lam_row + rhs - w * jdi, "swept": swept_rows(P, has_b)}


def swept_rows(P, has_b):
    """[R, 28] bool: knee and contact rows are swept unconditionally, joint-limit rows by the wave's mask bit"""
    s = visited_columns(P, has_b)
    s[:, 16:] = True
    return s


def pgs_ref64_brute(y0, Ac, lam0, lo_c, hi_c, mu, swept, iters):
    """ONE robot, the oracle's row update (oracle/orr_oracle.c, projected Gauss-Seidel) in float64, slots in solve order:
        lam_r <- clamp(lam_r + (rhs_r - A_r . lam - cfm_r lam_r) / (A_rr + cfm_r)),  friction bounds -/+ mu lam[normal] of the moment.
    Divided through by (A_rr + cfm_r) and written with the inputs the device gets (Ac = -A / (A_rr + cfm) off the diagonal, and
    y0 = the right-hand side of the warm start lam0) that is  lam_r <- clamp(y0_r + sum_{c != r} Ac[r][c] (lam_c - lam0_c)).
    -> lam after each sweep [iters + 1, 28] (row 0: lam0)."""
    lam = np.array(lam0, dtype=np.float64)
    out = [lam.copy()]
    for _ in range(iters):
        for r in SLOT_ORDER:
            if not swept[r]:
                continue
            v = y0[r]
            for c in range(N_SLOTS):
                if c != r:
                    v += Ac[r, c] * (lam[c] - lam0[c])
            if NRM_SLOT[r] >= 0:
                hi = mu[r] * lam[NRM_SLOT[r]]
                lo = -hi
            else:
                lo, hi = lo_c[r], hi_c[r]
            lam[r] = min(max(v, lo), hi)
        out.append(lam.copy())
    return np.array(out)


def pgs_ref64(S, P, iters):
    """pgs_ref64_brute for every robot at once: S = a scaled system (scaled_system64, or float32 inputs cast up), P the problem (bounds).
    -> [iters + 1, R, 28]"""
    y0, Ac, lam0, swept = (np.asarray(S[k], dtype=np.float64) if k != "swept" else S[k] for k in ("y0", "Ac", "lam0", "swept"))
    lo_c, hi_c, mu = P["lo_c"].astype(np.float64), P["hi_c"].astype(np.float64), P["mu"].astype(np.float64)
    lam = lam0.copy()
    out = [lam.copy()]
    for _ in range(iters):
        for r in SLOT_ORDER:
            v = y0[:, r] + np.einsum("nc,nc->n", Ac[:, r], lam - lam0)       # Ac[r][r] = 0
            if NRM_SLOT[r] >= 0:
                hi = mu[:, r] * lam[:, NRM_SLOT[r]]
                lo = -hi
            else:
                lo, hi = lo_c[:, r], hi_c[:, r]
            lam[:, r] = np.where(swept[:, r], np.minimum(np.maximum(v, lo), hi), lam[:, r])
        out.append(lam.copy())
    return np.array(out)


def _fma(a, b, c):
    """a b + c rounded once to the operands' type (float32: the product-sum in float64, rounded once more; float64: as numpy has it)"""
    if a.dtype == F32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    return a * b + c


def pgs_yform(I, has_b, iters):
    """The generic pgs_sweeps of csrc/orr_physics.h (the C++ form behind ORR_GENERIC_PGS) restated in numpy, in the type of the inputs:
    float32 inputs give the float32 FLOOR (one rounding per fused operation), float64 inputs the same algorithm in float64.
    I = lane-space inputs (solver_lane_inputs): rows lamA wA jdiA rhsA loA hiA muA lam_nA [R, 16], the same for bank B, AcA / AcB
    [R, 16, 28], lam [R, 28], swept [R, 28].  A row lane keeps y (its unclamped value), the robot keeps lam[28].
    -> lam after each sweep [iters + 1, R, 28]"""
    dt = I["lam"].dtype
    yA = I["lamA"] + _fma(-I["wA"], I["jdiA"], I["rhsA"])
    yB = I["lamB"] + _fma(-I["wB"], I["jdiB"], I["rhsB"])
    hiE, loE = _fma(I["muA"], I["lam_nA"], I["hiA"]), _fma(-I["muA"], I["lam_nA"], I["loA"])
    AcA, AcB, swept = I["AcA"], I["AcB"], I["swept"]
    lam = I["lam"].copy()
    zero = dt.type(0)
    mun = [np.where(NRM_SLOT[LANE_SLOT_A][None, :] == 16 + g, I["muA"], zero) for g in range(4)]
    out = [lam.copy()]
    for _ in range(iters):
        for r in SLOT_ORDER:
            old = lam[:, r:r + 1]
            if r < 4 or r >= 16:
                src = r if r < 4 else r - 12
                yp = _fma(-AcA[:, :, r], old, yA)
                if 16 <= r < 20:
                    sb = np.maximum(yA[:, src], zero)
                else:
                    sb = np.minimum(np.maximum(yA[:, src], loE[:, src]), hiE[:, src])       # lo <= hi always: the median of the three
                sb = sb[:, None]
                yA = _fma(AcA[:, :, r], sb, yp)
                if has_b:
                    yB = _fma(AcB[:, :, r], sb - old, yB)
                if 16 <= r < 20:
                    d = sb - old
                    hiE, loE = _fma(mun[r - 16], d, hiE), _fma(-mun[r - 16], d, loE)
                lam[:, r] = sb[:, 0]
            elif has_b:
                on = swept[:, r:r + 1]
                yp = _fma(-AcB[:, :, r], old, yB)
                sb = np.maximum(yB[:, r], zero)[:, None]
                yB = np.where(on, _fma(AcB[:, :, r], sb, yp), yB)
                yA = np.where(on, _fma(AcA[:, :, r], sb - old, yA), yA)
                lam[:, r] = np.where(on[:, 0], sb[:, 0], lam[:, r])
        out.append(lam.copy())
    return np.array(out)


def solver_lane_inputs(P, has_b, dt=F32):
    """The sweeps' inputs per lane, as the test hands them to orrp_pgs_a / _ab: the columns of delassus_ref64 scaled and rounded ONCE to
    float32 (dt = float64: not rounded), w and lam_n of the warm start."""
    S = scaled_system64(P, has_b)
    n = len(P["rr"])
    rd = lambda x: np.asarray(x, dtype=np.float64).astype(dt)     # noqa: E731
    I = {"lam": rd(S["lam0"]), "swept": S["swept"]}
    la = LANE_SLOT_A
    nrm = NRM_SLOT[la]
    lam_n = np.where(nrm[None, :] >= 0, S["lam0"][:, np.maximum(nrm, 0)], 0.0)
    for key, src in (("lam", P["lam"]), ("w", S["w"]), ("jdi", P["jdi"]), ("rhs", P["rhs"]), ("cfm", P["cfm"]), ("lo", P["lo_c"]),
                     ("hi", P["hi_c"]), ("mu", P["mu"])):
        I[key + "A"] = rd(src[:, la])
        b = rd(src[:, :16]).copy()
        b[:, :4] = 0
        I[key + "B"] = b
    I["lam_nA"], I["lam_nB"] = rd(lam_n), np.zeros((n, 16), dtype=dt)
    I["AcA"] = rd(S["Ac"][:, la, :])
    I["AcB"] = rd(S["Ac"][:, :16, :]).copy()
    I["AcB"][:, :4] = 0
    if not has_b:
        I["AcB"][:] = 0
    return I


def pgs_records(P, I):
    """[R * 16, 105] float32 records of orrp_pgs_a / _ab from lane inputs (layout: tests/device_probe/orr_probe_solver.hip)"""
    n = len(I["lam"])
    rec = np.zeros((n, 16, 105), dtype=F32)
    for off, bank in ((0, "A"), (10, "B")):
        for k, key in enumerate(("lam", "w", "jdi", "rhs", "cfm", "lo", "hi", "mu", "lam_n")):
            rec[:, :, off + k] = I[key + bank]
    rec[:, :, 9] = NRM_SLOT[LANE_SLOT_A][None, :]
    rec[:, :, 19] = -1
    rec[:, :, 20:48], rec[:, :, 48:76] = I["AcA"], I["AcB"]
    rec[:, :, 76:104] = I["lam"][:, None, :]
    rec[:, :, 104] = np.repeat(np.asarray(P["mask"], dtype=np.uint32), 4).view(F32)[:, None]
    return rec.reshape(n * 16, 105)


def delassus_records(P):
    """[R * 16, 75] float32 records of orrp_delassus_pgs_a / _ab.  The ContactGeom of a leg sits in its normal row's lane (4 + leg), the
    only lane dpp_contact_triplet reads it from; every other lane carries P["gfill"], values nothing may depend on."""
    n = len(P["rr"])
    rec = np.zeros((n, 16, 75), dtype=F32)

    def row(off, slots, valid):
        jl = np.zeros((n, 16, 3), dtype=F32)
        J = solver_jacobians(P)
        for l, r in enumerate(slots):
            g = SLOT_LEG[r]
            jl[:, l] = J[:, r, 6 + 3 * g:9 + 3 * g]
        fields = [P["active"][:, slots].astype(F32), np.broadcast_to(SLOT_LEG[slots].astype(F32), (n, 16)),
                  np.broadcast_to(NRM_SLOT[slots].astype(F32), (n, 16)), jl[:, :, 0], jl[:, :, 1], jl[:, :, 2], P["rhs"][:, slots],
                  P["jdi"][:, slots], P["lam"][:, slots], P["cfm"][:, slots], P["lo_c"][:, slots], P["hi_c"][:, slots], P["mu"][:, slots]]
        for k, f in enumerate(fields):
            rec[:, :, off + k] = f
        rec[:, :, off + 13:off + 31] = P["W"][:, slots]
        rec[:, ~valid, off:off + 31] = 0
        rec[:, ~valid, off + 2] = -1
    row(0, LANE_SLOT_A, np.ones(16, dtype=bool))
    row(31, np.arange(16), np.arange(16) >= 4)
    rec[:, :, 62:74] = P["gfill"]
    for g in range(4):
        rec[:, 4 + g, 62:65] = P["rr"][:, g]
        rec[:, 4 + g, 65:74] = P["ck"][:, g].reshape(n, 9)
    rec[:, :, 74] = np.repeat(np.asarray(P["mask"], dtype=np.uint32), 4).view(F32)[:, None]
    return rec.reshape(n * 16, 75)


def wave_masks(active):
    """the wave's row mask as physics_substep lays it out: the union over its four robots of the active slots, bit = slot for 0..15,
    bit 16 + (lane - 4) for the bank-A lanes 4..15 (slots 16..27)"""
    a = np.asarray(active, dtype=bool).reshape(-1, 4, N_SLOTS).any(axis=1)
    return (a.astype(np.uint32) << np.arange(N_SLOTS, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)


def gen_solver_bucket(name, n=SOLVER_ROBOTS, seed=0):
    """One named bucket of n robots' solver problems (n a multiple of 4: whole waves).  M^-1 is a random SPD 18 x 18 matrix with its
    eigenvalues spread over 2.5 decades, W = M^-1 J^T rounded to float32, jdi = 1 / (J_r . W_r + cfm) rounded to float32 (0 for an
    inactive row), rhs already multiplied by jdi; half of the robots carry a warm start.  Inactive rows are pinned as the row setup pins
    them (rhs, jdi, impulse and bounds 0) but keep a Jacobian and a response, as on the device.
      standing      all four legs down, friction 0.5 .. 1, low tangential velocities
      sliding       friction 0.2 .. 0.5, high tangential velocities
      limits        a quarter of the joints has a limit row (the wave's mask then carries bits of rows other robots lack)
      missing_legs  every wave lacks one leg in all four robots; the others come and go
      soft          cfm > 0 on the toe normals
      idle          no active row at all"""
    assert name in SOLVER_BUCKETS and n % 4 == 0
    rng = np.random.RandomState(1000 + 17 * SOLVER_BUCKETS.index(name) + seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, N_DOF, N_DOF)))
    ev = 10.0 ** rng.uniform(-1.25, 1.25, (n, N_DOF))
    ev[:, 0], ev[:, 1] = 10.0 ** -1.25, 10.0 ** 1.25
    Minv = np.einsum("nij,nj,nkj->nik", Q, ev, Q)
    P = {"rr": (rng.uniform(-1, 1, (n, 4, 3)) * np.array([0.3, 0.2, 0.4])).astype(F32),
         "ck": (rng.standard_normal((n, 4, 3, 3)) * 0.3).astype(F32),                    # ck[leg][k] = (c_k0, c_k1, c_k2)
         "sgn": rng.choice([-1.0, 1.0], (n, 12)).astype(F32),
         "gfill": (rng.standard_normal((n, 16, 12)) * 0.3).astype(F32)}
    J = solver_jacobians(P)
    P["W"] = np.einsum("nij,nrj->nri", Minv, J).astype(F32)
    diag = np.einsum("nrk,nrk->nr", J, P["W"].astype(np.float64))
    # which rows exist
    act = np.zeros((n, N_SLOTS), dtype=bool)
    if name != "idle":
        act[:, 0:4] = rng.uniform(size=(n, 4)) < 0.9
        down = np.ones((n, 4), dtype=bool) if name == "standing" else rng.uniform(size=(n, 4)) < 0.75
        if name == "missing_legs":
            down[np.arange(n), np.repeat(rng.randint(0, 4, n // 4), 4)] = False
        if name == "limits":
            act[:, 4:16] = rng.uniform(size=(n, 12)) < 0.25
        act[:, 16:20] = down
        act[:, 20:28] = np.repeat(down, 2, axis=1)
    P["active"] = act
    P["mask"] = wave_masks(act)
    cfm = np.zeros((n, N_SLOTS))
    if name == "soft":
        cfm[:, 16:20] = diag[:, 16:20] * 10.0 ** rng.uniform(-2, 0, (n, 4))
    cfm = np.where(act, cfm, 0.0).astype(F32)
    jdi = np.where(act, 1.0 / (diag + cfm), 0.0).astype(F32)
    # right-hand sides in units of sqrt(diag) (an impulse of ~1 / sqrt(diag) per unit): normals biased to push, limits symmetric,
    # tangential velocities small (standing) or large (sliding) against the normal ones
    sd = np.sqrt(diag)
    tang = {"standing": 0.5, "sliding": 1.1}.get(name, 1.0)
    g = rng.standard_normal((n, N_SLOTS))
    g[:, 16:20] += {"standing": 1.5, "sliding": 1.0}.get(name, 0.5)
    g[:, 20:28] *= tang
    rhs = np.where(act, g * sd * jdi.astype(np.float64), 0.0).astype(F32)
    mu = np.zeros((n, N_SLOTS))
    mu[:, 20:28] = np.repeat(rng.uniform(0.2, 0.5, (n, 4)) if name == "sliding" else rng.uniform(0.5, 1.0, (n, 4)), 2, axis=1)
    P["mu"] = np.where(act, mu, 0.0).astype(F32)
    # knee bounds +-fr dt, scaled over two decades around the size of the unclamped impulse so that rows end on either side
    hi = np.zeros((n, N_SLOTS))
    hi[:, 0:4] = 10.0 ** rng.uniform(-1.5, 0.5, (n, 4)) / sd[:, 0:4]
    hi[:, 4:20] = BIG
    hi = np.where(act, hi, 0.0).astype(F32)
    hi[:, 20:28] = 0
    lo = np.zeros((n, N_SLOTS), dtype=F32)
    lo[:, 0:4] = -hi[:, 0:4]
    P["hi_c"], P["lo_c"], P["cfm"], P["jdi"], P["rhs"] = hi, lo, cfm, jdi, rhs
    # warm start (half of the robots): inside the bounds for knee, normal and limit rows; friction rows may sit outside their cone
    warm = (rng.uniform(size=(n, 1)) < 0.5) & act
    l0 = np.abs(rng.standard_normal((n, N_SLOTS))) / sd
    l0[:, 0:4] = np.minimum(l0[:, 0:4], hi[:, 0:4].astype(np.float64)) * rng.choice([-1.0, 1.0], (n, 4))
    l0[:, 20:28] *= 0.7 * rng.choice([-1.0, 1.0], (n, 8))
    P["lam"] = np.where(warm, l0, 0.0).astype(F32)
    P["name"] = name
    return P


def select_robots(P, idx):
    """the problems of robots idx (a new batch; the wave masks are rebuilt for the new grouping)"""
    idx = np.asarray(idx)
    Q = {k: v[idx] for k, v in P.items() if k not in ("mask", "name")}
    Q["mask"] = wave_masks(Q["active"])
    Q["name"] = P["name"]
    return Q


def solver_row_kinds(P):
    """{kind: [R, 28] bool} of the ACTIVE rows"""
    a = P["active"]
    k = {"knee": np.zeros_like(a), "limit": np.zeros_like(a), "normal": np.zeros_like(a), "friction": np.zeros_like(a)}
    k["knee"][:, 0:4], k["limit"][:, 4:16], k["normal"][:, 16:20], k["friction"][:, 20:28] = a[:, 0:4], a[:, 4:16], a[:, 16:20], a[:, 20:28]
    return k


def solver_bucket_stats(P, L):
    """What the bucket conditions are checked on: L = pgs_ref64(...)[: 12] (float64, 11 sweeps).  Fractions of the ACTIVE rows of each kind
    by where they end after 10 sweeps, and the median over the robots of the 11th sweep's largest change relative to the robot's
    largest impulse."""
    lam = L[SOLVER_ITERS]
    k = solver_row_kinds(P)
    bound = P["mu"].astype(np.float64) * lam[:, np.maximum(NRM_SLOT, 0)]
    frac = lambda m, kind: m.sum() / max(k[kind].sum(), 1)      # noqa: E731
    scale = np.abs(lam).max(axis=1)
    ok = scale > 0
    change = np.abs(L[SOLVER_ITERS + 1] - lam).max(axis=1)
    return {"friction_on_cone": frac(k["friction"] & (bound > 0) & (np.abs(lam) == bound), "friction"),
            "friction_inside": frac(k["friction"] & (np.abs(lam) < bound), "friction"),
            "normal_zero": frac(k["normal"] & (lam == 0), "normal"), "normal_positive": frac(k["normal"] & (lam > 0), "normal"),
            "limit_zero": frac(k["limit"] & (lam == 0), "limit"), "limit_positive": frac(k["limit"] & (lam > 0), "limit"),
            "knee_on_bound": frac(k["knee"] & (np.abs(lam) == P["hi_c"].astype(np.float64)), "knee"),
            "knee_inside": frac(k["knee"] & (np.abs(lam) < P["hi_c"].astype(np.float64)), "knee"),
            "last_sweep_change": float(np.median(change[ok] / scale[ok])) if ok.any() else 0.0}


def system_from_lane_inputs(I):
    """the scaled system (as scaled_system64 returns it) that the float32 lane inputs of orrp_pgs_a / _ab state, cast up to float64"""
    f = lambda k: I[k].astype(np.float64)     # noqa: E731
    n = len(I["lam"])
    Ac, y0 = np.zeros((n, N_SLOTS, N_SLOTS)), np.zeros((n, N_SLOTS))
    Ac[:, LANE_SLOT_A] = f("AcA")
    Ac[:, 4:16] = f("AcB")[:, 4:]
    y0[:, LANE_SLOT_A] = f("lamA") + f("rhsA") - f("wA") * f("jdiA")
    y0[:, 4:16] = (f("lamB") + f("rhsB") - f("wB") * f("jdiB"))[:, 4:]
    return {"Ac": Ac, "y0": y0, "lam0": f("lam"), "swept": I["swept"]}
