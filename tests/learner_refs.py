"""float64 references, error bounds and float32 restatements of the learner-side kernels (csrc/orr_learner.hip; gae_kernel of
csrc/orr_policy.hip).  numpy only: tests/test_learner_refs_cpu.py shows on the CPU that every comparison here passes on the restatement
and rejects a seeded defect; tests/test_gpu_learner_edges.py applies the same comparisons to the device's outputs.

Two kinds of bound (the rules of tests/stage_refs.py):
  short   sums and short chains: (chained roundings + 1) x U x the sum of the terms' magnitudes, U = 2^-24 (gpu_kit.EPS).  The count of
          each path stands next to its bound with the kernel lines it was read from.  Where a term carries a budget of its own (the gz
          behind a gb) that budget is added (first order).
  long    anything behind expf / powf / sqrtf: FLOOR_FACTOR x the error of the float32 restatement (same operation order, np.exp on
          float32) against float64 on the same inputs + SLACK_REL of the group's largest magnitude.  EXP_FACTORS would name a group that
          needs more, with its cause; it is empty.
Every reference takes the float32 inputs and the float32 scalars the host wrapper passes (1 / var, log_norm, 1 / m: formed here in
float32 as the wrapper forms them) and widens them.  A restatement's `defect` is never anything the device runs."""
import ctypes
import math

import numpy as np

from tests.gpu_kit import EPS as U

F32, F64 = np.float32, np.float64
FLOOR_FACTOR, SLACK_REL = 2.0, 2.0 ** -22
EXP_FACTORS = {}
NAN = F32(np.nan)
K_ACT = 12
LOG_2PI = 1.8378770664093454836          # kLog2Pi


def f32(x):
    return np.ascontiguousarray(x, dtype=F32)


def bits(x):
    return f32(x).view(np.uint32)


def fma(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def ratio_of(got, ref, bound):
    """largest |got - ref| / bound; 0 / 0 counts as 0, anything non-finite in got as inf"""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.broadcast_to(np.asarray(bound, F64), np.shape(ref))
    if got.shape != ref.shape or not np.isfinite(got).all():
        return np.inf
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def long_bound(restated, ref, group=None):
    """the long chains' rule, one number for the group"""
    ref = np.asarray(ref, F64)
    ferr = float(np.abs(np.asarray(restated, F64) - ref).max())
    return EXP_FACTORS.get(group, FLOOR_FACTOR) * ferr + SLACK_REL * float(np.abs(ref).max())


# ---- the reductions the kernels share ---------------------------------------------------------------------------------------------------------

def wave_tree(x):
    """wave_sum (orr_learner.hip:24-28) on [..., 64]: lane 0's value of the shuffle-down tree"""
    x = np.array(x, dtype=F32)
    for o in (32, 16, 8, 4, 2, 1):
        x[..., :o] = x[..., :o] + x[..., o:2 * o]
    return x[..., 0]


def block_partials(acc):
    """a loss head's per-workgroup partials (:70-78): acc [m, cols] -> [ceil(m / 256), cols]; four wave trees, (r0 + r1) + (r2 + r3)"""
    m, cols = acc.shape
    nblk = (m + 255) // 256
    a = np.zeros((nblk * 256, cols), dtype=F32)
    a[:m] = acc
    r = wave_tree(a.reshape(nblk, 4, 64, cols).transpose(0, 1, 3, 2))
    return (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])


def finish4(partials, defect=None):
    """ppo_head_finish_kernel and its siblings (:87-91): four interleaved row groups one after the other, (r0 + r1) + (r2 + r3)"""
    red = np.zeros((4, partials.shape[1]), dtype=F32)
    for part in range(3 if defect == "three_groups" else 4):
        for b in range(part, len(partials), 4):
            red[part] = red[part] + partials[b]
    return (red[0] + red[1]) + (red[2] + red[3])


def head_sum_chain(m):
    """roundings from a sample's value to a loss head's sum: wave tree 6 (:26), four waves 2 (:78), a row group's ceil(nblk / 4) partials one
    after the other (:87), the four groups 2 (:91)"""
    nblk = (m + 255) // 256
    return 6 + 2 + (nblk + 3) // 4 + 2


K_FEW = 16


def colsum_chain(nblk):
    """colsum_finish_kernel: few rows (:410-413) ceil(nblk / 4) adds in an accumulator + 2; many rows (:421-433) an accumulator takes every
    64th row: ceil(nblk / 64), + 2 (:427), + the 16 groups one after the other (:432)"""
    return (nblk + 3) // 4 + 2 if nblk <= K_FEW else (nblk + 63) // 64 + 2 + 16


def colsum_restate(partials, defect=None):
    """One job of colsum_finish_kernel with launch_finish's grid (:573): the HOST chooses the number of workgroups by its own threshold, a
    workgroup its path by the kernel's; columns nobody writes stay NaN.  defect: "tail_skip" (the loop behind the 64-row body starts one row
    late), "switch15" (the kernel's threshold at 15)."""
    partials = f32(partials)
    nblk, C = partials.shape
    nwg = (C + 255) // 256 if nblk <= K_FEW else (C + 15) // 16
    few = nblk <= (15 if defect == "switch15" else K_FEW)
    out = np.full(C, NAN, dtype=F32)
    if few:
        hi = min(C, nwg * 256)
        s = np.zeros((4, hi), dtype=F32)
        for b in range(nblk):
            s[b & 3] = s[b & 3] + partials[b, :hi]
        out[:hi] = (s[0] + s[1]) + (s[2] + s[3])
        return out
    hi = min(C, nwg * 16)
    red = np.zeros((16, hi), dtype=F32)
    for part in range(16):
        s = np.zeros((4, hi), dtype=F32)
        b = part
        while b + 48 < nblk:
            for u in range(4):
                s[u] = s[u] + partials[b + 16 * u, :hi]
            b += 64
        if defect == "tail_skip":
            b += 16
        u = 0
        while b < nblk:
            s[u & 3] = s[u & 3] + partials[b, :hi]
            b, u = b + 16, u + 1
        red[part] = (s[0] + s[1]) + (s[2] + s[3])
    t = np.zeros(hi, dtype=F32)
    for q in range(16):
        t = t + red[q]
    out[:hi] = t
    return out


def colsum_ref(partials):
    """-> (float64 column sums, bound): colsum_chain(rows) roundings on the column's magnitudes"""
    p = np.asarray(partials, F64)
    return p.sum(axis=0), (colsum_chain(p.shape[0]) + 1) * U * np.abs(p).sum(axis=0)


# ---- orr_relu_backward / orr_head_backward ---------------------------------------------------------------------------------------------------

def cols_ok(c):
    return c >= 4 and c % 4 == 0 and c // 4 <= 256 and 256 % (c // 4) == 0


def rows_chain(c):
    """relu_backward_kernel: a thread adds its 32 / side rows (:331, :364; the weight gradient's fmaf :354 likewise), then `side` threads'
    values are added one after the other (:377, :385); threads beyond row 32 hold zeros"""
    nacc = min(256 // (c // 4), 32)
    return 32 // nacc + nacc - 1


def relu_select(g, h):
    """the bit-exact outcome: g where h > 0, +0.0 elsewhere"""
    return np.where(f32(h) > 0, f32(g), F32(0.0))


def relu_backward_restate(g, h, gy=None, w=None, defect=None):
    """relu_backward_kernel<K> + the finishing launch: -> (g out, gb[, gw]).  K = 0: g is masked; K > 0: gz = mask(gy w^T), gw = h^T gy.
    defect: "last_row", "mask_ge", "wpart_swap", or one of colsum_restate's."""
    h = f32(h)
    m, c = h.shape
    K = 0 if gy is None else gy.shape[1]
    c4n = c // 4
    nacc = min(256 // c4n, 32)
    nblk = (m + 31) // 32
    out = np.full((m, c), NAN, dtype=F32) if K else f32(g).copy()
    partials = np.zeros((nblk, c), dtype=F32)
    wpart = np.full((nblk, (c + K) * K), NAN, dtype=F32)
    m_run = m - 1 if defect == "last_row" else m
    for blk in range(nblk):
        r0, r1 = 32 * blk, min(m_run, 32 * blk + 32)
        X, H = np.zeros((32, c), dtype=F32), np.zeros((32, c), dtype=F32)
        H[:r1 - r0] = h[r0:r1]
        if K:
            Y = np.zeros((32, K), dtype=F32)
            Y[:r1 - r0] = gy[r0:r1]
            s = np.zeros((r1 - r0, c), dtype=F32)
            for k in range(K):
                s = fma(Y[:r1 - r0, k:k + 1], f32(w)[None, :, k], s)
            gv = s
        else:
            gv = f32(g)[r0:r1]
        keep = (h[r0:r1] >= 0) if defect == "mask_ge" else (h[r0:r1] > 0)
        gv = np.where(keep, gv, F32(0.0))
        out[r0:r1] = gv
        X[:r1 - r0] = gv
        A = X.reshape(32 // nacc, nacc, c)
        acc = A[0]
        for j in range(1, 32 // nacc):
            acc = acc + A[j]
        t = acc[0]
        for s_ in range(1, nacc):
            t = t + acc[s_]
        partials[blk] = t
        if K:
            HA, YA = H.reshape(32 // nacc, nacc, c), Y.reshape(32 // nacc, nacc, K)
            gw = np.zeros((nacc, c, K), dtype=F32)
            for j in range(32 // nacc):
                gw = fma(HA[j][:, :, None], YA[j][:, None, :], gw)
            tw = gw[0]
            for s_ in range(1, nacc):
                tw = tw + gw[s_]
            c4, e = np.arange(c4n)[:, None], np.arange(4 * K)[None, :]
            val = tw[4 * c4 + e // K, e % K]                                   # the sum a thread holds for (q, k) = (e / K, e % K)
            idx = (4 * c4 + e % K) * K + e // K if defect == "wpart_swap" else (4 * c4 + e // K) * K + e % K     # :386
            wpart[blk][idx] = val
    gb = colsum_restate(partials, defect)
    if not K:
        return out, gb
    return out, gb, colsum_restate(wpart[:, :c * K], defect).reshape(c, K)


def relu_backward_ref(g, h):
    """-> gb: (float64, bound).  rows_chain + colsum_chain roundings on the kept entries' magnitudes"""
    h = f32(h)
    kept = np.where(h > 0, np.asarray(g, F64), 0.0)
    chain = rows_chain(h.shape[1]) + colsum_chain((h.shape[0] + 31) // 32)
    return kept.sum(axis=0), (chain + 1) * U * np.abs(kept).sum(axis=0)


def head_backward_ref(gy, w, h):
    """-> {gz, gb, gw: (float64, bound)}.  gz: K fmaf (:353).  gb: the gz' own budgets + the sum's chain.  gw: a thread's 32 / side fmaf
    (:354), `side` values one after the other (:385), then the column sum: the same chain on |h| |gy|"""
    gy64, w64, h64 = np.asarray(gy, F64), np.asarray(w, F64), np.asarray(h, F64)
    K = gy64.shape[1]
    keep = f32(h) > 0
    gz = np.where(keep, gy64 @ w64.T, 0.0)
    b_gz = np.where(keep, (K + 1) * U * (np.abs(gy64) @ np.abs(w64).T), 0.0)
    chain = rows_chain(h64.shape[1]) + colsum_chain((h64.shape[0] + 31) // 32)
    return {"gz": (gz, b_gz), "gb": (gz.sum(axis=0), b_gz.sum(axis=0) + (chain + 1) * U * np.abs(gz).sum(axis=0)),
            "gw": (h64.T @ gy64, (chain + 1) * U * (np.abs(h64).T @ np.abs(gy64)))}


# ---- the loss heads ----------------------------------------------------------------------------------------------------------------------------

def _logf(x):
    """the host's logf, as orr_ppo_head calls it"""
    try:
        libm = ctypes.CDLL("libm.so.6")
        libm.logf.restype, libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
        return F32(libm.logf(ctypes.c_float(float(x))))
    except (OSError, AttributeError):
        return F32(np.log(F32(x)))


def ppo_head_scalars(m, std):
    """what orr_ppo_head passes by value (:598-603)"""
    var = F32(std) * F32(std)
    return {"inv_var": F32(1.0) / var, "log_norm": F32(-6.0) * _logf(F32(2.0) * F32(3.14159265358979323846) * var), "inv_m": F32(1.0) / F32(m)}


def log_norm_of(log_std):
    """log_norm_of (:107-112): twelve adds in double, one rounding"""
    s = 6.0 * LOG_2PI
    for x in f32(log_std):
        s += float(x)
    return F32(-s)


def _clip_rule(ratio, A, lo, hi, le=False):
    s1, s2 = ratio * A, np.minimum(np.maximum(ratio, lo), hi) * A
    inside = (ratio >= lo) & (ratio <= hi)
    passes = inside | ((s1 <= s2) if le else (s1 < s2))
    return s1, s2, inside, passes


def ppo_head_ref(mean, value, batch, std, clip, vf_coef, log_std=None, ent_coef=0.0):
    """float64 of orr_ppo_head (log_std None) / orr_ppo_head_logstd: the analytic gradient of ppo.PPO.update's loss (what autograd gives: a
    sample inside the clip range or on the unclipped side passes -A).  -> dict of float64 arrays + "ratio", "dead" (gradient exactly 0)."""
    mean64, batch64 = np.asarray(mean, F64), np.asarray(batch, F64)
    m = len(mean64)
    d = batch64[:, :K_ACT] - mean64
    old, A, ret = batch64[:, 12], batch64[:, 13], batch64[:, 14]
    inv_m = float(F32(1.0) / F32(m))
    vf64 = float(F32(vf_coef))
    if log_std is None:
        sc = ppo_head_scalars(m, std)
        z2 = d * d * float(sc["inv_var"])
        logp = -0.5 * z2.sum(axis=1) + float(sc["log_norm"])
        dlogp_dmean = d * float(sc["inv_var"])
    else:
        ls = np.asarray(f32(log_std), F64)
        z = d * np.exp(-ls)
        z2 = z * z
        logp = -0.5 * z2.sum(axis=1) + float(log_norm_of(log_std))        # the float32 constant, as its sibling's wrapper passes one
        dlogp_dmean = z * np.exp(-ls)
    ratio = np.exp(logp - old)
    s1, s2, inside, passes = _clip_rule(ratio, A, float(F32(1.0) - F32(clip)), float(F32(1.0) + F32(clip)))      # lo, hi as the kernel forms them (:55)
    gl = np.where(passes, -A, 0.0) * ratio * inv_m
    dv = np.asarray(value, F64) - ret
    gv = vf64 * 2.0 * dv * inv_m
    gm = gl[:, None] * dlogp_dmean
    R = {"g_mean": gm, "g_value": gv, "gb_mean": gm.sum(axis=0), "gb_value": gv.sum(), "surr": (-np.minimum(s1, s2)).sum() * inv_m,
         "vloss": (dv * dv).sum() * inv_m, "ratio": ratio, "dead": gl == 0.0, "dv": dv, "gl": gl, "inside": inside}
    if log_std is not None:
        R.update({"g_logstd": (gl[:, None] * (z2 - 1.0)).sum(axis=0) - float(F32(ent_coef)), "entropy": ls.sum() + 6.0 * (LOG_2PI + 1.0),
                  "kl": ((ratio - 1.0) - (logp - old)).sum() * inv_m, "clipfrac": float((~inside).sum()) / m, "terms_ls": gl[:, None] * (z2 - 1.0)})
    return R


def ppo_head_restate(mean, value, batch, std, clip, vf_coef, log_std=None, ent_coef=0.0, defect=None):
    """ppo_head_kernel / ppo_head_logstd_kernel + their finish in float32, operation for operation.  defect: "last_row", "clip_le",
    "three_groups"."""
    mean, batch, value = f32(mean), f32(batch), f32(value)
    m = len(mean)
    clip, vf = F32(clip), F32(vf_coef)
    inv_m = F32(1.0) / F32(m)
    d = batch[:, :K_ACT] - mean
    old, A, ret = batch[:, 12], batch[:, 13], batch[:, 14]
    sq = np.zeros(m, dtype=F32)
    if log_std is None:
        sc = ppo_head_scalars(m, std)
        for k in range(K_ACT):
            sq = sq + d[:, k] * d[:, k]
        logp = F32(-0.5) * sq * sc["inv_var"] + sc["log_norm"]
    else:
        inv_std = np.exp(-f32(log_std))
        z = d * inv_std
        for k in range(K_ACT):
            sq = sq + z[:, k] * z[:, k]
        logp = F32(-0.5) * sq + log_norm_of(log_std)
    log_ratio = logp - old
    ratio = np.exp(log_ratio)
    s1, s2, inside, passes = _clip_rule(ratio, A, F32(1.0) - clip, F32(1.0) + clip, le=defect == "clip_le")
    dr = np.where(passes, -A, F32(0.0))
    dv = value - ret
    gv = vf * F32(2.0) * dv * inv_m
    cols = 16 if log_std is None else 32
    acc = np.zeros((m, cols), dtype=F32)
    if log_std is None:
        gl = dr * ratio * inv_m * sc["inv_var"]
        gm = gl[:, None] * d
    else:
        gl = dr * ratio * inv_m
        gm = gl[:, None] * z * inv_std
        acc[:, 15], acc[:, 16] = (ratio - F32(1.0)) - log_ratio, np.where(inside, F32(0.0), F32(1.0))
        acc[:, 17:29] = gl[:, None] * (z * z - F32(1.0))
    acc[:, :12], acc[:, 12], acc[:, 13], acc[:, 14] = gm, gv, -np.minimum(s1, s2), dv * dv
    gm, gv = gm.copy(), gv.copy()
    if defect == "last_row":
        acc[m - 1], gm[m - 1], gv[m - 1] = 0.0, NAN, NAN
    t = finish4(block_partials(acc), defect)
    R = {"g_mean": gm, "g_value": gv, "gb_mean": t[:12], "gb_value": t[12], "surr": t[13] * inv_m, "vloss": t[14] * inv_m, "ratio": ratio}
    if log_std is not None:
        R.update({"kl": t[15] * inv_m, "clipfrac": t[16] / F32(m), "g_logstd": t[17:29] - F32(ent_coef), "entropy": F32(6.0) - log_norm_of(log_std)})
    return R


LONG_HEAD_GROUPS = ("g_mean", "gb_mean", "surr", "g_logstd", "kl")
KL_EXPF_ULPS = 2.0


def ppo_head_bounds(ref, restated, vf_coef):
    """-> {name: bound}.  Behind expf (the ratio and all it scales): the long rule per group.  Short: g_value = vf 2 dv / m: dv 1, vf 1, 1 / m 1
    + its own 1 (:65-66): 4; gb_value: + head_sum_chain; vloss: dv 1, square 1, the sum, 1 / m 2 (:68, :95); entropy: the double sum's
    rounding and 6 - it (:194): 2; clipfrac is exact: 0."""
    m = len(ref["g_value"])
    B = {k: long_bound(restated[k], ref[k], "head." + k) for k in LONG_HEAD_GROUPS if k in ref}
    if "kl" in B:
        # (ratio - 1) - log_ratio (:159) cancels to ~ log_ratio^2 / 2 and hands an ulp of the ratio on unscaled: 6e-8 against terms of 0.04.
        # The restatement's np.exp errs evenly about zero and the mean over m averages it away (its own error: 1e-9, a tenth of the
        # slack), so twice that says nothing about an expf that leans one way by a fraction of an ulp, which the mean keeps.  The two ulps
        # the long rule's factor is meant to grant the device's expf are granted here explicitly: 2 U x the mean ratio.
        B["kl"] = B["kl"] + KL_EXPF_ULPS * U * float(np.abs(ref["ratio"]).mean())
    B["g_value"] = 5 * U * np.abs(ref["g_value"])
    B["gb_value"] = (4 + head_sum_chain(m) + 1) * U * np.abs(ref["g_value"]).sum()
    B["vloss"] = (4 + head_sum_chain(m) + 1) * U * ref["vloss"]
    if "entropy" in ref:
        B["entropy"] = 3 * U * (6.0 + abs(ref["entropy"] - 6.0))
    return B


def near_clip_edge(ref, restated, clip):
    """samples whose float64 ratio lies within the ratio's own (relative, long-rule) bound of 1 +- clip: left out of the exact-zero check"""
    r = ref["ratio"]
    rel = FLOOR_FACTOR * float(np.abs(np.asarray(restated["ratio"], F64) / r - 1.0).max()) + SLACK_REL
    lo, hi = float(F32(1.0) - F32(clip)), float(F32(1.0) + F32(clip))
    return (np.abs(r - lo) <= rel * r) | (np.abs(r - hi) <= rel * r)


def distill_head_ref(mean, target):
    """-> {g_mean, gb_mean, loss: (float64, bound)}.  g = 2 d / m: d 1, 1 / m 1 + its own 1 (:232-236): 3; gb: + head_sum_chain;
    loss: d 1, twelve fmaf 12 (:236), the sum, 1 / m 2 (:264)"""
    d = np.asarray(mean, F64) - np.asarray(target, F64)
    m = len(d)
    inv_m = float(F32(1.0) / F32(m))
    g = 2.0 * d * inv_m
    ch = head_sum_chain(m)
    loss = (d * d).sum() * inv_m
    return {"g_mean": (g, 4 * U * np.abs(g)), "gb_mean": (g.sum(axis=0), (3 + ch + 1) * U * np.abs(g).sum(axis=0)),
            "loss": (loss, (1 + 12 + ch + 2 + 1) * U * loss)}


def distill_head_restate(mean, target, defect=None):
    d = f32(mean) - f32(target)
    m = len(d)
    inv_m = F32(1.0) / F32(m)
    acc = np.zeros((m, 16), dtype=F32)
    sq = np.zeros(m, dtype=F32)
    for k in range(K_ACT):
        sq = fma(d[:, k], d[:, k], sq)
    acc[:, :12], acc[:, 12] = F32(2.0) * d * inv_m, sq
    g = acc[:, :12].copy()
    if defect == "last_row":
        acc[m - 1], g[m - 1] = 0.0, NAN
    t = finish4(block_partials(acc), defect)
    return {"g_mean": g, "gb_mean": t[:12], "loss": t[12] * inv_m}


def regress_chain(m):
    """regress_head_kernel's column sums: a thread's four rows (:283, :290) 4, sixteen threads one after the other (:300) 15, the column sum"""
    return 4 + 15 + colsum_chain((m + 63) // 64)


def regress_head_ref(pred, target):
    """-> {g, gb, loss: (float64, bound)}.  g = d (2 / m): d 1, 1 / m and 2 / m 1, the product 1 (:279, :287-288): 3; gb: + regress_chain;
    loss: d 1, a row's four squares (1 + 2), four rows 4 (:291), wave tree 6, four waves 2, 1 / m 2 (:303), the column sum"""
    d = np.asarray(pred, F64) - np.asarray(target, F64)
    m = len(d)
    inv_m = float(F32(1.0) / F32(m))
    g = d * (2.0 * inv_m)
    loss = (d * d).sum() * inv_m
    ch = 1 + 3 + 4 + 6 + 2 + 2 + colsum_chain((m + 63) // 64)
    return {"g": (g, 4 * U * np.abs(g)), "gb": (g.sum(axis=0), (3 + regress_chain(m) + 1) * U * np.abs(g).sum(axis=0)), "loss": (loss, (ch + 1) * U * loss)}


def regress_head_restate(pred, target, defect=None):
    d = f32(pred) - f32(target)
    m, c = d.shape
    inv_m = F32(1.0) / F32(m)
    scale = F32(2.0) * inv_m
    nblk = (m + 63) // 64
    g = np.full((m, c), NAN, dtype=F32)
    partials, loss_part = np.zeros((nblk, c), dtype=F32), np.zeros((nblk, 1), dtype=F32)
    m_run = m - 1 if defect == "last_row" else m
    for blk in range(nblk):
        r0, r1 = 64 * blk, min(m_run, 64 * blk + 64)
        D = np.zeros((64, 64), dtype=F32)                  # 16 threads of four columns per row; those beyond c stay zero (:282)
        D[:r1 - r0, :c] = d[r0:r1]
        G = D * scale
        g[r0:r1] = G[:r1 - r0, :c]
        acc = np.zeros((16, 64), dtype=F32)                # [rsub][column]
        sq = np.zeros((16, 16), dtype=F32)                 # [rsub][q]
        for j in range(4):
            rows = slice(16 * j, 16 * j + 16)
            acc = acc + G[rows]
            Q = D[rows].reshape(16, 16, 4)
            sq = sq + ((Q[..., 0] * Q[..., 0] + Q[..., 1] * Q[..., 1]) + (Q[..., 2] * Q[..., 2] + Q[..., 3] * Q[..., 3]))
        t = acc[0]
        for k in range(1, 16):
            t = t + acc[k]
        partials[blk] = t[:c]
        w = wave_tree(sq.reshape(4, 64))                   # thread = 16 rsub + q: a wave holds four rsub
        loss_part[blk, 0] = ((w[0] + w[1]) + (w[2] + w[3])) * inv_m
    return {"g": g, "gb": colsum_restate(partials, defect), "loss": colsum_restate(loss_part, defect)[0]}


def gauss_prepare_restate(noise, log_std):
    """gauss_prepare_kernel (:205-217) -> (scaled, logp)"""
    x, ls = f32(noise), f32(log_std)
    x2 = x * x
    q = [(x2[:, 4 * j] + x2[:, 4 * j + 1]) + (x2[:, 4 * j + 2] + x2[:, 4 * j + 3]) for j in range(3)]
    return np.exp(ls) * x, F32(-0.5) * ((q[0] + q[1]) + q[2]) + log_norm_of(ls)


def gauss_prepare_ref(noise, log_std):
    x, ls = np.asarray(noise, F64), np.asarray(f32(log_std), F64)
    return x * np.exp(ls), -0.5 * (x * x).sum(axis=1) - ls.sum() - 6.0 * LOG_2PI


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------------

ADAM_MPI_EPSILON = 1


def adam_ref(p, g, m, v, t0, lr, b1, b2, eps, gscale, flags, steps=None):
    """The float64 recursion on the float32 values of lr, b1, b2, eps and grad_scale; g: one gradient per step.  -> (p, m, v, bound_m,
    bound_v) after the last step.  m: g gscale 1, g - m 1, 1 - b1 and the product 2, the sum 1 (:450-452): 5 a step; v: v b2 2, g g 1 + 2 for
    g's, 1 - b2 and the product 2, the sum 1 (:453): 8 a step; a step's budget rides on the next one's."""
    lr, b1, b2, eps, gscale = (float(F32(x)) for x in (lr, b1, b2, eps, gscale))
    p, m, v = np.asarray(p, F64).copy(), np.asarray(m, F64).copy(), np.asarray(v, F64).copy()
    bm, bv = np.zeros_like(m), np.zeros_like(v)
    for i, gr in enumerate(g):
        t = t0 + i + 1
        gg = np.asarray(gr, F64) * gscale
        bm = b1 * bm + (5 + 1) * U * (np.abs(m) + np.abs(gg))
        bv = b2 * bv + (8 + 1) * U * (v * b2 + gg * gg * (1.0 - b2))
        m = m + (gg - m) * (1.0 - b1)
        v = v * b2 + gg * gg * (1.0 - b2)
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        if flags & ADAM_MPI_EPSILON:
            p = p - lr * math.sqrt(bc2) / bc1 * m / (np.sqrt(v) + eps)
        else:
            p = p - lr / bc1 * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v, bm, bv


def adam_restate(p, g, m, v, t0, lr, b1, b2, eps, gscale, flags, defect=None):
    """adam_body (:443-463) in float32.  defect: "t_not_plus_one", "mpi_always"."""
    lr, b1, b2, eps, gscale = (F32(x) for x in (lr, b1, b2, eps, gscale))
    p, m, v = f32(p).copy(), f32(m).copy(), f32(v).copy()
    one = F32(1.0)
    mpi = bool(flags & ADAM_MPI_EPSILON) or defect == "mpi_always"
    with np.errstate(all="ignore"):
        for i, gr in enumerate(g):
            t = F32(t0 + i + (0 if defect == "t_not_plus_one" else 1))
            bc1, bc2 = one - np.power(b1, t), one - np.power(b2, t)
            sq2 = np.sqrt(bc2)
            step = lr * sq2 / bc1 if mpi else lr / bc1
            vs = one if mpi else one / sq2
            gg = f32(gr) * gscale
            m = m + (gg - m) * (one - b1)
            v = v * b2 + gg * gg * (one - b2)
            p = p - step * m / (np.sqrt(v) * vs + eps)
    return p, m, v


# ---- the gradient norm of orr_update_control ---------------------------------------------------------------------------------------------------

def sumsq_restate(g):
    """grad_sumsq_kernel + update_control_kernel's fold (:508-537) -> the float32 sum of squares"""
    g = f32(g)
    P = (len(g) + 1023) // 1024
    x = np.zeros(P * 1024, dtype=F32)
    x[:len(g)] = g
    q = (x * x).reshape(P, 2, 128, 4)
    s4 = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    lane = s4[:, 0] + s4[:, 1]                                # [P, 128]
    w = wave_tree(lane.reshape(P, 2, 64))
    partials = w[:, 0] + w[:, 1]
    fold = np.zeros(64, dtype=F32)
    for b in range(0, P, 64):
        chunk = partials[b:b + 64]
        fold[:len(chunk)] = fold[:len(chunk)] + chunk
    return wave_tree(fold)


def sumsq_bound(n):
    """orr_learner.hip:496-499, relative to the exact sum"""
    P = (n + 1023) // 1024
    return (17 + (P + 63) // 64) * U


# ---- GAE -----------------------------------------------------------------------------------------------------------------------------------------

def legacy_starts(dones, first_starts, own=False, ignore_first=False):
    """the `start` flag gae_kernel reads under ORR_GAE_LEGACY_INDEX (orr_policy.hip:358-361), [T, N] bool"""
    T, N = dones.shape
    out = np.zeros((T, N), dtype=bool)
    for k in range(T):
        for n in range(N):
            f = k * N + (n if own else 2 * n + 1) + (N if own else 0)        # the defect: the robot's own flag of the next step
            ts, js = f // N, f % N
            if ts >= T:
                out[k, n] = False
            elif ts == 0:
                out[k, n] = True if (first_starts is None or ignore_first) else bool(first_starts[js])
            else:
                out[k, n] = bool(dones[ts - 1, js])
    return out


def gae_run(rewards, vpred, dones, gamma, lam, bootstrap, legacy, first_starts, normalize, eps, f, defect=None):
    """gae_kernel (orr_policy.hip:346-376) in the float type f, on f's values of gamma, lam and eps taken from float32.
    -> (adv, ret, budget of adv before normalisation).  The budget, carried down the recursion: delta = r + gamma next own - v (:363) 3,
    last = delta + gamma lam nt last (:364) 3: (6 + 1) U on the terms' magnitudes, the older budget scaled by gamma lam nt.
    defect: "legacy_own", "first_ignored"."""
    r, v, d = np.asarray(rewards, f), np.asarray(vpred, f), np.asarray(dones, bool)
    T, N = r.shape
    gamma, lam, eps = f(F32(gamma)), f(F32(lam)), f(F32(eps))
    own = np.where(d, f(0.0), f(1.0))
    nt = own
    if legacy:
        nt = np.where(legacy_starts(d, first_starts, own=defect == "legacy_own", ignore_first=defect == "first_ignored"), f(0.0), f(1.0))
    adv, budget = np.zeros((T, N), dtype=f), np.zeros((T, N), dtype=F64)
    last, nxt, tot = np.zeros(N, dtype=f), (np.zeros(N, dtype=f) if bootstrap is None else np.asarray(bootstrap, f)), np.zeros(N, dtype=f)
    b_last = np.zeros(N, dtype=F64)
    for k in range(T - 1, -1, -1):
        delta = r[k] + gamma * nxt * own[k] - v[k]
        mag = np.abs(r[k]) + np.abs(gamma * nxt * own[k]) + np.abs(v[k]) + np.abs(gamma * lam * nt[k] * last)
        b_last = np.asarray(gamma * lam * nt[k], F64) * b_last + 7 * U * np.asarray(mag, F64)
        # the code object fuses this line (v_fmac_f32: hipcc contracts a * b + c): one rounding, and the restatement follows it
        last = fma(gamma * lam * nt[k], last, delta) if f is F32 else delta + gamma * lam * nt[k] * last
        adv[k], budget[k] = last, b_last
        tot = tot + last
        nxt = v[k]
    ret = adv + v
    if normalize:
        mean = tot / f(T)
        var = np.zeros(N, dtype=f)
        for k in range(T):
            dd = adv[k] - mean
            var = fma(dd, dd, var) if f is F32 else var + dd * dd          # fused as well
        with np.errstate(all="ignore"):
            inv = f(1.0) / (np.sqrt(var / f(T)) + eps)
        adv = (adv - mean) * inv
    return adv, ret, budget


def gae_ref(rewards, vpred, dones, gamma, lam, bootstrap=None, legacy=False, first_starts=None):
    """-> adv: (float64, bound), ret: (float64, bound: adv's + the sum's 2 U)"""
    adv, ret, b = gae_run(rewards, vpred, dones, gamma, lam, bootstrap, legacy, first_starts, False, 0.0, F64)
    return (adv, b), (ret, b + 2 * U * (np.abs(adv) + np.abs(np.asarray(vpred, F64))))


def normalize64(adv, eps):
    """rollout.normalize_per_robot in float64 -> (normalised, the robots' variances)"""
    adv = np.asarray(adv, F64)
    return (adv - adv.mean(axis=0)) / (adv.std(axis=0) + float(F32(eps))), adv.var(axis=0)


MIN_VAR = 1e-6


# ---- seeded inputs, shared by the CPU and the GPU tests: magnitudes mixed over the columns so that a swapped index cannot cancel ------------

def mixed(rng, *shape):
    return f32(rng.standard_normal(shape) * 10.0 ** -(np.arange(shape[-1]) % 4))


def relu_data(m, c, seed=0):
    """-> g [m, c], h [m, c] = relu of a normal draw (about half of it exactly zero)"""
    rng = np.random.RandomState(1000 * c + m + seed)
    return mixed(rng, m, c), f32(np.maximum(rng.standard_normal((m, c)), 0.0))


def head_backward_data(m, c, k, seed=0):
    rng = np.random.RandomState(100000 * k + 1000 * c + m + seed)
    return mixed(rng, m, k), mixed(rng, c, k), f32(np.maximum(rng.standard_normal((m, c)), 0.0))


LOG_STD_BOUNDS = (math.log(0.01), 0.0)       # ppo.LOG_STD_BOUNDS, checked by the CPU test


def uneven_log_std():
    """twelve unequal log-stds over the range the trainer allows"""
    return f32(np.linspace(LOG_STD_BOUNDS[0], LOG_STD_BOUNDS[1], K_ACT)[[5, 0, 11, 3, 8, 1, 10, 6, 2, 9, 4, 7]])


def head_data(m, std=0.125, log_std=None, spread=False, seed=0):
    """-> mean [m, 12], value [m], batch [m, 16] (actions, old log-probability, advantage, return, 0).  The old policy's means are shifted by
    0.08 standard deviations, so part of the ratios leaves [0.8, 1.2]; every seventh advantage is zero, their magnitudes cycle over four
    decades; the last sample is inside the range with a unit advantage; spread: the log-ratios moved by linspace(-20, 20)."""
    rng = np.random.RandomState(7000 + m + seed)
    sd = np.full(K_ACT, float(F32(std))) if log_std is None else np.exp(np.asarray(f32(log_std), F64))
    mean = f32(rng.standard_normal((m, K_ACT)))
    act = f32(mean + sd * rng.standard_normal((m, K_ACT)))
    z_old = (np.asarray(act, F64) - (np.asarray(mean, F64) + 0.08 * sd * rng.standard_normal((m, K_ACT)))) / sd
    old = -0.5 * (z_old * z_old).sum(axis=1) - np.log(sd).sum() - 6.0 * LOG_2PI
    if spread:
        old = old + np.linspace(-20.0, 20.0, m)
    z = (np.asarray(act, F64) - np.asarray(mean, F64)) / sd
    old[m - 1] = -0.5 * (z[m - 1] * z[m - 1]).sum() - np.log(sd).sum() - 6.0 * LOG_2PI - 0.05      # the last sample is live: ratio e^0.05, A = 1
    batch = np.zeros((m, 16), dtype=F32)
    batch[:, :12], batch[:, 12] = act, old
    batch[:, 13] = rng.standard_normal(m) * 10.0 ** -(np.arange(m) % 4)
    batch[::7, 13] = 0.0
    batch[m - 1, 13] = 1.0
    batch[:, 14] = rng.standard_normal(m)
    return mean, f32(rng.standard_normal(m)), batch


def tie_data(m, log_norm, seed=0):
    """The constructed tie: act == mean (the log-probability is exactly log_norm), old log-probability = log_norm (ratio exactly 1), for
    clip = 0, advantages of both signs and zero.  Every fifth sample's old log-probability is one off (ratio e or 1 / e: outside), with the
    same cycle of advantages: a zero advantage outside the range is where `s1 < s2` and `s1 <= s2` part."""
    rng = np.random.RandomState(9000 + m + seed)
    mean = f32(rng.standard_normal((m, K_ACT)))
    batch = np.zeros((m, 16), dtype=F32)
    batch[:, :12], batch[:, 12] = mean, F32(log_norm)
    batch[::5, 12] = F32(log_norm) + np.where(np.arange(0, m, 5) % 2 == 0, F32(1.0), F32(-1.0))
    batch[:, 13] = np.array([1.5, -0.75, 0.0, 0.001, -2.0, 0.0, 3.0], dtype=F32)[np.arange(m) % 7]
    batch[:, 14] = rng.standard_normal(m)
    return mean, f32(rng.standard_normal(m)), batch


def adam_data(n, steps=3, seed=0):
    """-> p, m, v (non-trivial moments for a preset step count), [g per step]"""
    rng = np.random.RandomState(300 + n + seed)
    g = [mixed(rng, n) for _ in range(steps)]
    return f32(rng.standard_normal(n)), f32(0.1 * mixed(rng, n)), f32(0.01 * mixed(rng, n) ** 2), g


def gae_data(T, N, rate, seed=0):
    """-> rewards, vpred [T, N], dones [T, N] bool at `rate`, first_starts [N] bool (random), bootstrap [N]"""
    rng = np.random.RandomState(50 + 1000 * T + N + int(10 * rate) + seed)
    r = f32(rng.uniform(0.1, 1.0, (T, N)) * 10.0 ** -(np.arange(N) % 3))
    v = f32(rng.standard_normal((T, N)))
    d = rng.uniform(size=(T, N)) < rate
    return r, v, d, rng.uniform(size=N) < 0.5, f32(rng.standard_normal(N))


RELU_COLS = (4, 8, 16, 32, 64, 128, 256, 512, 1024)
RELU_ROWS = (1, 31, 32, 33, 65)
HEADB_K, HEADB_COLS, HEADB_ROWS = (12, 1), (4, 16, 64, 256, 512, 1024), (1, 31, 33, 65)
COLSUM_ROWS = (1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 513)
COLSUM_COLS = (1, 15, 16, 17, 255, 256, 257)
HEAD_ROWS = (1, 255, 256, 257, 769, 1025)
SMALL_HEAD_ROWS = (1, 63, 64, 65, 257)
REGRESS_COLS = (4, 16, 48, 60, 64)
ADAM_N = (1, 5, 255, 256, 257, 1023, 1025, 4099)
ADAM_T0 = (0, 999, 99999)
SUMSQ_N = (1, 1023, 1024, 1025, 65537)
GAE_SHAPES = ((1, 1), (2, 1), (5, 2), (7, 5), (3, 255), (3, 256), (3, 257), (16, 33))
GAE_RATES = (0.0, 0.5, 1.0)
