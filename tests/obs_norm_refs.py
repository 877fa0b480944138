"""float64 references, float32 restatements and error bounds of running observation normalisation (csrc/orr_learner.hip:
running_stats_partial_kernel, running_stats_merge_kernel, normalize_rows_kernel; csrc/orr_policy.hip: pack_norm_kernel).  numpy only:
tests/test_obs_norm_refs_cpu.py shows on the CPU that every comparison here passes on the restatement and rejects a seeded defect,
tests/test_gpu_obs_norm.py applies the same comparisons to the device's outputs, tests/test_obs_norm_cpu.py to the torch path.

The bounds are the two rules stated at the top of tests/learner_refs.py, with that module's constants:
  short   (chained roundings + 1) x U x the sum of the terms' magnitudes: the normalised value, the folded bias, the folded forward
          pass's layer 0, and that bound carried through the two layers behind it (first order);
  long    FLOOR_FACTOR x the restatement's own error + SLACK_REL of the group's largest magnitude, one number per group: the merged
          mean and variance (float32 sums of up to 256 rows per partial) and rstd (behind a sqrt).
What the carried bound can and cannot do: it is a worst case (every rounding at its largest and of one sign, absolute values through two
layers), and measured errors sit at 1e-5 of it.  It tells the fold from its absence, from a fold of the weights alone and from a fold with
the wrong table - the tests show each of them beyond it - but not a small arithmetic regression in the fold; that is what the bit-for-bit
comparisons of the packed image and of the folded bias with their restatements are for.
The update's float32 stage (the partials) is restated operation for operation; its float64 merge is restated formula for formula, and a
compiler's choice of fused multiply-adds there can move a result by one float32 unit in rare cases: the long rule covers that, equality
with the restatement is printed by the GPU test and not asserted.
Every reference takes the float32 inputs and the float32 eps the host passes, and widens them.  A restatement's `defect` is never
anything the device runs."""
import numpy as np

from tests import learner_refs as lr
from tests.learner_refs import F32, F64, U, f32, fma

THREADS, PASSES, MERGE_THREADS = 320, 32, 1024      # ORR_RUNNING_STATS_THREADS, ORR_RUNNING_STATS_PASSES, kMergeThreads
EPS = F32(1e-2)                                     # ppo.NORM_EPS as the kernel receives it
GROUPS = ("mean", "var", "rstd")
COL_OFFSET, COL_CONST, COL_TINY = 0, 1, 2           # the three column kinds every data set here carries, by index


def pass_rows(d):
    return THREADS // (d // 4)


def block_rows(d):
    return PASSES * pass_rows(d)


def columns(n, d, seed, shift=0.0):
    """[n, d] float32: column 0 of mean 1000 and std 0.01, column 1 constant, column 2 of magnitude 1e-4, every other one offset + scale x a
    standard normal with its own offset in [-2, 2] and scale in [0.05, 3].  shift moves every mean (a later batch of another distribution)."""
    rng = np.random.RandomState(seed)
    off, scale = rng.uniform(-2.0, 2.0, d), np.exp(rng.uniform(np.log(0.05), np.log(3.0), d))
    x = (off + shift) + scale * rng.standard_normal((n, d))
    x[:, COL_OFFSET] = 1000.0 + shift + 0.01 * rng.standard_normal(n)
    x[:, COL_CONST] = 0.67
    x[:, COL_TINY] = 1e-4 * rng.standard_normal(n)
    return f32(x)


def fresh(d):
    """the identity record the host initialises"""
    return {"count": 0, "mean": np.zeros(d, F32), "var": np.ones(d, F32), "rstd": np.ones(d, F32), "batches": 0}


# ---- float64 references ----------------------------------------------------------------------------------------------------------------------

def moments64(x):
    """two-pass (count, mean, M2) of the rows of x"""
    x = np.asarray(x, F64)
    mean = x.mean(axis=0)
    return x.shape[0], mean, ((x - mean) ** 2).sum(axis=0)


def chan64(a, b):
    """the parallel formula on (count, mean, M2) triples; count 0 on the left: the right replaces it"""
    (na, ma, qa), (nb, mb, qb) = a, b
    if na == 0:
        return nb, mb, qb
    n, delta = na + nb, mb - ma
    return n, ma + delta * nb / n, qa + qb + delta * delta * (na * nb / n)


def rstd64(var, eps=EPS):
    return 1.0 / (np.sqrt(np.asarray(var, F64)) + F64(eps))


def stats64(batches, eps=EPS):
    """the record after the batches, one after the other: float64 moments of each, merged by chan64 = the moments of their concatenation"""
    acc = (0, None, None)
    for x in batches:
        acc = chan64(acc, moments64(x))
    n, mean, m2 = acc
    var = m2 / n
    return {"count": n, "mean": mean, "var": var, "rstd": rstd64(var, eps)}


def normalize64(x, mean, rstd):
    return (np.asarray(x, F64) - np.asarray(mean, F64)) * np.asarray(rstd, F64)


def fold64(w, b, mean, rstd):
    """-> (diag(rstd) W, b - (mean rstd) W) of the float32 inputs, in float64"""
    w, b, mean, rstd = (np.asarray(v, F64) for v in (w, b, mean, rstd))
    return rstd[:, None] * w, b - (mean * rstd) @ w


def mlp64(p, net, x):
    """the float64 net model/<net>* on x: (layer-0 pre-activation, output)"""
    g = lambda k: np.asarray(p[k], F64)     # noqa: E731
    z0 = x @ g("model/%s_fc0/w:0" % net) + g("model/%s_fc0/b:0" % net)
    h1 = np.maximum(np.maximum(z0, 0.0) @ g("model/%s_fc1/w:0" % net) + g("model/%s_fc1/b:0" % net), 0.0)
    return z0, h1 @ g("model/%s/w:0" % net) + g("model/%s/b:0" % net)


# ---- float32 restatements in the kernels' operation order ----------------------------------------------------------------------------------------

def partials_restate(x, defect=None):
    """running_stats_partial_kernel: [blocks, 2, d] shifted sums around the batch's first row.  A thread adds its rows (every pass_rows-th of
    the workgroup's) in order, the square by fmaf; thread 0 of a column group adds the row groups in order.  Rows beyond n add nothing, which
    adding a zero restates.  defect "naive": no shift, i.e. plain sums of x and x^2 in float32."""
    x = f32(x)
    n, d = x.shape
    side, rows = pass_rows(d), block_rows(d)
    blocks = (n + rows - 1) // rows
    shift = np.zeros(d, F32) if defect == "naive" else x[0]
    e = np.zeros((blocks * rows, d), F32)
    e[:n] = x - shift
    e = e.reshape(blocks, PASSES, side, d)
    s1, s2 = np.zeros((blocks, side, d), F32), np.zeros((blocks, side, d), F32)
    for p in range(PASSES):
        s1 = s1 + e[:, p]
        s2 = fma(e[:, p], e[:, p], s2)
    a1, a2 = s1[:, 0], s2[:, 0]
    for k in range(1, side):
        a1, a2 = a1 + s1[:, k], a2 + s2[:, k]
    return np.stack((a1, a2), axis=1)


def merge_restate(rec, partials, x, eps=EPS, defect=None):
    """running_stats_merge_kernel on a record {count, mean, var, rstd}: 1024 / d consecutive ranges of the partials, each added in index
    order in float64, the ranges in their order; the batch's moments and the merge in float64; float32 results, rstd from the float32 var.
    defects: "naive" (the partials are unshifted: M2 = S2 - S1^2 / n with everything up to here in float32), "no_delta" (the merge drops
    delta^2 n_a n_b / n), "batch_weight" (the merge weighs the record by the batches behind it and the batch by 1, not by rows),
    "rstd_inside" (1 / sqrt(var + eps))."""
    x = f32(x)
    n, d = x.shape
    blocks = partials.shape[0]
    segs = MERGE_THREADS // d
    per = (blocks + segs - 1) // segs
    S = np.zeros((2, d), F64)
    for seg in range(segs):
        part = np.asarray(partials[seg * per:min(blocks, (seg + 1) * per)], F64)
        S = S + (np.cumsum(part, axis=0)[-1] if len(part) else 0.0)
    nb = F64(n)
    if defect == "naive":
        s1, s2 = f32(S[0]), f32(S[1])
        mean = (s1 / F32(n)).astype(F64)
        m2 = np.maximum(s2 - s1 * s1 / F32(n), F32(0.0)).astype(F64)
    else:
        mean = x[0].astype(F64) + S[0] / nb
        m2 = np.maximum(S[1] - S[0] * S[0] / nb, 0.0)
    tot, na = nb, int(rec["count"])
    if na > 0:
        a, mean_a = F64(na), rec["mean"].astype(F64)
        if defect == "batch_weight":
            a, nb = F64(rec["batches"]), F64(1.0)
        delta, tot = mean - mean_a, a + nb
        cross = 0.0 if defect == "no_delta" else delta * delta * (a * nb / tot)
        m2 = rec["var"].astype(F64) * a + (m2 if defect != "batch_weight" else m2 / F64(n)) + cross
        mean = mean_a + delta * (nb / tot)
    var = f32(m2 / tot)
    rstd = 1.0 / np.sqrt(var.astype(F64) + F64(eps)) if defect == "rstd_inside" else 1.0 / (np.sqrt(var.astype(F64)) + F64(eps))
    return {"count": max(na, 0) + n, "mean": f32(mean), "var": var, "rstd": f32(rstd), "batches": rec.get("batches", 0) + 1}


def update_restate(rec, x, eps=EPS, defect=None):
    """orr_running_stats_update"""
    return merge_restate(rec, partials_restate(x, defect if defect == "naive" else None), x, eps, defect)


def stats_restate(batches, eps=EPS, defect=None):
    """the record after the batches, from the identity"""
    rec = fresh(batches[0].shape[1])
    for x in batches:
        rec = update_restate(rec, x, eps, defect)
    return rec


def normalize_restate(x, mean, rstd):
    """normalize_rows_kernel: a subtraction and a multiplication, both rounded"""
    return (f32(x) - f32(mean)) * f32(rstd)


def fold_restate(w, b, mean, rstd, defect=None):
    """pack_norm_kernel, unpacked: (rstd_i W_ij in float32, b_j - the fmaf chain over i of (mean_i rstd_i) W_ij from +0).
    defects: "bias_left" (the weights are scaled, the bias is b), "mean_only" (mean where mean * rstd belongs)."""
    w, b, mean, rstd = f32(w), f32(b), f32(mean), f32(rstd)
    if defect == "bias_left":
        return rstd[:, None] * w, b.copy()
    ms = mean if defect == "mean_only" else mean * rstd
    s = np.zeros(w.shape[1], F32)
    for i in range(w.shape[0]):
        s = fma(ms[i], w[i], s)
    return rstd[:, None] * w, b - s


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------------

def stats_ratios(got, batches, eps=EPS):
    """{group: largest error / the long bound} of a record against the float64 moments of the batches' concatenation; the count must be the
    integer sum (inf otherwise)"""
    ref, rest = stats64(batches, eps), stats_restate(batches, eps)
    out = {g: lr.ratio_of(got[g], ref[g], lr.long_bound(rest[g], ref[g])) for g in GROUPS}
    out["count"] = 0.0 if int(got["count"]) == ref["count"] else np.inf
    return out


def normalize_bound(x, mean, rstd):
    """2 roundings: the difference (relative to itself), the product"""
    return 3 * U * np.abs(normalize64(x, mean, rstd))


def fold_bias_bound(w, b, mean, rstd):
    """k + 2 roundings: mean * rstd, the k fmafs of the chain, the subtraction; terms |b_j| and |mean_i rstd_i W_ij|"""
    w, b, mean, rstd = (np.asarray(v, F64) for v in (w, b, mean, rstd))
    return (w.shape[0] + 3) * U * (np.abs(b) + np.abs(mean * rstd) @ np.abs(w))


def folded_forward_bound(p, net, x, mean, rstd):
    """[n, outputs]: the error budget of the forward kernel's model/<net>* output on RAW x [n, k] with the folded layer 0 against mlp64 on
    normalize64(x).  Layer 0's pre-activation is sum_i x_i (rstd_i W_ij) + b'_j: one rounding of the scaled weight, the k fmafs of the
    matrix-core chain, the bias addition -> k + 2 roundings over the terms |x_i rstd_i W_ij| and |b'_j|, plus b'_j's own budget
    (fold_bias_bound).  Carried on, first order, ReLU being 1-Lipschitz: a layer of fan-in K adds (K + 2) U (sum |h_i W_ij| + |b_j|) to
    sum_i (budget of h_i) |W_ij|."""
    g = lambda k: np.asarray(p[k], F64)     # noqa: E731
    x, mean, rstd = (np.asarray(v, F64) for v in (x, mean, rstd))
    w0, b0 = g("model/%s_fc0/w:0" % net), g("model/%s_fc0/b:0" % net)
    k = w0.shape[0]
    wf, bf = fold64(w0, b0, mean, rstd)
    e = (k + 3) * U * (np.abs(x) @ np.abs(wf) + np.abs(bf)) + fold_bias_bound(w0, b0, mean, rstd)
    h = np.maximum(normalize64(x, mean, rstd) @ w0 + b0, 0.0)
    for name in ("model/%s_fc1" % net, "model/%s" % net):
        w, b = g(name + "/w:0"), g(name + "/b:0")
        e = e @ np.abs(w) + (w.shape[0] + 3) * U * (np.abs(h) @ np.abs(w) + np.abs(b))
        h = np.maximum(h @ w + b, 0.0)
    return e
