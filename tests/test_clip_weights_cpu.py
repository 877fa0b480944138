"""Weighted and failure-adaptive clip sampling without a GPU: the host statements of the draw rule and of the curriculum's update
(openroborl_amd.env_draws), the argument validators (openroborl_amd.env_spec), and the C-ABI's declarations against the loader."""
import os
import re

import numpy as np
import pytest

from openroborl_amd import _abi, _lib, env_draws as ed, env_spec as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 24
NEW_ENTRIES = ("orr_set_clip_weights", "orr_get_clip_thresholds", "orr_sizeof_clip_curriculum", "orr_set_clip_curriculum",
               "orr_clip_curriculum_update")


def boundary_draws(cum):
    """every threshold, its predecessor, 0 and 2^24 - 1, as valid 24-bit integers"""
    cum = np.asarray(cum, dtype=np.int64)
    m = np.concatenate([cum, cum - 1, [0, ONE - 1]])
    return np.unique(m[(m >= 0) & (m < ONE)])


@pytest.mark.parametrize("n", range(1, 17))
def test_uniform_thresholds_pick_the_integer_rule(n):
    cum = ed.clip_thresholds_uniform(n)
    assert cum[0] == 0 and cum[-1] == ONE and len(cum) == n + 1 and (np.diff(cum) > 0).all()
    m = boundary_draws(cum)
    np.testing.assert_array_equal(ed.clip_draw_weighted(m, cum), ed.clip_draw_index(m, n))
    rng = np.random.RandomState(n)
    m = rng.randint(0, ONE, 4096)
    np.testing.assert_array_equal(ed.clip_draw_weighted(m, cum), ed.clip_draw_index(m, n))


@pytest.mark.parametrize("w", [1.0, 0.25, 3.0, 0.1, 0.7])
def test_equal_weights_give_the_uniform_thresholds(w):
    for n in range(1, 17):
        np.testing.assert_array_equal(ed.clip_thresholds([w] * n), ed.clip_thresholds_uniform(n))


def test_zero_weight_entries_get_empty_intervals():
    cum = ed.clip_thresholds([1.0, 0.0, 2.5, 0.5])
    np.testing.assert_array_equal(cum, [0, ONE // 4, ONE // 4, ONE // 4 + 5 * ONE // 8, ONE])
    m = np.concatenate([boundary_draws(cum), np.random.RandomState(0).randint(0, ONE, 10000)])
    k = ed.clip_draw_weighted(m, cum)
    assert set(k.tolist()) == {0, 2, 3}
    # leading and trailing zeros: the first interval with room takes m = 0, the last one 2^24 - 1
    cum = ed.clip_thresholds([0.0, 1.0, 1.0, 0.0])
    np.testing.assert_array_equal(cum, [0, 0, ONE // 2, ONE, ONE])
    np.testing.assert_array_equal(ed.clip_draw_weighted([0, ONE // 2 - 1, ONE // 2, ONE - 1], cum), [1, 1, 2, 2])


def test_thresholds_are_monotone_and_end_at_one():
    rng = np.random.RandomState(7)
    for _ in range(200):
        n = int(rng.randint(1, 17))
        w = rng.uniform(0.0, 10.0, n) * (rng.uniform(size=n) > 0.3)
        if not w.sum() > 0:
            w[0] = 1.0
        cum = ed.clip_thresholds(w)
        assert cum[0] == 0 and cum[-1] == ONE and (np.diff(cum) >= 0).all() and len(cum) == n + 1
        assert (np.diff(cum)[w.astype(np.float32) == 0] == 0).all()           # a zero weight: an empty interval
        # the interval lengths are the probabilities to one count each
        p = w.astype(np.float32).astype(np.float64)
        np.testing.assert_allclose(np.diff(cum), ONE * p / p.sum(), atol=1.0, rtol=0)


def test_weight_validators_refuse_what_the_abi_refuses():
    sets = {"laikago": [0, 1, 2, 3]}
    assert es.clip_weights_spec(None, sets) == {"laikago": None}
    np.testing.assert_array_equal(es.clip_weights_spec([1, 0, 2.5, 0.5], sets)["laikago"], np.float32([1, 0, 2.5, 0.5]))
    for bad in ([1, 2, 3], [1, 2, 3, 4, 5], [1, -1, 1, 1], [1, float("nan"), 1, 1], [1, float("inf"), 1, 1], [0, 0, 0, 0], "1,2,3,4", 3.0,
                [True, 1, 1, 1], [[1, 1, 1, 1]], {"mini_cheetah": [1, 1, 1, 1]}):
        with pytest.raises(ValueError):
            es.clip_weights_spec(bad, sets)
    mixed = {"laikago": [0, 1], "mini_cheetah": [2]}
    got = es.clip_weights_spec({"laikago": [1, 3]}, mixed)
    np.testing.assert_array_equal(got["laikago"], np.float32([1, 3]))
    assert got["mini_cheetah"] is None
    with pytest.raises(ValueError):
        es.clip_weights_spec([1, 3], mixed)           # a list is for every robot: the mini-cheetah's set has one clip


def test_curriculum_validators_refuse_what_the_abi_refuses():
    sets = {"laikago": [0, 1, 2, 3]}
    assert es.clip_curriculum_spec(None, sets) is None
    s = es.clip_curriculum_spec((0.2, 0.1), sets, default_ref=600.0)
    assert (s.alpha, s.eps, s.metric) == (np.float32(0.2), np.float32(0.1), _abi.CLIP_METRICS.index("length"))
    assert list(s.ref)[:4] == [600.0] * 4
    s = es.clip_curriculum_spec({"alpha": 1.0, "eps": 0.0, "metric": "return", "ref": [10.0, 20.0, 30.0, 40.0]}, sets)
    assert s.metric == 1 and list(s.ref)[:4] == [10.0, 20.0, 30.0, 40.0]
    assert es.clip_curriculum_spec((0.5, 0.5, "step_reward"), sets).ref[2] == 1.0
    mixed = {"laikago": [0, 1], "mini_cheetah": [2]}
    s = es.clip_curriculum_spec({"alpha": 0.5, "eps": 0.5, "ref": {"laikago": [100.0, 200.0], "mini_cheetah": 300.0}}, mixed)
    assert list(s.ref)[:3] == [100.0, 200.0, 300.0]
    for bad in ((0.0, 0.1), (1.5, 0.1), (float("nan"), 0.1), (0.2, -0.1), (0.2, 1.1), (0.2, float("nan")), (0.2, 0.1, "speed"), (0.2,), 0.2,
                {"alpha": 0.2}, {"alpha": 0.2, "eps": 0.1, "beta": 1}, {"alpha": 0.2, "eps": 0.1, "ref": 0.0},
                {"alpha": 0.2, "eps": 0.1, "ref": -1.0}, {"alpha": 0.2, "eps": 0.1, "ref": float("inf")},
                {"alpha": 0.2, "eps": 0.1, "ref": float("nan")}, {"alpha": 0.2, "eps": 0.1, "ref": [1.0, 2.0]},
                {"alpha": 0.2, "eps": 0.1, "ref": {"mini_cheetah": 1.0}}, {"alpha": 0.2, "eps": 0.1, "ref": {"laikago": [1.0, 2.0]}}):
        with pytest.raises(ValueError):
            es.clip_curriculum_spec(bad, sets, default_ref=600.0)
    with pytest.raises(ValueError):
        es.clip_curriculum_spec((0.2, 0.1), sets)     # the length metric without a ref and without the env's default
    assert _abi.OrrClipCurriculum.ref.size == 4 * _abi.MAX_CLIPS


def test_episode_score_rounds_and_clamps():
    q = ed.clip_episode_score([0.0, 300.0, 600.0, 900.0, -5.0, float("nan"), 1.0], 600.0)
    np.testing.assert_array_equal(q, [0, 32768, 65536, 65536, 0, 0, int(np.floor(65536.0 / 600.0 + 0.5))])
    assert ed.clip_episode_score(3.0, 0.0) == 65536 and ed.clip_episode_score(0.0, 0.0) == 0     # inf clamps, 0 / 0 = NaN scores 0


def test_curriculum_step_on_hand_computed_cases():
    Z = np.zeros(_abi.MAX_CLIPS)
    sets = {"laikago": [0, 1]}
    # alpha = 1, eps = 0.1, scores 1 and 0: f = (0, 1), p = (0.05, 0.95)
    n, S = Z.copy(), Z.copy()
    n[:2], S[:2] = 5, (5 * 65536, 0)
    ema, th = ed.clip_curriculum_step(Z, n, S, sets, 1.0, 0.1)
    np.testing.assert_array_equal(ema[:2], [1.0, 0.0])
    np.testing.assert_allclose(np.diff(th["laikago"]) / ONE, [0.05, 0.95], atol=1e-7, rtol=0)
    assert th["laikago"][0] == 0 and th["laikago"][-1] == ONE
    # a clip without episodes keeps its EMA; the other one moves by alpha
    n, S = Z.copy(), Z.copy()
    n[0], S[0] = 4, 4 * 32768
    start = Z.copy()
    start[:2] = 0.25, 0.75
    ema, th = ed.clip_curriculum_step(start, n, S, sets, 0.5, 0.0)
    np.testing.assert_array_equal(ema[:2], [0.5 * 0.25 + 0.5 * 0.5, 0.75])
    np.testing.assert_allclose(np.diff(th["laikago"]) / ONE, [0.625 / 0.875, 0.25 / 0.875], atol=1e-7, rtol=0)
    # all EMAs at 1: uniform, whatever eps; a set of one clip gets no thresholds
    ones = Z.copy()
    ones[:4] = 1.0
    ema, th = ed.clip_curriculum_step(ones, Z, Z, {"laikago": [0, 1, 2], "mini_cheetah": [3]}, 0.3, 0.2)
    np.testing.assert_array_equal(th["laikago"], ed.clip_thresholds_uniform(3))
    assert "mini_cheetah" not in th and (ema == ones).all()
    # eps = 1: uniform to a count; a clip listed twice takes two shares
    ema, th = ed.clip_curriculum_step(start, Z, Z, {"laikago": [0, 1, 1]}, 0.3, 1.0)
    np.testing.assert_allclose(th["laikago"], ed.clip_thresholds_uniform(3), atol=1, rtol=0)
    ema, th = ed.clip_curriculum_step(start, Z, Z, {"laikago": [0, 1, 1]}, 0.3, 0.0)
    np.testing.assert_allclose(np.diff(th["laikago"]) / ONE, np.array([0.75, 0.25, 0.25]) / 1.25, atol=1e-7, rtol=0)


def test_header_still_says_abi_5_and_the_loader_has_every_new_prototype():
    with open(os.path.join(ROOT, "include", "openroborl_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+ORR_ABI_VERSION\s+5\b", hdr) and _abi.ABI_VERSION == 5
    declared = set(re.findall(r"^int32_t\s+(orr_[a-z_]*clip[a-z_]*)\s*\(", hdr, flags=re.M))
    assert set(NEW_ENTRIES) <= declared
    with open(_lib.__file__) as f:
        loader = f.read()
    for name in sorted(declared):
        assert name in _lib.EXPORTS, name
        assert "L.%s.restype = C.c_int32" % name in loader, name
    for i, name in enumerate(_abi.CLIP_METRICS):
        assert re.search(r"#define\s+ORR_CLIP_METRIC_%s\s+%d\b" % (name.upper(), i), hdr), name
    L = _lib.load()
    for name in NEW_ENTRIES:
        assert hasattr(L, name), name
    assert L.orr_sizeof_clip_curriculum() == _abi.C.sizeof(_abi.OrrClipCurriculum) == 12 + 4 * _abi.MAX_CLIPS


def test_null_handles_are_refused_without_a_device():
    L = _lib.load()
    w = (_abi.C.c_float * 2)(1.0, 1.0)
    assert L.orr_set_clip_weights(None, 0, w, 2) < 0 and b"orr_set_clip_weights" in L.orr_last_error()
    assert L.orr_set_clip_curriculum(None, None) < 0 and b"orr_set_clip_curriculum" in L.orr_last_error()
    assert L.orr_clip_curriculum_update(None, None, None) < 0 and b"orr_clip_curriculum_update" in L.orr_last_error()
    assert L.orr_get_clip_thresholds(None, 0, None, None) < 0 and b"orr_get_clip_thresholds" in L.orr_last_error()
