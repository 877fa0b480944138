"""Shared by the randomiser tests and tests/golden/make_golden_randomizer.py: the 31 uniforms behind a row of the randomiser's params
buffer, from the oracle's Philox stream.  orc_uniform takes a 32-bit draw index (blocks below 2^30); the randomiser's two newer blocks
(0x40000000, 0x40000001) lie beyond it, so they come from orc_philox_raw with orc_uniform's own counter and key layout - the same
function either way, which stream_uniform asserts on the draws that both can address."""
import ctypes as C

import numpy as np

from openroborl_amd import _abi, env as envmod


def stream_uniform(L, seed, robot, episode, draw):
    """Draw `draw` (4 * block + word, any block below 2^32) of the stream (seed, robot, episode): a 24-bit fraction in [0, 1)."""
    draw = int(draw)
    ctr = (C.c_uint32 * 4)(int(robot), int(episode), draw >> 2, 0x4F52524C)
    key = (C.c_uint32 * 2)(int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    L.orc_philox_raw(ctr, key)
    u = (ctr[draw & 3] >> 8) / 16777216.0
    if draw < (1 << 32):
        assert u == L.orc_uniform(int(seed), int(robot), int(episode), draw)
    return u


def stream_rows(L, seed, robots, episodes):
    """The params-buffer rows [len(robots), RAND_ROW] (float64) that resets write for the streams (seed, robots[i], episodes[i])."""
    idx = envmod.randomizer_draw_indices()
    U = np.array([[stream_uniform(L, seed, r, e, d) for d in idx] for r, e in zip(robots, episodes)])
    return envmod.randomizer_row(U.reshape(-1, len(idx)))


def load_cases(g):
    """The fixture's cases: name -> (config dict of parameter name -> [lo, hi], rows [N, RAND_ROW], before, after), before / after =
    dicts of record field -> [N, k] read from the reference's robot ahead of and behind the randomiser's call."""
    out = {}
    for name in [str(x) for x in g["cases"]]:
        en, lo, hi = g["%s/enabled" % name], g["%s/lo" % name], g["%s/hi" % name]
        cfg = {p: [float(lo[i]), float(hi[i])] for i, p in enumerate(_abi.RAND_PARAM_NAMES) if en[i]}
        fields = ("STRENGTH", "MASS_RATIO", "INERTIA_RATIO", "KNEE_FRICTION", "LATENCY", "FOOT_MU")
        out[name] = (cfg, g["%s/rows" % name], {f: g["%s/before/%s" % (name, f)] for f in fields}, {f: g["%s/after/%s" % (name, f)] for f in fields})
    return out
