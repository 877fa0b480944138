"""The GPU side of the measurement tools stays runnable: tools/laikago_identify.py's HipProbe (four candidates in the four robot-type
slots of one launch) on the two tables whose results are quoted in DESIGN.md section 7.2, and the development build of the env kernels
that the timing tools share (tools/dev_build.py): its per-wave timeline and phase timers."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_identification_probe_separates_the_round_4_table_from_the_identified_one():
    """One launch group = [round-4 table, the recorded chosen candidate, round-4 table, chosen candidate] under the fit policy laikago_trot,
    200 steps, 64 robots each: the slots do not leak into each other (the same table in two slots gives the same level - not the same bits:
    the robots of two slots have different global indices, i.e. other start phases) and the chosen candidate keeps walking where round 4's
    table has long fallen."""
    import laikago_identify as li
    rec = json.load(open(os.path.join(ROOT, "profiles", "r05_laikago_identify.json")))
    r4, ch = li.shipped_theta(), rec["chosen"]["theta"]
    probe = li.HipProbe(64)
    out = probe.run_group("laikago_trot", "laikago_trot", [r4, ch, dict(r4), dict(ch)], li.config_overrides(r4), steps=200)
    assert abs(out[0]["len"] - out[2]["len"]) < 45 and abs(out[1]["len"] - out[3]["len"]) < 20        # same table, another slot: same level
    assert out[2]["F"] <= 0.5 and out[3]["F"] >= 0.8
    assert out[0]["len"] < 160 and out[0]["F"] <= 0.5                  # round 4's table: mean survival ~130 steps
    assert out[1]["len"] > 170 and out[1]["F"] >= 0.8                  # the identified table: measured 182 of 200 steps, 0.9 still up (the warm-up starts are the weaker ones)


WAVE_TIMELINE_CHILD = r"""
import ctypes as C, os, sys
sys.path.insert(0, %r)
import dev_build
L = dev_build.load(*dev_build.PHASE_TIMERS)          # before anything loads the library: ORR_LIB_PATH
import torch
from openroborl_amd.env import VecQuadrupedEnv


def two_steps():
    env = VecQuadrupedEnv(task_name="imitation_learning_laikago", num_robot=18, seed=0, auto_reset=False)
    env.reset()
    dev_build.wave_rows(L, 5)                         # allocates; the launches after it are recorded
    act = torch.zeros(18, 12, device=env.device)
    for _ in range(2):
        env.step(act)
    rows = dev_build.wave_rows(L, 5)
    env.close()
    print("rows", rows.tolist())
    assert (rows[:, 0] > 0).all() and (rows[:, 1] > rows[:, 0]).all() and (rows[:, 2] > 0).all(), rows
    fin = dev_build.decode_slot(rows)[0]
    assert (fin == 0).all() and (fin[4] & 0b1100) == 0, fin
    return rows


cyc = (C.c_longlong * 40)()
L.orr_debug_phase_cycles(cyc, 1)
one = two_steps()
L.orr_debug_phase_cycles(cyc, 1)
print("phase cycles", list(cyc[:16]))
assert all(v > 0 for v in cyc[:16]), list(cyc)
os.environ["ORR_STEP_WAVES_PER_EU"] = "2"            # read by orr_create: the two-wave unit's kernel from here on
two = two_steps()
assert (two[:, 0] > one[:, 1].max()).all()           # rows of the second env's launches, not leftovers of the first
L.orr_debug_phase_cycles(cyc, 1)
assert not any(cyc[:16]), list(cyc)                  # the two-wave unit carries no phase timers: it WAS that unit's kernel
print("TIMELINE OK")
"""


def test_phase_timer_build_records_the_wave_timeline_from_both_step_units():
    """The -DORR_PHASE_TIMERS library (tools/dev_build.py, built by __graft_entry__.build) in a fresh process, since ORR_LIB_PATH has to
    be set before the library loads.  18 robots = five waves, the last with two padding lane groups: the smallest batch with a partial
    wave.  After two steps without auto-reset every wave's timeline row (orr_debug_wave_times: the one timeline, which the phase timers'
    build implies) has a start, a later end, shader cycles and no finished robot - the padding groups of the fifth wave included - and
    the instrumented wave has non-zero cycle totals in the phase slots 0..15.  Then the same with ORR_STEP_WAVES_PER_EU=2: the step
    kernel of the two-wave unit, which does not see the timers, writes its rows through the same KParams the main unit built."""
    import subprocess
    out = subprocess.run([sys.executable, "-c", WAVE_TIMELINE_CHILD % os.path.join(ROOT, "tools")], capture_output=True, text=True, timeout=900,
                         env={k: v for k, v in os.environ.items() if not k.startswith("ORR_")})
    assert out.returncode == 0 and "TIMELINE OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
