"""Compile-only (no GPU): the order of memory instructions at the end of the step kernel and in the reset kernel.

Loads, stores and atomics of a wave share one in-order counter (vmcnt), so a load that is waited for behind a store or an atomic sits
out that one's whole round trip.  Past its sub-step loop the step kernel therefore issues every load first - the reference frames of
the step, the cold-table constants and the frames of an inline auto-reset - and every store and atomic at the very end, and the four
target times are picked by register selects, not by a vector load of the kernel arguments (orr_task.h, target_frame_steps).  Checked on
the listings of the one-wave and the two-wave unit, compiled with line tables as tools/isa_lines.py compiles them:

  1. no load instruction is attributed to target_frame_steps, and its selects are there;
  2. past the sub-step loop of orr_step_kernel<0, 1> / <0, 2>, and in orr_reset_kernel<false, false>, no global / flat load follows a
     global store or atomic in the listing;
  3. exactly one `s_waitcnt vmcnt` follows the first store of orr_step_kernel<0, 1>: the one wait for the episode-log slot and the
     launch ticket, two returning atomics issued back to back (in the two-wave unit: no wait and no load between the two).

"Past the sub-step loop" = every instruction behind the loop's back edge that is not one of the loop's own side blocks
(isa_stats.loop_side_blocks: rare paths that the block placement puts there).

The same checks were run once against the parent's listing (the tree before this order) and fail there: its selects over the four
kernel arguments (there written out in orr_env_kernels.h and in the reset) each carry a global_load_dword with an `s_waitcnt
vmcnt(0)` right behind it; the loads of the reset's target time, frames and warm-up pose follow the episode-log atomic and the
reward / done stores, and in the reset kernel the frame loads' wait follows the store of ring entry #1; eight `s_waitcnt vmcnt`
follow the first store of orr_step_kernel<0, 1>.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lines  # noqa: E402
import isa_stats  # noqa: E402

UNITS = ("one", "two")
RESET_KERNEL = "_Z16orr_reset_kernelILb0ELb0E"
TASK_H = os.path.join(ROOT, "openroborl_amd", "csrc", "orr_task.h")
HELPER = "target_frame_steps"


def is_load(t):
    return re.match(r"^(global|flat|buffer|scratch)_load", t) is not None


def is_global_load(t):
    return re.match(r"^(global|flat)_load", t) is not None


def is_store_or_atomic(t):
    return re.match(r"^(global|flat)_(store|atomic)", t) is not None


def is_vm_wait(t):
    return t.startswith("s_waitcnt") and "vmcnt" in t


def helper_lines():
    """(first, last) source line of target_frame_steps in orr_task.h: from its signature to the closing brace in column 0"""
    src = open(TASK_H).read().split("\n")
    first = next(i for i, l in enumerate(src) if re.match(r"^__device__ .*\b%s\(const orr_config" % HELPER, l))
    last = next(i for i in range(first, len(src)) if src[i] == "}")
    return first + 1, last + 1


@pytest.fixture(scope="module")
def listings():
    """{unit: the unit's listing with line tables}, after checking that the line tables left the step kernel's instruction count alone"""
    names = ("env", "w2")
    plain = isa_stats.compile_units(units=names)
    dbg = isa_stats.compile_units(["-gline-tables-only"], units=names)
    assert len(plain) == len(dbg) == 2
    out = {}
    for name, p, d in zip(UNITS, plain, dbg):
        sym = isa_stats.STEP_KERNELS[isa_lines.UNITS[name]][0]
        kp, kd = isa_stats.parse_kernel(p, sym), isa_stats.parse_kernel(d, sym)
        assert kp is not None and kd is not None, sym
        if name == "one":       # (the two-wave unit's spill code moves by a few instructions with the line tables: tools/isa_lines.py)
            assert len(kp[0]) == len(kd[0])
        out[name] = d
    return out


def step_end(lines, name):
    """[(instruction, (file, line))] of the step kernel past its sub-step loop, in listing order"""
    sym = isa_stats.STEP_KERNELS[isa_lines.UNITS[name]][0]
    insts, labels, locs, _ = isa_stats.parse_kernel(lines, sym)
    files = isa_lines.file_table(lines)
    lo, hi = isa_stats.substep_loop(insts, labels)
    assert hi - lo > 2000, "not the sub-step loop"
    side = set(isa_stats.loop_side_blocks(insts, labels, lo, hi))
    return [(insts[i], (files.get(locs[i][0], "?"), locs[i][1]) if locs[i] else ("?", 0)) for i in range(hi + 1, len(insts)) if i not in side]


def whole_kernel(lines, sym):
    k = isa_stats.parse_kernel(lines, sym)
    assert k is not None, sym
    files = isa_lines.file_table(lines)
    insts, locs = k[0], k[2]
    return [(insts[i], (files.get(locs[i][0], "?"), locs[i][1]) if locs[i] else ("?", 0)) for i in range(len(insts))]


def loads_behind_stores(seq):
    """the global / flat loads of a listing excerpt that come after its first store or atomic"""
    first = next((i for i, (t, _) in enumerate(seq) if is_store_or_atomic(t)), None)
    assert first is not None, "no store in the excerpt"
    return first, [(t, w) for t, w in seq[first:] if is_global_load(t)]


@pytest.mark.parametrize("name", UNITS)
def test_no_load_is_attributed_to_the_target_time_helper(listings, name):
    lo, hi = helper_lines()
    assert 5 <= hi - lo <= 12, (lo, hi)
    sym = isa_stats.STEP_KERNELS[isa_lines.UNITS[name]][0]
    kernels = [whole_kernel(listings[name], sym)] + ([whole_kernel(listings[name], RESET_KERNEL)] if name == "one" else [])
    for seq in kernels:
        own = [t for t, (f, ln) in seq if f == "orr_task.h" and lo <= ln <= hi]
        print("%s: %d instructions attributed to %s: %s" % (name, len(own), HELPER, sorted({t.split()[0] for t in own})))
        assert not [t for t in own if is_load(t)], [t for t in own if is_load(t)]
        assert len([t for t in own if t.startswith("v_cndmask")]) >= 3          # the selects over the four scalars are there
        # the scalars themselves arrive by scalar loads of the kernel arguments, if any load is attributed to the helper at all
        assert all(t.startswith("s_load") for t in own if "load" in t.split()[0])


@pytest.mark.parametrize("name", UNITS)
def test_no_load_follows_a_store_or_atomic_past_the_substep_loop(listings, name):
    seq = step_end(listings[name], name)
    first, bad = loads_behind_stores(seq)
    print("%s: %d instructions past the loop, first store at +%d, %d global loads in front of it" % (
        name, len(seq), first, sum(1 for t, _ in seq[:first] if is_global_load(t))))
    assert sum(1 for t, _ in seq[:first] if is_global_load(t)) >= 2 * 26          # the frames of the step and of the inline reset
    assert not bad, bad[:4]


def test_no_load_follows_a_store_or_atomic_in_the_reset_kernel(listings):
    seq = whole_kernel(listings["one"], RESET_KERNEL)
    first, bad = loads_behind_stores(seq)
    assert sum(1 for t, _ in seq[:first] if is_global_load(t)) >= 26
    assert not bad, bad[:4]


def test_one_wait_follows_the_first_store_of_the_one_wave_step_kernel(listings):
    """The one-wave unit only: the two-wave unit's 256 registers make it reload spilled values from scratch between the record's
    stores, and scratch loads count on vmcnt too, so its stores carry waits of their own (they did before this order as well)."""
    seq = step_end(listings["one"], "one")
    first = next(i for i, (t, _) in enumerate(seq) if is_store_or_atomic(t))
    waits = [(t, w) for t, w in seq[first:] if is_vm_wait(t)]
    returning = [t for t, _ in seq[first:] if t.startswith("global_atomic") and " sc0" in t]
    print("waits behind the first store: %s; returning atomics: %d" % (waits, len(returning)))
    assert len(returning) == 2                     # the episode-log slot and the launch ticket
    assert len(waits) == 1, waits
    at = next(i for i, (t, _) in enumerate(seq) if is_vm_wait(t) and i >= first)
    assert sum(1 for t, _ in seq[first:at] if t.startswith("global_atomic") and " sc0" in t) == 2      # the one wait is behind both


def test_the_two_returning_atomics_of_the_two_wave_step_kernel_are_issued_back_to_back(listings):
    seq = step_end(listings["two"], "two")
    at = [i for i, (t, _) in enumerate(seq) if t.startswith("global_atomic") and " sc0" in t]
    assert len(at) == 2
    assert not [t for t, _ in seq[at[0]:at[1]] if is_vm_wait(t) or is_global_load(t)]
