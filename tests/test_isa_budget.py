"""Compile-only (no GPU): the instruction budget of the step kernel's sub-step loop.

The step kernel is bound by the instruction issue of a lone wave, so the static size of the sub-step loop is
what a change of the loop is judged by before it is measured.  The yardstick is the tree before the fused subtree sums
(profiles/r07_isa_stats.txt): 3213 instructions in the loop of the one-wave unit, 3299 in the two-wave unit's, no spilled VGPR / no
scratch access in the loop of the one-wave and the friction-anchor unit, 26 spilled VGPRs / one scratch access in the two-wave unit's.
profiles/r08_isa_stats.txt records what the tree reached; this test asserts "below the parent".
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lines  # noqa: E402
import isa_stats  # noqa: E402

PARENT_LOOP = {"one": 3213, "two": 3299}
PARENT_SPILLED_VGPRS = {"one": 0, "two": 26, "anchor": 0}
PARENT_LOOP_SCRATCH = {"one": 0, "two": 1, "anchor": 0}


@pytest.fixture(scope="module")
def units():
    """{unit: (instructions of the step kernel, (first, last) of its sub-step loop, spilled VGPRs)} of the plain build"""
    listings = isa_stats.compile_units()
    assert len(listings) == 3
    out = {}
    for name, u in isa_lines.UNITS.items():
        sym = isa_stats.STEP_KERNELS[u][0]
        k = isa_stats.parse_kernel(listings[u], sym)
        assert k is not None, sym
        insts, labels = k[0], k[1]
        res = isa_stats.resources("\n".join(listings[u]), sym)
        assert res is not None, sym
        out[name] = (insts, isa_stats.substep_loop(insts, labels), int(res[5]))
    return out


def loop_of(units, name):
    insts, (lo, hi), _ = units[name]
    return insts[lo:hi + 1]


@pytest.mark.parametrize("name", ["one", "two"])
def test_substep_loop_is_shorter_than_the_parents(units, name):
    n = len(loop_of(units, name))
    print("%s-wave unit: sub-step loop %d instructions (parent %d)" % (name, n, PARENT_LOOP[name]))
    assert n > 2000, "not the sub-step loop"      # the loop search found something else
    assert n < PARENT_LOOP[name]


@pytest.mark.parametrize("name", ["one", "two", "anchor"])
def test_no_more_spills_or_scratch_in_the_loop_than_the_parent(units, name):
    spilled = units[name][2]
    scratch = isa_stats.scratch_accesses(loop_of(units, name))
    print("%s: %d spilled VGPRs, %d scratch accesses in the sub-step loop" % (name, spilled, scratch))
    assert spilled <= PARENT_SPILLED_VGPRS[name]
    assert scratch <= PARENT_LOOP_SCRATCH[name]


def test_no_unfused_row_shift_move_is_left_in_the_one_wave_loop(units):
    """The subtree sums are v_add_f32_dpp in place: a v_mov_b32_dpp ... row_shl in the loop is the unfused form (gone, not moved)."""
    loop = loop_of(units, "one")
    bad = [t for t in loop if t.startswith("v_mov_b32_dpp") and "row_shl" in t]
    assert not bad, bad[:4]
    fused = [t for t in loop if t.startswith("v_add_f32_dpp") and "row_shl" in t]
    assert len(fused) == 30, len(fused)           # 15 values (I[6], f[6], h[3]), two steps each


def test_by_line_attribution_covers_the_plain_builds_loop(units):
    """tools/isa_lines.py: the build with line tables has the plain build's instruction counts, and every instruction of the loop is
    attributed to exactly one source line."""
    d = isa_lines.by_line("one")
    insts, (lo, hi), _ = units["one"]
    assert d["plain"] == {"kernel": len(insts), "loop": hi - lo + 1}
    assert d["lines"] == d["plain"]
    assert sum(sum(c.values()) for c in d["classes"].values()) == hi - lo + 1
    known = sum(sum(c.values()) for (f, _), c in d["classes"].items() if f != "?")
    assert known > 0.95 * (hi - lo + 1)           # the line tables are there (not a build without -g)
    zero_moves = sum(r["length"] for r in d["zero_runs"])
    assert zero_moves <= sum(m["constant"] for m in d["movs"].values())
