"""Compile-only (no GPU): the WHOLE sub-step loop of the step kernels, the code behind its back edge included.

tests/test_isa_budget.py measures the loop as the span of its backward branch.  Since the rare paths of a sub-step (joint-limit bank,
fall proxies: ORR_RARE in csrc/orr_physics.h) are placed behind that branch in the one-wave units, the span is the common path plus two
rare blocks, and about a third of the loop's code lies outside it.  tools/isa_stats.py's loop_side_blocks finds that code by control
flow (what the loop's first instruction reaches and is reached from); this test holds the whole loop to the figures of the tree before
the blocks moved (span + outside: 3156 + 68 one wave, 3235 + 0 two waves, 3290 + 68 friction anchors) and to no scratch access outside
the span.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lines  # noqa: E402
import isa_stats  # noqa: E402

WHOLE_LOOP_BEFORE = {"one": 3156 + 68, "two": 3235, "anchor": 3290 + 68}


@pytest.fixture(scope="module")
def loops():
    """{unit: (instructions, (first, last) of the span, indices outside the span)}"""
    listings = isa_stats.compile_units()
    out = {}
    for name, u in isa_lines.UNITS.items():
        insts, labels = isa_stats.parse_kernel(listings[u], isa_stats.STEP_KERNELS[u][0])[:2]
        lo, hi = isa_stats.substep_loop(insts, labels)
        out[name] = (insts, (lo, hi), isa_stats.loop_side_blocks(insts, labels, lo, hi))
    return out


@pytest.mark.parametrize("name", ["one", "two", "anchor"])
def test_whole_loop_is_shorter_than_before_the_rare_blocks_moved(loops, name):
    insts, (lo, hi), side = loops[name]
    n = hi - lo + 1 + len(side)
    print("%s: span %d + %d outside = %d (before: %d)" % (name, hi - lo + 1, len(side), n, WHOLE_LOOP_BEFORE[name]))
    assert not any(lo <= i <= hi for i in side)
    assert n < WHOLE_LOOP_BEFORE[name]


@pytest.mark.parametrize("name", ["one", "two", "anchor"])
def test_no_scratch_access_in_the_loops_code_outside_its_span(loops, name):
    insts, _, side = loops[name]
    assert isa_stats.scratch_accesses([insts[i] for i in side]) == 0


def test_the_sweeps_with_the_joint_limit_bank_are_found_outside_the_span(loops):
    """The closure is not empty by accident: the one-wave unit's bank-B sweeps (row_newbcast on both banks) sit behind the back edge."""
    insts, (lo, hi), side = loops["one"]
    dpp = lambda idx: sum(1 for i in idx if "dpp" in insts[i].split()[0])   # noqa: E731
    assert dpp(side) > 150 and dpp(range(lo, hi + 1)) > 300
