#!/usr/bin/env python3
"""Which values the sub-step loop of the step kernel reloads from AGPRs (development aid).

usage: python tools/isa_agprs.py [--unit one|two|anchor] [extra hipcc flags...]
The one-wave units fill the 256 architectural VGPRs and park further values in AGPRs; every use inside the loop costs a
v_accvgpr_read_b32, i.e. an issue slot.  Compiles the unit with -gline-tables-only (tools/isa_lines.py checks that this leaves the
instruction stream alone) and prints, for every such read inside the loop: the AGPR, the source line the read is attributed to, whether
the AGPR is written inside the loop (then it is no loop invariant), the source lines of the writes in front of the loop, and the first
instruction that uses the value.
"""
import argparse
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lines  # noqa: E402
import isa_stats  # noqa: E402


def audit(unit="one", extra_flags=()):
    """-> (loop length, rows): one row (agpr, offset in the loop, line of the read, offsets of the writes inside the loop, lines of the
    writes outside it, first use) per v_accvgpr_read_b32 of the loop, and the number of v_accvgpr_write_b32 inside it"""
    u = isa_lines.UNITS[unit]
    sym = isa_stats.STEP_KERNELS[u][0]
    dbg = isa_stats.compile_units(list(extra_flags) + ["-gline-tables-only"], only_main=u == 0)[u]
    insts, labels, locs, _ = isa_stats.parse_kernel(dbg, sym)
    lo, hi = isa_stats.substep_loop(insts, labels)
    files = isa_lines.file_table(dbg)
    where = lambda i: "%s:%d" % (files.get(locs[i][0], "?"), locs[i][1]) if locs[i] else "?"   # noqa: E731
    writes = collections.defaultdict(list)
    for i, t in enumerate(insts):
        m = re.match(r"v_accvgpr_write_b32 a(\d+),", t)
        if m:
            writes[int(m.group(1))].append(i)
    rows = []
    for i in range(lo, hi + 1):
        m = re.match(r"v_accvgpr_read_b32 (v\d+), a(\d+)", insts[i])
        if not m:
            continue
        a = int(m.group(2))
        use = next((insts[k] for k in range(i + 1, min(i + 60, hi + 1))
                    if " " in insts[k] and re.search(r"\b%s\b" % m.group(1), insts[k].split(None, 1)[1])), "?")
        rows.append((a, i - lo, where(i), [w - lo for w in writes[a] if lo <= w <= hi],
                     sorted({where(w) for w in writes[a] if not lo <= w <= hi}), use))
    return hi - lo + 1, sorted(rows), sum(1 for i in range(lo, hi + 1) if insts[i].startswith("v_accvgpr_write"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--unit", choices=sorted(isa_lines.UNITS), default="one")
    args, extra = ap.parse_known_args()
    n, rows, nw = audit(args.unit, extra)
    print("==== %s: v_accvgpr_read_b32 in the sub-step loop (%d instructions)" % (isa_stats.STEP_KERNELS[isa_lines.UNITS[args.unit]][1], n))
    print("%-5s %-7s %-26s %-22s %-44s %s" % ("agpr", "loop+", "read at", "written in the loop", "written in front of the loop at", "first use"))
    for a, off, at, w_in, w_out, use in rows:
        print("a%-4d %-7d %-26s %-22s %-44s %s" % (a, off, at, ",".join("+%d" % w for w in w_in) or "no (invariant)", " ".join(w_out), use))
    print("%d reads of %d AGPRs, %d of them of loop invariants; %d v_accvgpr_write_b32 in the loop" % (
        len(rows), len({r[0] for r in rows}), sum(1 for r in rows if not r[3]), nw))


if __name__ == "__main__":
    main()
