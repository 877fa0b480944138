#!/usr/bin/env python3
"""Where the instructions of the step kernel's sub-step loop come from: instruction classes per source line (development aid).

usage: python tools/isa_lines.py [--unit one|two|anchor] [--top N] [--min-run N] [extra hipcc flags...]
Compiles the env kernels twice with the product's flags, plain and with -gline-tables-only (line tables only: no variable
locations, so the instruction stream stays what it is), CHECKS that the step kernel and its sub-step loop hold the same number of
instructions either way, and attributes every instruction of the loop to the source line of its innermost inlined frame.  Prints
  - the lines of the loop by instruction count, split into tools/isa_stats.py's classes,
  - the register moves (v_mov_b32 without DPP) split into constant and register sources, per line,
  - the runs of `v_mov vN, 0` with the label they sit under and the branch that leads there: a run behind a label that only a skip
    path reaches (the zero fill of a leg without contact, of a bank that is off) is not waste, a run on the common path is.
"""
import argparse
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_stats  # noqa: E402

UNITS = {"one": 0, "two": 1, "anchor": 2}     # index into isa_stats.compile_units() and isa_stats.STEP_KERNELS


def file_table(lines):
    """{file number: base name} from the .file directives of one unit's listing"""
    out = {}
    for l in lines:
        m = re.match(r'^\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            out[int(m.group(1))] = os.path.basename(m.group(3) or m.group(2))
    return out


def is_plain_mov(t):
    return t.split()[0] in ("v_mov_b32_e32", "v_mov_b32", "v_mov_b32_e64")


def mov_source_is_constant(t):
    src = t.split(",", 1)[1].strip()
    return not re.match(r"^[vsa]\d+$|^[vsa]\[|^vcc|^exec|^m0|^ttmp", src)


def is_zero_mov(t):
    return is_plain_mov(t) and t.split(",", 1)[1].strip() in ("0", "0x0")


def by_line(unit="one", extra_flags=()):
    """The attribution as data: dict with kernel / loop totals of the plain and the line-table build and, for the loop, the classes per
    (file, line), the moves by source kind per (file, line) and the runs of zero moves."""
    u = UNITS[unit]
    sym, title = isa_stats.STEP_KERNELS[u]
    only_main = u == 0
    plain = isa_stats.compile_units(extra_flags, only_main=only_main)[u]
    dbg = isa_stats.compile_units(list(extra_flags) + ["-gline-tables-only"], only_main=only_main)[u]
    p_insts, p_labels, _, _ = isa_stats.parse_kernel(plain, sym)
    p_lo, p_hi = isa_stats.substep_loop(p_insts, p_labels)
    insts, labels, locs, under = isa_stats.parse_kernel(dbg, sym)
    lo, hi = isa_stats.substep_loop(insts, labels)
    files = file_table(dbg)
    where = lambda i: (files.get(locs[i][0], "?"), locs[i][1]) if locs[i] else ("?", 0)   # noqa: E731
    classes = collections.defaultdict(collections.Counter)
    movs = collections.defaultdict(collections.Counter)
    for i in range(lo, hi + 1):
        classes[where(i)][isa_stats.classify(insts[i].split()[0])] += 1
        if is_plain_mov(insts[i]):
            movs[where(i)]["constant" if mov_source_is_constant(insts[i]) else "register"] += 1
    # who branches to a label (forward branches inside the loop): tells a skip target from a fall-through block
    branched_to = collections.Counter()
    for i in range(lo, hi + 1):
        m = re.match(r"^s_c?branch\S*\s+(\S+)$", insts[i])
        if m:
            branched_to[m.group(1)] += 1
    runs = []
    i = lo
    while i <= hi:
        if is_zero_mov(insts[i]):
            j = i
            while j + 1 <= hi and is_zero_mov(insts[j + 1]) and under[j + 1] == under[i]:
                j += 1
            at_label = under[i] is not None and labels.get(under[i]) == i      # the run opens its block
            runs.append({"length": j - i + 1, "label": under[i], "opens_block": at_label, "branches_to_label": branched_to.get(under[i], 0),
                         "offset": i - lo, "lines": sorted({where(k) for k in range(i, j + 1)})})
            i = j + 1
        else:
            i += 1
    return {"title": title, "plain": {"kernel": len(p_insts), "loop": p_hi - p_lo + 1},
            "lines": {"kernel": len(insts), "loop": hi - lo + 1}, "classes": classes, "movs": movs, "zero_runs": runs}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--unit", choices=sorted(UNITS), default="one")
    ap.add_argument("--top", type=int, default=40, help="source lines to print (by instruction count)")
    ap.add_argument("--min-run", type=int, default=2, help="shortest run of `v_mov vN, 0` to list")
    args, extra = ap.parse_known_args()
    d = by_line(args.unit, extra)
    print("==== %s: sub-step loop by source line" % d["title"])
    print("plain build: kernel %d / loop %d instructions; with -gline-tables-only: %d / %d" %
          (d["plain"]["kernel"], d["plain"]["loop"], d["lines"]["kernel"], d["lines"]["loop"]))
    if d["plain"] != d["lines"]:
        sys.exit("the line tables changed the instruction stream: the attribution below would not be the product's")
    tot = collections.Counter()
    for c in d["classes"].values():
        tot.update(c)
    cols = [k for k, _ in tot.most_common()]
    print("total %d: %s" % (sum(tot.values()), "  ".join("%s %d" % (k, tot[k]) for k in cols)))
    print("%-26s %6s  %s" % ("file:line", "count", "classes"))
    ranked = sorted(d["classes"].items(), key=lambda kv: -sum(kv[1].values()))
    for (f, ln), c in ranked[:args.top]:
        print("%-26s %6d  %s" % ("%s:%d" % (f, ln), sum(c.values()), "  ".join("%s %d" % (k, c[k]) for k in cols if c[k])))
    if len(ranked) > args.top:
        print("... %d more lines, %d instructions" % (len(ranked) - args.top, sum(sum(c.values()) for _, c in ranked[args.top:])))
    nc = sum(m["constant"] for m in d["movs"].values())
    nr = sum(m["register"] for m in d["movs"].values())
    print("-- register moves (v_mov_b32 without DPP): %d from a constant, %d from a register" % (nc, nr))
    for (f, ln), m in sorted(d["movs"].items(), key=lambda kv: -sum(kv[1].values()))[:args.top]:
        print("%-26s constant %3d  register %3d" % ("%s:%d" % (f, ln), m["constant"], m["register"]))
    runs = [r for r in d["zero_runs"] if r["length"] >= args.min_run]
    print("-- runs of `v_mov vN, 0` (%d of length >= %d, %d moves in them); 'opens its block' + branches to the label = a fill on the path that "
          "a branch reaches" % (len(runs), args.min_run, sum(r["length"] for r in runs)))
    for r in runs:
        print("  %3d x at loop+%-5d under %-12s %-16s branches to the label: %d   %s" % (
            r["length"], r["offset"], r["label"], "opens its block" if r["opens_block"] else "inside the block", r["branches_to_label"],
            " ".join("%s:%d" % w for w in r["lines"][:4])))


if __name__ == "__main__":
    main()
