#!/usr/bin/env python3
"""Static instruction statistics of orr_step_kernel<0> from the compiler's assembly (development aid).

usage: python tools/isa_stats.py [extra hipcc flags...]
Compiles the env kernels' units (csrc/orr_kernels*.hip) to gfx950 assembly with the product's flags, finds the step kernels, and prints instruction
counts by class for the whole kernel and for its hottest region (the sub-step loop = the largest backward-branch body)."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openroborl_amd import _lib  # noqa: E402


def classify(m):
    if m.startswith("v_pk_"):
        return "valu_pk"
    if m.startswith("v_mfma"):
        return "mfma"
    if m.startswith("v_accvgpr"):
        return "agpr_move"
    if m.endswith("_dpp") or "dpp" in m:
        return "valu_dpp"
    if m.startswith("v_mov") or m.startswith("v_cndmask") or m.startswith("v_readlane") or m.startswith("v_writelane") or m.startswith("v_readfirstlane"):
        return "valu_move/select"
    if m.startswith("v_"):
        return "valu_math"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith("global_") or m.startswith("buffer_") or m.startswith("flat_") or m.startswith("scratch_"):
        return "vmem"
    if m.startswith("s_waitcnt"):
        return "s_waitcnt"
    if m.startswith("s_nop"):
        return "s_nop"
    if m.startswith("s_cbranch") or m.startswith("s_branch"):
        return "branch"
    if m.startswith("s_load") or m.startswith("s_buffer_load"):
        return "smem"
    if m.startswith("s_"):
        return "salu"
    return "other"


STEP_KERNELS = (("_Z15orr_step_kernelILi0ELi1ELb0E", "step kernel, one wave per SIMD"), ("_Z15orr_step_kernelILi0ELi2ELb0E", "step kernel, two waves per SIMD"),
                ("_Z15orr_step_kernelILi0ELi1ELb1E", "step kernel with friction anchors (one wave per SIMD)"),
                ("_Z15orr_step_kernelILi0ELi1ELb0ELb1ELb0E", "step kernel with clip sets (one wave per SIMD)"),
                ("_Z15orr_step_kernelILi0ELi1ELb0ELb1ELb1E", "step kernel with clip sets and task noise (one wave per SIMD)"))
# the reward-terms unit's (orr_kernels_terms.hip; MODE = kModeTerms | 0): a table of its own, STEP_KERNELS[-1] stays the noise kernel
TERMS_STEP_KERNELS = (("_Z15orr_step_kernelILi4ELi1ELb0ELb1ELb1E", "step kernel with clip sets, task noise and reward terms (one wave per SIMD)"),)
# the contact-output unit's (orr_kernels_contacts.hip; MODE = kModeContacts | 0 and kModeContacts | kModeTerms | 0), likewise
CONTACT_STEP_KERNELS = (("_Z15orr_step_kernelILi8ELi1ELb0ELb1ELb1E", "step kernel with clip sets, task noise and contact outputs (one wave per SIMD)"),
                        ("_Z15orr_step_kernelILi12ELi1ELb0ELb1ELb1E", "step kernel with clip sets, task noise, reward terms and contact outputs (one wave per SIMD)"))
# the actuator unit's (orr_kernels_actuator.hip; MODE = kModeActuator | kModeContacts | kModeTerms | 0), likewise
ACTUATOR_STEP_KERNELS = (("_Z15orr_step_kernelILi28ELi1ELb0ELb1ELb1E", "step kernel with clip sets, task noise, reward terms, contact outputs, torque limits and actuator outputs (one wave per SIMD)"),)
# the sensor unit's (orr_kernels_sensor.hip; MODE = kModeSensor | kModeActuator | kModeContacts | kModeTerms | 0), likewise
SENSOR_STEP_KERNELS = (("_Z15orr_step_kernelILi60ELi1ELb0ELb1ELb1E", "step kernel with sensor noise on top of the actuator variant (one wave per SIMD)"),)
# the randomiser unit's (orr_kernels_randomizer.hip; MODE = kModeRandomizer | kModeSensor | kModeActuator | kModeContacts | kModeTerms | 0), likewise
RANDOMIZER_STEP_KERNELS = (("_Z15orr_step_kernelILi124ELi1ELb0ELb1ELb1E", "step kernel with the table-driven randomiser on top of the sensor variant (one wave per SIMD)"),)
# the push unit's (orr_kernels_push.hip; MODE = kModePush | kModeRandomizer | kModeSensor | kModeActuator | kModeContacts | kModeTerms | 0), likewise
PUSH_STEP_KERNELS = (("_Z15orr_step_kernelILi252ELi1ELb0ELb1ELb1E", "step kernel with external pushes on top of the randomiser variant (one wave per SIMD)"),)


def compile_units(extra_flags=(), only_main=False, units=("env", "w2", "anchor")):
    """Device assembly of the env kernels' translation units, each with the product's flags for it (+ extra_flags): one list of lines
    per unit.  `units` = names of _lib.ALL_ENV_UNITS, compiled in the table's order; the default is the three that tools/isa_lines.py and
    tests/test_isa_budget.py address by index (0 main, 1 two-wave, 2 friction anchors), "multiclip" adds the clip-set unit, "noise" the
    task-noise unit, "terms" (_lib.TERMS_UNITS, behind them) the reward-terms unit, "contacts" (_lib.CONTACT_UNITS) the
    contact-output unit, "actuator" (_lib.ACTUATOR_UNITS) the actuator unit, "sensor" (_lib.SENSOR_UNITS) the sensor-noise unit, "randomizer"
    (_lib.RANDOMIZER_UNITS) the randomiser unit, "push" (_lib.PUSH_UNITS, last) the push unit."""
    src_dir = os.path.dirname(os.environ.get("ORR_ISA_SRC", _lib.SRC))      # another tree's orr_kernels.hip (A/B of code generation)
    out_dir = tempfile.mkdtemp()
    listings = []
    for name, src, flags, _ in (_lib.ALL_ENV_UNITS + _lib.TERMS_UNITS + _lib.CONTACT_UNITS + _lib.ACTUATOR_UNITS + _lib.SENSOR_UNITS + _lib.RANDOMIZER_UNITS + _lib.PUSH_UNITS)[:1 if only_main else None]:
        src = os.path.join(src_dir, os.path.basename(src))
        if name not in units or not os.path.exists(src):      # (an older tree has fewer units)
            continue
        out = os.path.join(out_dir, name + ".s")
        flags = [f for f in flags if f not in ("-shared", "-fPIC")] + list(extra_flags)
        subprocess.check_call([_lib.HIPCC] + flags + ["-S", "--cuda-device-only", "-o", out, src], stderr=subprocess.DEVNULL)
        listings.append(open(out).read().split("\n"))
    return listings


def parse_kernel(lines, sym):
    """Instructions of the kernel `sym` in an assembly listing, or None: (insts, labels, locs, under) with labels = {label: index of the
    instruction behind it}, locs[i] = (file number, line) of the last .loc directive in front of instruction i (None without debug
    lines) and under[i] = the last label in front of it."""
    try:
        start = next(i for i, l in enumerate(lines) if re.match(r"^%s.*:" % sym, l))
    except StopIteration:
        return None
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    labels = {}
    insts, locs, under = [], [], []
    loc = lab = None
    for l in lines[start:end + 1]:
        t = l.split(";")[0].strip()
        if not t:
            continue
        m = re.match(r"^(\.?[A-Za-z_0-9$]+):$", t)
        if m:
            labels[m.group(1)] = len(insts)
            lab = m.group(1)
            continue
        if t.startswith("."):
            m = re.match(r"^\.loc\s+(\d+)\s+(\d+)", t)
            if m:
                loc = (int(m.group(1)), int(m.group(2)))
            continue
        insts.append(t)
        locs.append(loc)
        under.append(lab)
    return insts, labels, locs, under


def substep_loop(insts, labels):
    """(first, last) instruction of the sub-step loop = the backward branch whose body holds the most DPP instructions (the Gauss-Seidel
    sweeps live there); the largest backward branch alone can be some other loop of the step-end / reset code"""
    best = (0, 0, 0)
    dpp_prefix = [0]
    for t in insts:
        dpp_prefix.append(dpp_prefix[-1] + ("dpp" in t.split()[0]))
    best_key = (-1, -1)
    for i, t in enumerate(insts):
        m = re.match(r"^s_c?branch\S*\s+(\S+)$", t)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            lo = labels[m.group(1)]
            key = (dpp_prefix[i + 1] - dpp_prefix[lo], i - lo)
            if key > best_key:
                best_key, best = key, (i - lo, lo, i)
    return best[1], best[2]


def loop_side_blocks(insts, labels, lo, hi):
    """The instructions of the loop [lo, hi] that lie OUTSIDE its span: code that the block placement put behind the back edge (rare
    paths: orr_physics.h, ORR_RARE).  The loop is the set of instructions that can be reached from its first instruction and from
    which that one can be reached again (control flow at instruction granularity: a conditional branch has two successors, s_branch
    one, s_endpgm none); what the step kernel runs past the loop never comes back.  -> sorted indices outside lo .. hi"""
    n = len(insts)
    succ = [[] for _ in range(n)]
    for i, t in enumerate(insts):
        m = re.match(r"^s_(c?)branch\S*\s+(\S+)$", t)
        if m and m.group(2) in labels:
            succ[i].append(labels[m.group(2)])
        if not (m and not m.group(1)) and not t.startswith("s_endpgm") and i + 1 < n:
            succ[i].append(i + 1)
    pred = [[] for _ in range(n)]
    for i, ss in enumerate(succ):
        for j in ss:
            if j < n:
                pred[j].append(i)

    def reach(edges):
        seen, todo = {lo}, [lo]
        while todo:
            for j in edges[todo.pop()]:
                if j < n and j not in seen:
                    seen.add(j)
                    todo.append(j)
        return seen
    return sorted(i for i in reach(succ) & reach(pred) if not lo <= i <= hi)


def scratch_accesses(seg):
    return sum(1 for t in seg if t.startswith("scratch_") or t.startswith("buffer_") and "offen" in t)


def resources(meta, sym):
    """(LDS bytes, scratch bytes per lane, sgprs, spilled sgprs, vgprs, spilled vgprs) from the kernel's metadata, as strings, or None"""
    m = re.search(r"\.group_segment_fixed_size:\s+(\d+)(?:(?!\.group_segment_fixed_size).)*?\.name:\s+%s.*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)" % sym, meta, re.S)
    return m.groups() if m else None


def main():
    lines = [l for u in compile_units(sys.argv[1:], units=[u[0] for u in _lib.ALL_ENV_UNITS + _lib.TERMS_UNITS + _lib.CONTACT_UNITS + _lib.ACTUATOR_UNITS + _lib.SENSOR_UNITS + _lib.RANDOMIZER_UNITS + _lib.PUSH_UNITS]) for l in u]
    meta = "\n".join(lines)
    # one report per variant of the step kernel (WPE 1: one wave per SIMD, WPE 2: two; see orr_env_kernels.h)
    for sym, title in STEP_KERNELS + TERMS_STEP_KERNELS + CONTACT_STEP_KERNELS + ACTUATOR_STEP_KERNELS + SENSOR_STEP_KERNELS + RANDOMIZER_STEP_KERNELS + PUSH_STEP_KERNELS:
        k = parse_kernel(lines, sym)
        if k is None:
            continue
        insts, labels = k[0], k[1]
        lo, hi = substep_loop(insts, labels)
        print("==== %s" % title)
        for name, seg in (("whole kernel", insts), ("largest loop (sub-steps)", insts[lo:hi + 1])):
            c = collections.Counter(classify(t.split()[0]) for t in seg)
            tot = sum(c.values())
            print("%s: %d instructions (scratch accesses: %d)" % (name, tot, scratch_accesses(seg)))
            for k, v in c.most_common():
                print("   %-18s %6d  %5.1f%%" % (k, v, 100.0 * v / tot))
        side = loop_side_blocks(insts, labels, lo, hi)
        if side:
            seg = [insts[i] for i in side]
            print("code of the loop outside that span (behind its back edge): %d instructions (scratch accesses: %d); loop with it: %d" % (
                len(seg), scratch_accesses(seg), hi - lo + 1 + len(seg)))
        r = resources(meta, sym)
        if r:
            print(" LDS %s B, scratch %s B per lane, sgpr %s (spilled %s), vgpr %s (spilled %s)" % r)


if __name__ == "__main__":
    main()
