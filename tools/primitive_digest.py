#!/usr/bin/env python3
"""Reduce the `PRIMITIVE <name> <build> max_err=... bound=... n=...` lines of a GPU test run (pytest -s) to one line per entry and
build: the line that comes closest to its bound (or misses it by most), of all the buckets and parameters in the name's brackets, with
the number of lines and values it stands for.  profiles/device_primitives.txt holds the solver probe's lines in this form.

usage: python -m pytest tests/test_gpu_solver_primitives.py -m gpu -s -q | python tools/primitive_digest.py"""
import re
import sys


def digest(lines):
    best, order = {}, []
    for l in lines:
        m = re.search(r"PRIMITIVE (.*) (\S+) max_err=(\S+) bound=(\S+) n=(\d+)\s*$", l)
        if not m:
            continue
        name, build, e, b, n = m.group(1), m.group(2), float(m.group(3)), float(m.group(4)), int(m.group(5))
        key = (re.sub(r"\[.*?\]", "", name), build)
        ratio = e / b if b > 0 else (0.0 if e == 0 else float("inf"))
        if key not in best:
            order.append(key)
            best[key] = [ratio, m.group(0).strip(), 0, 0]
        if ratio > best[key][0]:
            best[key][0], best[key][1] = ratio, m.group(0).strip()
        best[key][2] += 1
        best[key][3] += n
    return ["%s   (worst of %d lines, %d values)" % (best[k][1], best[k][2], best[k][3]) for k in order]


if __name__ == "__main__":
    print("\n".join(digest(sys.stdin)))
