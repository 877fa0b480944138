"""Are the kernels of a translation unit the same instructions in two trees?  Needs the compiler only, no GPU:
python tools/diag/kernel_asm_diff.py OTHER_TREE [unit ...]        (units: names of _lib's build rows, default: policy learner)

Each unit's source is compiled to gfx950 assembly (device only, the unit's own flags) in OTHER_TREE (e.g. `git worktree add` of the parent
commit) and in this tree; the text of every kernel, from its label to its end label, is compared line by line.  Prints one line per kernel:
its number of lines and `identical`, `DIFFERENT` (with the first differing line) or `only here` / `only there`."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
from openroborl_amd import _lib  # noqa: E402


def kernels(asm):
    """{demangled-ish name: [lines]} of every .amdhsa_kernel of an assembly text"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M)
    lines = asm.splitlines()
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].lstrip().startswith((".section", ".Lfunc_end")))
        body = [l.split(";")[0].rstrip() for l in lines[start + 1:end]]
        body = [l for l in body if l and (not l.lstrip().startswith((".L", ".p2align")) or l.lstrip().startswith(".LBB"))]
        out[name] = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in body]      # a label carries the function's number within the unit
    return out


def demangle(name):
    import shutil
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return name
    text = subprocess.run([tool, name], stdout=subprocess.PIPE, check=True).stdout.decode().strip()
    return re.sub(r"\(anonymous namespace\)::|\(.*\)$|^void ", "", text)     # the kernel and its template arguments


def assembly(tree, unit):
    name, src, flags, _ = unit
    src = os.path.join(tree, os.path.relpath(src, HERE))
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, name + ".s")
        subprocess.check_call([_lib.HIPCC] + [f for f in flags if f != "-shared"] + ["--cuda-device-only", "-S", "-o", out, src], stderr=subprocess.DEVNULL)
        return open(out).read()


def main():
    other = os.path.abspath(sys.argv[1])
    wanted = sys.argv[2:] or ["policy", "learner"]
    rows = [u for u in _lib.ALL_UNITS if u[0] in wanted]
    moved = 0
    for unit in rows:
        a, b = kernels(assembly(other, unit)), kernels(assembly(HERE, unit))
        print("unit %s (%s):" % (unit[0], os.path.relpath(unit[1], HERE)))
        for name in sorted(set(a) | set(b)):
            if name not in a or name not in b:
                print("  %-110s %5d lines   %s" % (demangle(name), len(a.get(name) or b.get(name)), "only here" if name in b else "only there"))
                continue
            if a[name] == b[name]:
                print("  %-110s %5d lines   identical" % (demangle(name), len(a[name])))
            else:
                moved += 1
                first = next((i for i, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
                print("  %-110s %5d / %d lines   DIFFERENT from line %d" % (demangle(name), len(a[name]), len(b[name]), first))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
