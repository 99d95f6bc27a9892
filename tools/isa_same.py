#!/usr/bin/env python3
"""Are the compiled kernels of two builds the same? Compares device assembly (hipcc --save-temps: *-gfx950.s) kernel by kernel.

    python3 tools/isa_same.py OLD.s [OLD2.s ...] -- NEW.s [NEW2.s ...] [--rename REGEX REPL]...

A kernel is its label through .Lfunc_end, which takes in its .amdhsa_* descriptor block. Comments go, .LBB<n>_ / .Ltmp<n> /
.Lfunc_end<n> lose their numbers, mangled names are demangled; every --rename is then applied to the OLD side's names (a kernel
whose template parameters were re-spelled). Kernels pair by name. One line per kernel, `same` or `DIFFERENT` with the first
differing lines; exit status 1 on any difference and on any kernel that only one side has. It diffs text and looks for nothing.
"""
import re
import subprocess
import sys


def kernels(paths, renames):
    text = "\n".join(open(p).read() for p in paths)
    names = sorted(set(re.findall(r"\b_Z\w+", text)))
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    for rx, repl in renames:
        plain = [re.sub(rx, repl, n) for n in plain]
    table = dict(zip(names, plain))
    out = {}
    for m in re.finditer(r"^\t\.type\t(\w+),@function\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        body = re.sub(r"\b_Z\w+", lambda t: "K" if t.group(0) == m.group(1) else table[t.group(0)], m.group(2))
        body = re.sub(r"\.(LBB|Ltmp|Lfunc_end)\d+", r".\1", re.sub(r";.*", "", body))
        out[table.get(m.group(1), m.group(1))] = [ln.strip() for ln in body.split("\n") if ln.strip()]
    return out


def main():
    args, renames = sys.argv[1:], []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append((args[i + 1], args[i + 2]))
        del args[i:i + 3]
    cut = args.index("--")
    old, new = kernels(args[:cut], renames), kernels(args[cut + 1:], [])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            verdict = "MISSING from the %s side" % ("old" if name not in old else "new")
        elif old[name] == new[name]:
            verdict = "same (%d lines)" % len(new[name])
        else:
            at = next((i for i, (a, b) in enumerate(zip(old[name], new[name])) if a != b), min(len(old[name]), len(new[name])))
            verdict = "DIFFERENT at line %d of %d / %d:\n    - %s\n    + %s" % (at, len(old[name]), len(new[name]), " | ".join(old[name][at:at + 3]), " | ".join(new[name][at:at + 3]))
        bad += not verdict.startswith("same")
        print("%s: %s" % (name, verdict))
    print("# %d kernels, %d same, %d different or missing" % (len(set(old) | set(new)), len(set(old) | set(new)) - bad, bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
