#!/usr/bin/env python3
"""Generator draws per basic block of the kernels that inline the path RNG, read from the gfx950 ISA hipcc emits.

    python3 tools/isa_draws.py > profiles/<tag>_isa_draws.txt

Compiles pt_wavefront_shade.hip, pt_kernel.hip and pt_features.hip to assembly with the library's flags (device side only) and lists,
for every instance of wf_shade, pt_megakernel and pt_features, the basic blocks that hold draws of the counter-based
generator (rt_math.h: draw i = mix64(s + i * gamma)) with their instruction counts. A draw is recognised by the mixer's middle
step, the 64-bit `z ^ (z >> 27)` (one per mix64; the shift amount occurs nowhere else in these kernels); beside it the block's
v_mad_u64_u32 (two per mix64: its 64-bit multiplications; a gen_index adds those of its widening multiply) and, for a
gen_range, the `| 0x3ff00000` of the 52-bit mantissa trick. mix64 also hashes the path key (three per camera ray): those count
as draws here.

What to look for: a redraw loop (`for tries < RT_MAX_REJECT`) around a draw is turned into a block of FOUR draws side by side,
of which the accepted-first-try path needs one; with the first draw peeled out of the loop every block on that path holds one
draw per call site (a run of one-draw blocks: x, y, z of a sampler try follow each other), and the four-draw blocks that remain
are the redraw loops themselves, behind a branch that is (almost) never taken. Blocks are listed in layout order with the loop
depth LLVM notes beside their labels.

A static count, not a profile. ISA=<dir> reads <dir>/<source>.s made earlier with the same flags instead of compiling.
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(HERE, "raytracer_2022_amd", "csrc", "hip")
SOURCES = ["pt_wavefront_shade.hip", "pt_kernel.hip", "pt_features.hip"]
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-math-errno", "--offload-arch=gfx950", "-fno-slp-vectorize", "-mllvm", "-disable-machine-licm",
         "--cuda-device-only", "-S"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = "/opt/rocm/llvm/bin/llvm-cxxfilt"
WANTED = ("wf_shade", "pt_megakernel", "pt_features")

SHR27 = re.compile(r"^v_lshrrev_b64\s+v\[\d+:\d+\],\s*27,")
OR3FF = re.compile(r"^v_or_b32\S*\s+.*0x3ff00000")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BBCOMMENT = re.compile(r"^; %bb\.\d+:")


def compile_to_asm(src, out, extra=()):
    p = subprocess.run([HIPCC] + FLAGS + list(extra) + ["-o", out, src], capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        raise RuntimeError("hipcc failed on %s" % src)
    return open(out).read()


def kernels(asm):
    """{mangled name: [line, ...]} for every kernel of an assembly listing (from its label to s_endpgm's function end)."""
    lines = asm.split("\n")
    names = [m.group(1) for m in (re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    out = {}
    for name in names:
        start = next((i for i, l in enumerate(lines) if l.startswith(name + ":")), None)
        if start is None:
            continue
        end = next((i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end")), len(lines))
        out[name] = lines[start + 1:end]
    return out


def blocks(body):
    """[(label, note, [instruction, ...])] in layout order; `note` is the loop comment LLVM puts beside the label."""
    out = [("entry", "", [])]
    for l in body:
        m = LABEL.match(l)
        if m or BBCOMMENT.match(l):
            label = m.group(1) if m else l.split(":")[0].lstrip("; ")
            note = l.split(";", 1)[1].strip() if (m and ";" in l) else ""
            out.append((label, note, []))
            continue
        t = l.strip()
        if t.startswith(";") and not out[-1][2] and ("Loop" in t or "Header" in t):        # continuation of the label's loop comment
            out[-1] = (out[-1][0], (out[-1][1] + " " + t.lstrip("; ")).strip(), out[-1][2])
            continue
        if not t or t.startswith((";", ".", "//")):
            continue
        out[-1][2].append(t)
    return [b for b in out if b[2]]


def census(insns):
    """Counts of one instruction list: all, vector ALU, v_mad_u64_u32, mixer middle steps (= draws), mantissa ors."""
    ops = [i.split()[0] for i in insns]
    return {
        "all": len(ops),
        "valu": sum(1 for o in ops if o.startswith("v_")),
        "mad": sum(1 for o in ops if o.startswith("v_mad_u64_u32")),
        "draws": sum(1 for i in insns if SHR27.match(i)),
        "or3ff": sum(1 for i in insns if OR3FF.match(i)),
    }


def depth_of(note):
    m = re.search(r"Depth=(\d+)", note)
    return int(m.group(1)) if m else 0


def demangle(names):
    if not os.path.exists(CXXFILT):
        return {n: n for n in names}
    p = subprocess.run([CXXFILT] + list(names), capture_output=True, text=True)
    got = p.stdout.strip().split("\n")
    return dict(zip(names, got)) if p.returncode == 0 and len(got) == len(names) else {n: n for n in names}


def report(asm, source):
    ks = kernels(asm)
    names = [n for n in ks if any(w in n for w in WANTED)]
    pretty = demangle(names)
    for n in names:
        bl = blocks(ks[n])
        rows = [(lab, note, census(ins)) for lab, note, ins in bl]
        tot = census([i for _, _, ins in bl for i in ins])
        with_draws = [r for r in rows if r[2]["draws"]]
        hist = {}
        for r in with_draws:
            hist[r[2]["draws"]] = hist.get(r[2]["draws"], 0) + 1
        print("%s: %s" % (source, re.sub(r"\(.*$", "", pretty[n])))
        print("    %d instructions (%d vector), %d draws in %d blocks; blocks by draws held: %s"
              % (tot["all"], tot["valu"], tot["draws"], len(with_draws), ", ".join("%d x %d" % (hist[k], k) for k in sorted(hist)) or "-"))
        for lab, note, c in with_draws:
            print("    %-10s draws %d  instructions %3d  vector %3d  v_mad_u64_u32 %2d  |0x3ff00000 %d  loop depth %d"
                  % (lab, c["draws"], c["all"], c["valu"], c["mad"], c["or3ff"], depth_of(note)))


def main():
    print("# tools/isa_draws.py: basic blocks that hold generator draws (mix64), from hipcc's gfx950 assembly")
    print("# flags: %s" % " ".join(FLAGS[:-2]))
    with tempfile.TemporaryDirectory() as tmp:
        for src in SOURCES:
            if os.environ.get("ISA"):
                asm = open(os.path.join(os.environ["ISA"], src.replace(".hip", ".s"))).read()
            else:
                asm = compile_to_asm(os.path.join(HIP, src), os.path.join(tmp, src.replace(".hip", ".s")))
            report(asm, src)


if __name__ == "__main__":
    main()
