#!/usr/bin/env python3
"""The denoisers (rt_denoise*, rt_denoise_dual*) against the interval enclosure of tests/denoise_exact.py and the closed forms
of tests/denoise_cases.py. One line per case and output: the largest relative interval width, the worst |got - mid| /
half-width (1 is the interval's edge) and the values outside, for the numpy restatements and, with --gpu, for the library's
host form on every case and its device form on the device cases; then the closed forms' residuals in ulps of the expected
value (0 where the comparison is for equality). profiles/denoise_exact.log is this tool's output, without and with --gpu.

--mutants seeds the eight mistakes of tests/test_denoise_ref.py's table into scratch copies of `restate` / `restate_dual`
(text replacements in the modules' source, executed in a namespace of their own; nothing is written) and prints which
enclosure cases and which closed forms name each, with the worst distance from the interval's middle in interval widths.

    python tools/denoise_report.py [--gpu] [--mutants] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import denoise_cases as DC      # noqa: E402

SWAPPED = ("ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)", "ok = (qx >= 0) & (qx < H) & (qy >= 0) & (qy < W)")
THIRD = ("dist(a, a[qy, qx])", "dist(a[..., [0, 1, 1]], a[qy, qx][..., [0, 1, 1]])")
CLAMPED = [("sw = np.where(ok, sw + w, sw)", "sw = sw + w"),
           ("sv = np.where(ok[..., None], sv + w[..., None] * e[qy, qx], sv)", "sv = sv + w[..., None] * e[qy, qx]")]
# mistake -> (replacements in denoise_ref.py or None, replacements in denoise_dual_ref.py or None)
MUTANTS = {
    "1 step k + 1, not 2^k": ([("s = 1 << k", "s = k + 1")], [("taps(1 << k)", "taps(k + 1)"), ("taps(1 << t)", "taps(t + 1)")]),
    "2 sigma_k not halved": ([("np.float64(2.0 ** -k)", "np.float64(1.0)")], None),
    "3 taps clamped, not skipped": (CLAMPED, CLAMPED + [("sx = np.where(ok, sx + w * u[qy, qx], sx)", "sx = sx + w * u[qy, qx]"),
                                                        ("su = np.where(ok, su + (w * w) * u[qy, qx], su)", "su = su + (w * w) * u[qy, qx]")]),
    "4 u = su / sw": (None, [("u = su / (sw * sw)", "u = su / sw")]),
    "5 2 u_p for u_p + u_q": (None, [("((u + u[qy, qx]) + var_floor)", "((u + u) + var_floor)")]),
    "6 third albedo from the wrong plane": ([THIRD], [THIRD]),
    "7 rows and columns exchanged": ([SWAPPED], [SWAPPED]),
    "8 remodulation without the floor": ([("out = (e * m) * sp\n", "out = (e * a) * sp\n")], [("out = (e * m) * sp2", "out = (e * a) * sp2")]),
}


def mutated(module, replacements):
    """The functions of tests/<module>.py with the replacements made in its source, in a namespace of their own."""
    path = os.path.join(ROOT, "tests", module + ".py")
    src = open(path).read()
    for old, new in replacements:
        assert src.count(old) >= 1, (module, old)
        src = src.replace(old, new)
    ns = {"__name__": module + "_mutant"}
    exec(compile(src, path, "exec"), ns)
    return ns


class Mutant(DC.Restated):
    def __init__(self, single, dual):
        self.restate = mutated("denoise_ref", single)["restate"] if single else None
        self.restate_dual = mutated("denoise_dual_ref", dual)["restate_dual"] if dual else None

    def single(self, sums, guides, prm, rows=None):
        import numpy as np
        return self.restate(sums, DC.pack(guides), DC.blocks(np.shape(sums), prm)[0], rows)

    def dual(self, sum_a, sum_b, ga, gb, prm, rows=None):
        import numpy as np
        return self.restate_dual(sum_a, sum_b, DC.pack(ga), DC.pack(gb), *DC.blocks(np.shape(sum_a), prm), rows)


def mutant_table(say):
    forms = DC.closed_forms()
    for name, (single, dual) in MUTANTS.items():
        filt = Mutant(single, dual)
        have = [w for w, r in (("single", single), ("dual", dual)) if r]
        named, worst = [], 0.0
        for case in DC.CASES:
            if DC.CASES[case][0] not in have:
                continue
            rows = DC.against_enclosure(case, filt)
            if any(r[3] for r in rows):
                named.append(case)
                worst = max(worst, max(r[2] for r in rows) / 2)
        failed = []
        for fname, which, check in forms:
            if which not in have:
                continue
            try:
                check(filt)
            except AssertionError:
                failed.append("%s (%s)" % (fname, which))
        say("%s\n    enclosure: %d of %d cases, worst %.3g interval widths from the middle: %s\n    closed forms: %s"
            % (name, len(named), sum(DC.CASES[c][0] in have for c in DC.CASES), worst, "; ".join(named) or "NONE", "; ".join(failed) or "NONE"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gpu", action="store_true", help="the library on the current HIP device instead of the restatements")
    ap.add_argument("--mutants", action="store_true", help="the table of seeded mistakes instead")
    ap.add_argument("--out", help="append the report to this file as well")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if a.mutants:
        mutant_table(say)
    else:
        if a.gpu:
            import torch
            torch.zeros(1, device="cuda")
            filters = [(DC.Library(), list(DC.CASES)), (DC.Device(), DC.GPU_CASES)]
        else:
            filters = [(DC.Restated(), list(DC.CASES))]
        outside = 0
        for filt, cases in filters:
            say("== %s against the enclosure (cap on the relative width %g)" % (filt.name, DC.WIDTH_CAP))
            say("%-30s %-9s %-12s %-12s %s" % ("case", "output", "rel. width", "off middle", "outside"))
            for case in cases:
                t = time.time()
                for what, width, off, bad in DC.against_enclosure(case, filt):
                    say("%-30s %-9s %-12.3g %-12.3g %d" % (case, what, width, off, bad))
                    outside += bad + (width > DC.WIDTH_CAP)
                print("    (%.1f s)" % (time.time() - t), flush=True)
            say("== %s, closed forms: worst residual in ulps of the expected value" % filt.name)
            DC.worst_ulps.clear()
            for fname, which, check in DC.closed_forms():
                r = check(filt)
                say("%-44s %-7s holds%s" % (fname, which, "" if r is None else "  (ratios %.4f, %.4f)" % tuple(r)))
            for key, ulps in sorted(DC.worst_ulps.items()):
                say("    %-40s %.3g ulp" % (key, ulps))
        say("values outside or intervals over the cap: %d" % outside)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
