#!/usr/bin/env python3
"""True error of rt_math.h, family by family: one line per function and family of tests/math_cases.py with the count, the
worst error in ulps of the exact value (tests/math_ref.py: mpmath at 400 bits) and the argument that gives it, in hex.

    python3 tools/math_report.py                        # the header as the oracle (g++) compiles it
    python3 tools/math_report.py --gpu                  # the same header on the device (rt_debug_math_device)
    python3 tools/math_report.py --oracle-lib PATH      # another build of the oracle, e.g. the parent commit's

sqrt and '/' are counted in doubles that differ from numpy's IEEE results. profiles/math_edges.log holds the three runs."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import math_cases as MC   # noqa: E402
import math_ref as MR     # noqa: E402


def device_math(op, a, b):
    from raytracer_2022_amd import _ffi as F
    out = np.empty_like(a)
    dp = C.POINTER(C.c_double)
    F.check(F.lib().rt_debug_math_device(op, a.ctypes.data_as(dp), None if b is None else b.ctypes.data_as(dp), out.ctypes.data_as(dp), a.size))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gpu", action="store_true", help="run the functions on the device instead of the host")
    ap.add_argument("--oracle-lib", help="path of the oracle library to measure (default: oracle/librt_oracle.so)")
    args = ap.parse_args()
    if args.gpu:
        run, what = device_math, "device (rt_debug_math_device)"
    else:
        from oracle import oracle_ffi as O
        if args.oracle_lib:
            O.LIB_PATH = os.path.abspath(args.oracle_lib)
        O.lib()
        run, what = O.math_array, "host (%s)" % os.path.relpath(O.LIB_PATH, ROOT)
    print("# rt_math.h on the %s against mpmath at %d bits; error in ulps of the exact value" % (what, MR.PREC))
    print("%-5s %-62s %6s %12s  %s" % ("op", "family", "count", "worst", "at"))
    for op in (MR.SIN, MR.COS, MR.ACOS, MR.ATAN2, MR.LOG):
        a, b, _ = MC.concatenated(op)
        for name, n, w, arg in MR.family_errors(op, run(op, a, b)):
            print("%-5s %-62s %6d %12.4g  %s%s" % (MR.NAMES[op], name, n, w, arg, "" if w < MR.BOUNDS[op] else "   <-- not under %g" % MR.BOUNDS[op]))
    x = MC.sincos_at_or_above_2p52()
    s, c = run(MR.SIN, x, None), run(MR.COS, x, None)
    print("%-5s %-62s %6d %12s  sin = +0: %s, cos = 1: %s" % ("", "finite |x| >= 2^52 (defined, not measured)", len(x), "-",
                                                              bool(np.all(s == 0) and not np.signbit(s).any()), bool(np.all(c == 1))))
    for op in (MR.SQRT, MR.DIV):
        for name, (a, b) in MC.families(op).items():
            with np.errstate(all="ignore"):
                want = np.sqrt(a) if op == MR.SQRT else a / b
            got = run(op, a, b)
            differ = int((np.isnan(got) != np.isnan(want)).sum() + (MC.to_bits(got) != MC.to_bits(want))[~np.isnan(want) & ~np.isnan(got)].sum())
            print("%-5s %-62s %6d %12s  doubles that differ from IEEE (numpy): %d" % (MR.NAMES[op], name, len(a), "-", differ))


if __name__ == "__main__":
    main()
