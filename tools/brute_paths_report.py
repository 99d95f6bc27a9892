#!/usr/bin/env python3
"""One block per case of tests/path_cases.py against the per-sample path reference of tests/brute_paths.py: samples, compared
samples, the samples in each class, the compared samples in each arm the case is named for, and the worst error / tolerance per
quantity — the value (a ray's or a pixel's sum) for the oracle (rto_radiance, rt_render_cpu) and, with --gpu, for the device
(rt_radiance, rt_render); the direction for the oracle where it exposes the step (rto_scatter on specular cases,
rto_lights_random on the light halves); the weight's denominator through rto_lights_pdf_value. The device's direction and
weight are seen through the value alone: a texel of the probe cube times the weight. profiles/brute_paths.log is this
tool's output with --gpu.

    python tools/brute_paths_report.py [--gpu] [--out FILE] [case ...]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import brute_paths as BP        # noqa: E402
import path_cases as PC         # noqa: E402

SPECULAR = ("metal", "glass")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gpu", action="store_true", help="also run rt_radiance / rt_render on the current HIP device")
    ap.add_argument("--out", help="write the report to this file as well")
    ap.add_argument("cases", nargs="*", default=PC.NAMES + PC.CAMERA_NAMES)
    a = ap.parse_args()
    import raytracer_2022_amd as rt
    from oracle import oracle_ffi as O
    if a.gpu:
        import torch
        torch.zeros(1, device="cuda")
    lines, worst_all, failures = [], 0.0, 0

    def say(s):
        print(s, flush=True)
        lines.append(s)
    rows = np.arange(PC.H, dtype=np.uint32)
    for name in a.cases:
        camera = name in PC.CAMERA_CASES
        c = PC.camera_reference(name) if camera else PC.reference(name)
        P = c.paths
        compared = P.compared()
        counts = (PC.check_camera_floors if camera else PC.check_floors)(c)
        say("%-20s depth %d samples %5d compared %5d | %s | %s" % (
            name, c.depth, len(compared), compared.sum(), " ".join("%s %d" % kv for kv in counts.items() if kv[1]) or "no class taken",
            " ".join("%s %d" % (arm, (P.arms[arm] & compared).sum()) for arm in c.arms)))
        results = []
        if camera:
            got, st = O.render_cpu(c.desc, c.cam, c.params, rows, want_stats=True)
            results.append(("oracle", got, st.rng_draws))
            if a.gpu:
                got, st = rt.DeviceScene(c.desc).render(c.cam, c.params, rows, want_stats=True)
                results.append(("hip", got, st.rng_draws))
        else:
            got, st = O.radiance(c.desc, c.rays, spp=PC.SPP, background=PC.BACKGROUND, t_min=0.001, depth=c.depth, want_stats=True)
            results.append(("oracle", got, st.rng_draws))
            if a.gpu:
                got, st = rt.DeviceScene(c.desc).radiance(c.rays, spp=PC.SPP, background=PC.BACKGROUND, t_min=0.001, max_depth=c.depth, want_stats=True)
                results.append(("hip", got, st.rng_draws))
        for who, got, draws in results:
            try:
                say("    " + PC.hold(c, got, who, draws, quiet=True))
            except AssertionError as e:
                failures += 1
                say("    %s %s FAILED: %s" % (name, who, str(e)[:300]))
            worst_all = max(worst_all, BP.compare(np.asarray(got).reshape(-1, 3), c.value, c.tol, c.keep)[0])
        if not camera and name.startswith(SPECULAR):
            say("    %-20s oracle direction (rto_scatter, 300 samples) worst error / tolerance %.3e" % (name, PC.scatter_step(O, c)))
        if not camera and any(arm.startswith("light-") for arm in c.arms):
            wd, wp = PC.lights_step(O, c)
            say("    %-20s oracle direction (rto_lights_random, 400 samples) worst error / tolerance %.3e; pdf (rto_lights_pdf_value) %.3e" % (name, wd, wp))
    say("worst value error / tolerance overall %.3e; failures %d" % (worst_all, failures))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
