#!/usr/bin/env python3
"""Choose the defaults of the temporal accumulation (rt_temporal*) on the CPU: no GPU is used.

    python3 tools/temporal_grid.py > profiles/temporal_grid.log

GPU renders and feature buffers are the oracle's bit for bit and the accumulation is its numpy restatement's
(tests/temporal_ref.py), so every number below is the number a GPU run gives. Three camera paths — cornell_box, random_scene
with its aperture, final_scene — of 8 cameras on a line at 48 x 48, 4 spp per frame with a seed per frame; the target is a
256 spp render at the last camera. The display-value MSE sqrt(clip(c, 0, 0.999)) of the accumulated last frame over the grid

    tol_depth in {0.02, 0.05, 0.1, 0.2}  x  tol_normal in {0.05, 0.1, 0.3}  x  n_max in {8, 32},   w_min 0.25,

as a ratio to the MSE of the last frame alone. The grid point with the smallest sum of the three ratios is the package's
TEMPORAL_DEFAULTS; the same numbers at that point for one path the grid never saw close the log, with the fraction of pixels
that restart per frame (with both tests off for comparison: what the geometry alone loses).

    python3 tools/temporal_grid.py --media > profiles/temporal_media_grid.log

prints another table instead, at TEMPORAL_DEFAULTS and with both tests off, for cornell_smoke, final_scene, cornell_box and
random_scene: the ratio and the restart share under (1) first-hit records, (2) RT_FLAG_SURFACES records — the oracle's
composition on a copy of the scene whose media never answer (tests/surface_ref.py) — and (3) surface records with
RT_TEMPORAL_FAR_MISSES (tests/temporal_far_ref.py's restatement).
"""
import itertools
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import raytracer_2022_amd as rt  # noqa: E402
from oracle import oracle_ffi as O  # noqa: E402
import temporal_ref as R  # noqa: E402
import surface_ref as S  # noqa: E402
import temporal_far_ref as FR  # noqa: E402

TOL_DEPTH, TOL_NORMAL, N_MAX, W_MIN = (0.02, 0.05, 0.1, 0.2), (0.05, 0.1, 0.3), (8.0, 32.0), 0.25
THREADS = min(8, os.cpu_count() or 1)


def path_inputs(name, step):
    s, bg, cams, sums, feats = R.oracle_path(rt, O, name, step, threads=THREADS)
    return cams, sums, feats, R.oracle_target(rt, O, s, bg, cams[-1], threads=THREADS)


def ratio(inp, **kw):
    cams, sums, feats, target = inp
    out, _, restarts = R.accumulate(sums, feats, cams, rt.temporal_params(R.PATH_W, R.PATH_H, R.PATH_SPP, w_min=W_MIN, **kw))
    last = R.mse(sums[-1], R.PATH_SPP, target)
    acc = R.mse(out, R.PATH_SPP, target)
    return last, acc, acc / last, restarts


def main():
    print("# tools/temporal_grid.py: CPU oracle renders (%d cameras, %dx%d, %d spp, seed %d + frame; target %d spp, seed %d), numpy restatement"
          % (R.PATH_K, R.PATH_W, R.PATH_H, R.PATH_SPP, R.SEED, R.REF_SPP, R.REF_SEED))
    paths = [(name, path_inputs(name, step)) for name, step in R.PATH_STEP.items()]
    for name, inp in paths:
        print("path %-13s step %-5g mse_last %.6e" % (name, R.PATH_STEP[name], R.mse(inp[1][-1], R.PATH_SPP, inp[3])), flush=True)
    print("# grid: mse_accumulated and mse_accumulated / mse_last per path, then the sum of the three ratios")
    best, ties = None, []
    for td, tn, nm in itertools.product(TOL_DEPTH, TOL_NORMAL, N_MAX):
        cells, total = [], 0.0
        for name, inp in paths:
            _, acc, r, _ = ratio(inp, tol_depth=td, tol_normal=tn, n_max=nm)
            total += r
            cells.append("%s %.6e %.4f" % (name, acc, r))
        print("tol_depth %-5g tol_normal %-5g n_max %-3g  %s  sum %.4f" % (td, tn, nm, "  ".join(cells), total), flush=True)
        if best is None or total < best[0]:
            best, ties = (total, td, tn, nm), []
        elif total == best[0]:
            ties.append((td, tn, nm))
    total, td, tn, nm = best
    print("# chosen (smallest sum, the first of equals): tol_depth %g tol_normal %g n_max %g w_min %g  sum %.4f" % (td, tn, nm, W_MIN, total))
    for tie in ties:                                       # (a path of K frames cannot tell caps >= K apart)
        print("#   equal: tol_depth %g tol_normal %g n_max %g" % tie)
    print("# at the chosen point: mse_last, mse_accumulated, ratio, restarted pixels per frame (frames 1 .. 7); then the restarts with both tests off")
    for name, inp in paths + [(R.HELD_OUT[0], path_inputs(*R.HELD_OUT))]:
        last, acc, r, restarts = ratio(inp, tol_depth=td, tol_normal=tn, n_max=nm)
        off = ratio(inp, tol_depth=math.inf, tol_normal=math.inf, n_max=nm)
        print("%s %-13s mse_last %.6e  mse_accumulated %.6e  ratio %.4f  restarts %s  |  tests off: ratio %.4f  restarts %s"
              % ("held-out" if name == R.HELD_OUT[0] else "grid    ", name, last, acc, r, " ".join("%.2f" % x for x in restarts),
                 off[2], " ".join("%.2f" % x for x in off[3])), flush=True)


def media_table():
    import numpy as np
    W, H, spp = R.PATH_W, R.PATH_H, R.PATH_SPP
    print("# tools/temporal_grid.py --media: CPU oracle renders (%d cameras, %dx%d, %d spp, seed %d + frame; target %d spp, seed %d), numpy restatement"
          % (R.PATH_K, W, H, spp, R.SEED, R.REF_SPP, R.REF_SEED))
    print("# per cell: mse_accumulated / mse_last, then the restarted share of frames 1 .. 7; columns: first-hit records | surface records"
          " (RT_FLAG_SURFACES) | surface records and RT_TEMPORAL_FAR_MISSES")
    steps = dict(R.PATH_STEP, **{R.HELD_OUT[0]: R.HELD_OUT[1]})
    rows = np.arange(H, dtype=np.uint32)
    for name in ("cornell_smoke", "final_scene", "cornell_box", "random_scene"):
        s, bg, cams, sums, feats = R.oracle_path(rt, O, name, steps[name], threads=THREADS)
        surf = [S.oracle_surface_features(O, s.desc, c, R.frame_params(rt, W, H, spp, bg, k), rows)[0].reshape(H, W) for k, c in enumerate(cams)]
        same = all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(feats, surf))
        depths = np.concatenate([f["depth"].ravel() for f in surf])
        target = R.oracle_target(rt, O, s, bg, cams[-1], threads=THREADS)
        last = R.mse(sums[-1], spp, target)
        print("path %-13s step %-5g media %d  mse_last %.6e  surface records %s, every depth finite: %s"
              % (name, steps[name], s.desc.n_media, last, "bit-equal to first-hit records" if same else "differ", bool(np.isfinite(depths).all())), flush=True)
        for label, kw in (("defaults ", {}), ("tests off", {"tol_depth": math.inf, "tol_normal": math.inf})):
            cells = []
            for records, far in ((feats, False), (surf, False), (surf, True)):
                out, _, restarts = FR.accumulate(sums, records, cams, rt.temporal_params(W, H, spp, far_misses=far, **kw))
                cells.append("%.4f  restarts %s" % (R.mse(out, spp, target) / last, " ".join("%.2f" % x for x in restarts)))
            print("  %s  %s" % (label, "  |  ".join(cells)), flush=True)


if __name__ == "__main__":
    media_table() if "--media" in sys.argv[1:] else main()
