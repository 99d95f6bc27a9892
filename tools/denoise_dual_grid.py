#!/usr/bin/env python3
"""Choose the defaults of the variance-guided denoiser (rt_denoise_dual*) on the CPU: no GPU is used.

    python3 tools/denoise_dual_grid.py > profiles/denoise_dual_grid.log

GPU renders are the oracle's bit for bit and the filter is its numpy restatement's (tests/denoise_dual_ref.py), so every
number below is the number a GPU run gives. For the three views of the end-to-end tests — two frames of 2 spp at seed 2022
from the oracle, the features by the oracle composition of tests/features_ref.py, the target a 512 spp render at seed 7 —
the display-value MSE sqrt(clip(c, 0, 0.999)) of the dual filter over the grid

    sigma_color in {0.5, 1, 2, 4}  x  var_iter in {1, 2, 3}  x  var_floor in {1e-6, 1e-4, 1e-2},

the other parameters at rt_denoise's defaults; beside it mse_noisy (A + B at 4 spp) and mse_single (rt_denoise's restatement
at its defaults on A + B with features FA + FB and spp 4). The grid point with the smallest sum of the three ratios
mse_dual / mse_noisy is the package's DUAL_DEFAULTS; the same three numbers at that point for one view the grid never saw
close the log.
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import raytracer_2022_amd as rt  # noqa: E402
from oracle import oracle_ffi as O  # noqa: E402
import denoise_dual_ref as R  # noqa: E402
from denoise_ref import restate as restate_single  # noqa: E402
from features_ref import oracle_features  # noqa: E402

SIGMA_COLOR, VAR_ITER, VAR_FLOOR = (0.5, 1.0, 2.0, 4.0), (1, 2, 3), (1e-6, 1e-4, 1e-2)
THREADS = min(8, os.cpu_count() or 1)


def view_inputs(name, W, H):
    """The oracle's halves, features and target of a view, image order."""
    s = rt.HostScene(name, seed=2022)
    cam, bg = s.default_view(W / H)
    rows = rt.two_frame_rows(np.arange(H, dtype=np.uint32), H)
    params = rt.make_params(W, H, R.HALF_SPP, 50, bg, seed=R.SEED, n_frames=2)
    sums = O.render_cpu(s.desc, cam, params, rows, n_threads=THREADS)
    feat = oracle_features(O, s.desc, cam, params, rows)[0].reshape(2 * H, W)
    ref = O.render_cpu(s.desc, cam, rt.make_params(W, H, R.REF_SPP, 50, bg, seed=R.REF_SEED), np.arange(H, dtype=np.uint32), n_threads=THREADS)
    return sums[:H], sums[H:], feat[:H], feat[H:], R.display(ref, R.REF_SPP)


def baselines(sa, sb, fa, fb, target, W, H):
    noisy = sa + sb
    single = restate_single(noisy, R.add_features(fa, fb), rt.denoise_params(W, H, 2 * R.HALF_SPP))
    return R.mse(noisy, 2 * R.HALF_SPP, target), R.mse(single, 2 * R.HALF_SPP, target)


def mse_dual(sa, sb, fa, fb, target, W, H, sc, vi, vf):
    p, q = R.dual_blocks(rt, W, H, R.HALF_SPP, sigma_color=sc, var_iter=vi, var_floor=vf)
    return R.mse(R.restate_dual(sa, sb, fa, fb, p, q)[0], 2 * R.HALF_SPP, target)


def main():
    print("# tools/denoise_dual_grid.py: CPU oracle renders (2 frames x %d spp, seed %d; target %d spp, seed %d), numpy restatements"
          % (R.HALF_SPP, R.SEED, R.REF_SPP, R.REF_SEED))
    views = [(v, view_inputs(*v)) for v in R.GRID_VIEWS]
    base = {}
    for (name, W, H), inp in views:
        base[name] = baselines(*inp, W, H)
        print("view %-13s %dx%d  mse_noisy %.6e  mse_single %.6e  single/noisy %.4f" % (name, W, H, *base[name], base[name][1] / base[name][0]),
              flush=True)
    print("# grid: mse_dual and mse_dual / mse_noisy per view, then the sum of the three ratios")
    best = None
    for sc, vi, vf in itertools.product(SIGMA_COLOR, VAR_ITER, VAR_FLOOR):
        cells, total = [], 0.0
        for (name, W, H), inp in views:
            m = mse_dual(*inp, W, H, sc, vi, vf)
            total += m / base[name][0]
            cells.append("%s %.6e %.4f" % (name, m, m / base[name][0]))
        print("sigma_color %-4g var_iter %d var_floor %-6g  %s  sum %.4f" % (sc, vi, vf, "  ".join(cells), total), flush=True)
        if best is None or total < best[0]:
            best = (total, sc, vi, vf)
    total, sc, vi, vf = best
    print("# chosen (smallest sum): sigma_color %g var_iter %d var_floor %g  sum %.4f" % (sc, vi, vf, total))
    print("# at the chosen point: mse_noisy, mse_single, mse_dual, dual/noisy, dual/single, and whether dual <= 0.95 * single")
    for (name, W, H), inp in views + [(R.HELD_OUT_VIEW, view_inputs(*R.HELD_OUT_VIEW))]:
        noisy, single = base[name] if name in base else baselines(*inp, W, H)
        m = mse_dual(*inp, W, H, sc, vi, vf)
        print("%s %-13s mse_noisy %.6e  mse_single %.6e  mse_dual %.6e  dual/noisy %.4f  dual/single %.4f  margin %s"
              % ("held-out" if name == R.HELD_OUT_VIEW[0] else "grid    ", name, noisy, single, m, m / noisy, m / single,
                 "yes" if m <= 0.95 * single else "no"), flush=True)


if __name__ == "__main__":
    main()
