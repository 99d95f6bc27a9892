#!/usr/bin/env python3
"""The closed-form radiometry cases (tests/radiometry_cases.py) on the CPU oracle and, with --gpu, on the HIP path: one line
N, M, L, z, se/L per case and run, and the SE_REL / H_SE_REL tables of tests/radiometry_cases.py (the largest se / L of the
CPU oracle per case and N, over the tests' seed and a second one).

    python tools/radiometry_report.py --threads 8 > profiles/radiometry.log       # CPU: 2^18 and 2^24 samples per case
    python tools/radiometry_report.py --gpu --no-cpu >> profiles/radiometry.log   # the HIP path at 2^24
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import radiometry_cases as RC  # noqa: E402
import raytracer_2022_amd as rt  # noqa: E402
from oracle import oracle_ffi as O  # noqa: E402

SHAPES = {18: (256, 1024), 24: (4096, 4096)}
SEEDS = {18: RC.SEED_CPU, 24: RC.SEED_GPU}
H_SPP = {18: 64, 24: 4096}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--log2n", type=int, nargs="*", default=[18, 24])
    a = ap.parse_args()
    se_rel, h_se_rel, c_se_rel = {}, {}, {}
    if not a.no_cpu:
        for name, case in RC.CASES.items():
            _, desc = case["scene"](rt)
            for k in a.log2n:
                n_rays, spp = SHAPES[k]
                for seed in (SEEDS[k], SEEDS[k] + 1000):
                    sums = O.radiance(desc, RC.case_rays(rt, case, n_rays, seed), spp=spp, background=tuple(case["background"]),
                                      depth=case["depth"], n_threads=a.threads)
                    r = RC.check(name, sums, spp, tag="cpu")
                    se_rel.setdefault(name, {})[k] = max(r, se_rel.get(name, {}).get(k, 0.0))
        _, desc = RC.camera_scene(rt)
        for ap_ in RC.H_APERTURES:
            for k in a.log2n:
                for seed in (SEEDS[k], SEEDS[k] + 1000):
                    p = rt.make_params(RC.H_W, RC.H_H, H_SPP[k], 50, (0, 0, 0), seed=seed)
                    sums = O.render_cpu(desc, RC.camera(rt, ap_), p, np.arange(RC.H_H), n_threads=a.threads)
                    r = RC.check_camera(sums, H_SPP[k], tag="cpu  H_camera_ap%.1f" % ap_)
                    h_se_rel.setdefault(ap_, {})[H_SPP[k]] = max(r, h_se_rel.get(ap_, {}).get(H_SPP[k], 0.0))
        _, desc = RC.CASES["C_two_lights_bg"]["scene"](rt)
        for k in a.log2n:
            for seed in (SEEDS[k], SEEDS[k] + 1000):
                p = rt.make_params(RC.C_CAM_W, RC.C_CAM_H, H_SPP[k], 2, tuple(RC.BG_C), seed=seed)
                sums = O.render_cpu(desc, RC.narrow_camera(rt), p, np.arange(RC.C_CAM_H), n_threads=a.threads)
                r = RC.check("C_two_lights_bg", sums.reshape(-1, 3), H_SPP[k], tag="cpu camera")
                c_se_rel[H_SPP[k]] = max(r, c_se_rel.get(H_SPP[k], 0.0))
        print("SE_REL = {")
        for name, d in se_rel.items():
            print('    "%s": {%s},' % (name, ", ".join("%d: %.3e" % kv for kv in sorted(d.items()))))
        print("}")
        print("H_SE_REL = {%s}" % ", ".join("%.1f: {%s}" % (k, ", ".join("%d: %.3e" % kv for kv in sorted(d.items())))
                                            for k, d in h_se_rel.items()))
        print("C_CAM_SE_REL = {%s}" % ", ".join("%d: %.3e" % kv for kv in sorted(c_se_rel.items())))
    if a.gpu:
        import torch
        assert torch.cuda.is_available()
        torch.zeros(1, device="cuda")
        n_rays, spp = SHAPES[24]
        for name, case in RC.CASES.items():
            _, desc = case["scene"](rt)
            dev = rt.DeviceScene(desc)
            sums = dev.radiance(RC.case_rays(rt, case, n_rays, RC.SEED_GPU), spp=spp, background=tuple(case["background"]),
                                max_depth=case["depth"])
            RC.check(name, sums, spp, tag="gpu")
        _, desc = RC.CASES["C_two_lights_bg"]["scene"](rt)
        dev = rt.DeviceScene(desc)
        p = rt.make_params(RC.C_CAM_W, RC.C_CAM_H, H_SPP[24], 2, tuple(RC.BG_C), seed=RC.SEED_GPU)
        for engine in ("mega", "wavefront"):
            dev.set_engine(engine)
            sums = dev.render(RC.narrow_camera(rt), p, np.arange(RC.C_CAM_H))
            RC.check("C_two_lights_bg", sums.reshape(-1, 3), H_SPP[24], tag="gpu camera, %s" % engine)
        _, desc = RC.camera_scene(rt)
        dev = rt.DeviceScene(desc)
        for ap_ in RC.H_APERTURES:
            p = rt.make_params(RC.H_W, RC.H_H, H_SPP[24], 50, (0, 0, 0), seed=RC.SEED_GPU)
            RC.check_camera(dev.render(RC.camera(rt, ap_), p, np.arange(RC.H_H)), H_SPP[24], tag="gpu  H_camera_ap%.1f" % ap_)


if __name__ == "__main__":
    main()
