#!/usr/bin/env python3
"""Throughput of path-traced radiance for caller rays (rt_radiance_device) beside the render's on the same view.

    python3 tools/radiance_bench.py [--scenes final_scene,c2,c5] [--spp 64] [--steps 3] [--warmup 1] [--seed 7] [--no-probe]

Per scene, two workloads generated on the host from --seed (two runs give the same rays):
  (a) camera: one pinhole ray per pixel of an 800x800 view of the scene's default camera (the lens is not sampled; a jittered
      point of the pixel, a time in the shutter), rng_state = pixel index, --spp samples per ray;
  (b) probe (the light-probe shape): 1 024 rays from the camera's origin in directions spread over the sphere, 4 096 samples each.
One JSON line per (scene, workload): rays (`rays` of an RT_FLAG_COUNTERS call: world.hit calls), ms (rt_stats.ms of plain
calls, mean of --steps after --warmup), Mrays/s = rays / ms, and the render's Mrays/s measured the same way on an 800x800
frame of the same view at the same spp (--spp for both workloads) with spp_chunk = 1 — the two run the same kernels, only the
source of a path's first ray differs. The probe also gets a render of as many paths (32x32 pixels at its spp): a job that
fills an eighth of the path pool runs at a fraction of a full frame's rate whichever way its rays start. With --kernel-times
both also report the summed wf_trace / wf_shade device times (the pool then runs as one group of segments).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import raytracer_2022_amd as rt  # noqa: E402
from raytracer_2022_amd import _ffi as F  # noqa: E402

ASSETS = os.path.join(ROOT, "assets")
SCENES = {                       # label: (builder, param, assets)
    "final_scene": ("final_scene", 0, True),
    "c2": ("random_scene", 0, False),
    "c5": ("wwscene", 3, True),
}


def camera_workload(cam, W, H, g):
    n = W * H
    idx = np.arange(n)
    px, py = idx % W, idx // W
    u = (px + g.random(n)) / (W - 1)
    v = (py + g.random(n)) / (H - 1)
    o = np.array(cam.origin[:])
    d = np.array(cam.lower_left_corner[:]) + u[:, None] * np.array(cam.horizontal[:]) + v[:, None] * np.array(cam.vertical[:]) - o
    return rt.radiance_rays(o, d, time=g.uniform(cam.time0, cam.time1, n))


def probe_workload(cam, n, g):
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return rt.radiance_rays(np.array(cam.origin[:]), d, time=g.uniform(cam.time0, cam.time1, n))


def time_radiance(torch, dev, rays, spp, bg, steps, warmup, kernel_times):
    stream = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_out = torch.empty((len(rays), 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    st = F.rt_stats()
    dev.radiance_device(d_rays.data_ptr(), len(rays), d_out.data_ptr(), rt.radiance_params(spp, bg, flags=F.RT_FLAG_COUNTERS),
                        stream.cuda_stream, st)
    rays_traced = st.rays
    plain = rt.radiance_params(spp, bg, flags=F.RT_FLAG_KERNEL_TIMES if kernel_times else 0)
    ms = trace = shade = 0.0
    for i in range(warmup + steps):
        dev.radiance_device(d_rays.data_ptr(), len(rays), d_out.data_ptr(), plain, stream.cuda_stream, st)
        if i >= warmup:
            ms += st.ms / steps
            trace += st.trace_ms / steps
            shade += st.shade_ms / steps
    return rays_traced, ms, trace, shade


def time_render(dev, s, seed, spp, steps, warmup, kernel_times, W=800, H=800):
    cam, bg = s.default_view(W / H)
    rows = rt.shuffled_rows(H, seed)
    p = rt.make_params(W, H, spp, 50, bg, seed=seed, spp_chunk=1)
    _, st = dev.render(cam, p, rows, want_stats=True)
    rows_c = np.ascontiguousarray(rows, dtype=np.uint32)
    p.n_rows = len(rows_c)
    p.row_ids = rows_c.ctypes.data
    p.flags = F.RT_FLAG_KERNEL_TIMES if kernel_times else 0
    out = np.empty((H, W, 3))
    ms = trace = shade = 0.0
    for i in range(warmup + steps):
        kt = F.rt_stats()
        F.check(F.lib().rt_render(dev._h, C.byref(cam), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(kt)))
        if i >= warmup:
            ms += kt.ms / steps
            trace += kt.trace_ms / steps
            shade += kt.shade_ms / steps
    return st.rays, ms, trace, shade


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--probe-rays", type=int, default=1024)
    ap.add_argument("--probe-spp", type=int, default=4096)
    ap.add_argument("--no-probe", action="store_true")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--kernel-times", action="store_true")
    a = ap.parse_args()
    import torch
    for label in a.scenes.split(","):
        name, param, assets = SCENES[label]
        s = rt.HostScene(name, seed=2022, param=param, assets_dir=ASSETS if assets and os.path.isdir(ASSETS) else None)
        dev = rt.DeviceScene(s.desc)
        r_rays, r_ms, r_trace, r_shade = time_render(dev, s, a.seed, a.spp, a.steps, a.warmup, a.kernel_times)
        render_rate = r_rays / r_ms / 1e3
        g = np.random.default_rng(a.seed)
        cam, bg = s.default_view(1.0)
        runs = [("camera", camera_workload(cam, 800, 800, g), a.spp)]
        if not a.no_probe:
            runs.append(("probe", probe_workload(cam, a.probe_rays, g), a.probe_spp))
        for workload, rays, spp in runs:
            n_traced, ms, trace, shade = time_radiance(torch, dev, rays, spp, tuple(bg), a.steps, a.warmup, a.kernel_times)
            rate = n_traced / ms / 1e3
            row = {"scene": label, "builder": name, "param": param, "workload": workload, "n_rays": len(rays), "spp": spp,
                   "rays": n_traced, "ms": round(ms, 3), "mrays_per_s": round(rate, 1),
                   "render_spp": a.spp, "render_rays": r_rays, "render_ms": round(r_ms, 3), "render_mrays_per_s": round(render_rate, 1),
                   "vs_render": round(rate / render_rate, 3)}
            if workload == "probe":                  # (a render of as many paths: 32x32 pixels at the probe's spp)
                side = max(2, int(round(len(rays) ** 0.5)))
                p_rays, p_ms, _, _ = time_render(dev, s, a.seed, spp, a.steps, a.warmup, False, side, side)
                row.update({"render_same_paths": "%dx%dx%d" % (side, side, spp), "render_same_paths_mrays_per_s": round(p_rays / p_ms / 1e3, 1),
                            "vs_render_same_paths": round(rate / (p_rays / p_ms / 1e3), 3)})
            if a.kernel_times:
                row.update({"trace_ms": round(trace, 3), "shade_ms": round(shade, 3), "render_trace_ms": round(r_trace, 3),
                            "render_shade_ms": round(r_shade, 3)})
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
