#!/usr/bin/env python3
"""Throughput of the closest-hit queries (rt_intersect_device) beside the render's own traversal rate on the same scene.

    python3 tools/query_bench.py [--scenes final_scene,c2,c5,s1e5] [--steps 5] [--warmup 2] [--any-hit] [--seed 7]

Per scene, two workloads generated on the host from --seed (two runs give the same rays):
  (a) camera rays of an 800x800 view of the scene's default camera (pinhole: the lens is not sampled), 4 jittered samples
      per pixel, times uniform in the camera's shutter, rng_state = ray index;
  (b) one diffuse bounce from (a)'s hits: origin p, direction normal + a random unit vector; misses dropped (incoherent).
--any-hit also times (b) under RT_FLAG_ANY_HIT on the scenes without a ConstantMedium.
One JSON line per (scene, workload): rays, ms (HIP events around `steps` calls after `warmup`, per call), Mrays/s, and the
render's traversal rate on the same scene — `rays` of an RT_FLAG_COUNTERS render divided by `trace_ms` of a plain
RT_FLAG_KERNEL_TIMES render of the same frame (800x800, --render-spp samples (1000: the headline's frame), depth 50).
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
    "s1e5": ("random_scene", 158, False),
}


def camera_workload(cam, W, H, spp, g):
    n = W * H * spp
    idx = np.arange(n)
    px, py = (idx // spp) % W, (idx // spp) // W
    u = (px + g.random(n)) / (W - 1)
    v = (py + g.random(n)) / (H - 1)
    o = np.array(cam.origin[:])
    d = np.array(cam.lower_left_corner[:]) + u[:, None] * np.array(cam.horizontal[:]) + v[:, None] * np.array(cam.vertical[:]) - o
    return rt.query_rays(o, d, time=g.uniform(cam.time0, cam.time1, n))


def bounce_workload(hits, g):
    h = hits[hits["hit"] == 1]
    r = g.normal(size=(len(h), 3))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    return rt.query_rays(h["p"], h["normal"] + r, time=g.random(len(h)))


def time_queries(torch, dev, rays, any_hit, steps, warmup):
    stream = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_hits = torch.empty(len(rays) * 96, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(warmup):
        dev.intersect_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), stream.cuda_stream, any_hit=any_hit)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        dev.intersect_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), stream.cuda_stream, any_hit=any_hit)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps, d_hits.cpu().numpy().view(rt.HIT_DTYPE)


def render_traversal_rate(dev, s, seed, spp):
    if spp <= 0:
        return float("nan"), 0, 0.0
    W, H = 800, 800
    cam, bg = s.default_view(W / H)
    rows = rt.shuffled_rows(H, seed)
    p = rt.make_params(W, H, spp, 50, bg, seed=seed)
    _, st = dev.render(cam, p, rows, want_stats=True)
    p.flags |= F.RT_FLAG_KERNEL_TIMES
    rows_c = np.ascontiguousarray(rows, dtype=np.uint32)
    p.n_rows = len(rows_c)
    p.row_ids = rows_c.ctypes.data
    out = np.empty((H, W, 3))
    kt = F.rt_stats()
    F.check(F.lib().rt_render(dev._h, C.byref(cam), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(kt)))
    return st.rays / kt.trace_ms / 1e3, st.rays, kt.trace_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--any-hit", action="store_true")
    ap.add_argument("--render-spp", type=int, default=1000, help="samples per pixel of the render whose traversal rate is given (0: none)")
    a = ap.parse_args()
    import torch
    for label in a.scenes.split(","):
        name, param, assets = SCENES[label]
        s = rt.HostScene(name, seed=2022, param=param, assets_dir=ASSETS if assets and os.path.isdir(ASSETS) else None)
        dev = rt.DeviceScene(s.desc)
        render_rate, render_rays, trace_ms = render_traversal_rate(dev, s, a.seed, a.render_spp)
        g = np.random.default_rng(a.seed)
        cam, _ = s.default_view(1.0)
        cam_rays = camera_workload(cam, 800, 800, 4, g)
        ms_a, hits_a = time_queries(torch, dev, cam_rays, False, a.steps, a.warmup)
        bounce = bounce_workload(hits_a, g)
        runs = [("camera", cam_rays, False, ms_a), ("bounce", bounce, False, None)]
        if a.any_hit and s.desc.n_media == 0:
            runs.append(("bounce_any_hit", bounce, True, None))
        for workload, rays, any_hit, ms in runs:
            if ms is None:
                ms, _ = time_queries(torch, dev, rays, any_hit, a.steps, a.warmup)
            rate = len(rays) / ms / 1e3
            print(json.dumps({"scene": label, "builder": name, "param": param, "workload": workload, "rays": len(rays),
                              "ms": round(ms, 3), "mrays_per_s": round(rate, 1), "render_trace_mrays_per_s": round(render_rate, 1),
                              "render_rays": render_rays, "render_trace_ms": round(trace_ms, 3),
                              "vs_render": round(rate / render_rate, 3), "stack_need": dev.info()["stack_need"]}), flush=True)


if __name__ == "__main__":
    main()
