#!/usr/bin/env python3
"""What the scatter step (rt_scatter_device) costs, beside the query that feeds it and beside the engine it restates.

    python3 tools/scatter_bench.py --scene headline|c2|c4|c5 [--steps 10] [--warmup 3] [--spp 2] [--depth 50] [--seed 7]

One scene per run (a run is one step of a GPU job: give each its own time limit). The workload is the camera rays of an 800x800
view of the scene's default camera, one pinhole ray per pixel (640 000 records), generated on the host from --seed. Two JSON lines:

  "step": rt_scatter_device on the first-hit records of those rays beside rt_intersect_device on the same rays: three alternating
      windows of --steps warm calls each between two HIP events, ms per call (best window and the windows' spread), the
      statuses of the records, and rt_intersect_device on as many all-zero rays (what a query of ended entries costs).
  "loop": the whole device loop a caller would drive — torch buffers, rt_intersect_device -> rt_scatter_device chained with prev,
      --depth steps, no compaction, no early stop (that needs a read-back), every step's records kept for the unwinding — for
      --spp samples, beside rt_radiance_device on the same rays at the same spp and depth. Events round every call give the loop's
      time and its split into queries and scatter steps; the records say how many query entries were live: the rest of the
      queries' time went to dead lanes (an ended entry's next ray is all zeros and still goes through rt_intersect_device).
      The records are then unwound on the host (rt.unwind) and compared with rt_radiance_device's sums bit for bit.
"""
import argparse
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
    "headline": ("final_scene", 0, True),
    "c2": ("random_scene", 0, False),
    "c4": ("cornell_box", 0, False),
    "c5": ("wwscene", 3, True),
}
W = H = 800


def camera_rays(cam, g):
    n = W * H
    idx = np.arange(n)
    u, v = (idx % W + 0.5) / (W - 1), (idx // W + 0.5) / (H - 1)
    o = np.array(cam.origin[:])
    d = np.array(cam.lower_left_corner[:]) + u[:, None] * np.array(cam.horizontal[:]) + v[:, None] * np.array(cam.vertical[:]) - o
    return rt.radiance_rays(o, d, time=g.uniform(cam.time0, cam.time1, n), rng_state=g.integers(0, 2**63, n, dtype=np.uint64))


def window(torch, stream, call, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=list(SCENES), required=True)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch
    name, param, assets = SCENES[a.scene]
    s = rt.HostScene(name, seed=2022, param=param, assets_dir=ASSETS if assets and os.path.isdir(ASSETS) else None)
    dev = rt.DeviceScene(s.desc)
    cam, bg = s.default_view(W / H)
    bg = tuple(bg)
    rays = camera_rays(cam, np.random.default_rng(a.seed))
    n = len(rays)
    stream = torch.cuda.Stream()
    sp = rt.scatter_params(bg)
    f64max = float(np.finfo(np.float64).max)

    def query_rays_of(sample):
        return rt.query_rays(rays["origin"], rays["direction"], rays["time"], 0.001, f64max, rt.path_key(rays["rng_state"], 0, 0, sample))

    d_q0 = torch.from_numpy(query_rays_of(0).view(np.uint8)).cuda()
    d_rays = torch.empty_like(d_q0)
    d_hits = torch.empty(n * 96, dtype=torch.uint8, device="cuda")
    d_next = torch.empty(n * 80, dtype=torch.uint8, device="cuda")
    d_recs = torch.empty((a.depth, n * 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    # ---- one step on the first-hit records, beside the query of the same rays
    def query():
        dev.intersect_device(d_q0.data_ptr(), n, d_hits.data_ptr(), stream.cuda_stream)

    def scatter():
        dev.scatter_device(d_q0.data_ptr(), d_hits.data_ptr(), n, d_recs[0].data_ptr(), d_next.data_ptr(), sp, stream_ptr=stream.cuda_stream)
    for _ in range(a.warmup):
        query()
        scatter()
    # (what a query costs on entries whose path has ended: all-zero rays, as rt_scatter writes them)
    d_dead = torch.zeros(n * 80, dtype=torch.uint8, device="cuda")
    d_dead_hits = torch.empty(n * 96, dtype=torch.uint8, device="cuda")

    def query_dead():
        dev.intersect_device(d_dead.data_ptr(), n, d_dead_hits.data_ptr(), stream.cuda_stream)
    query_dead()
    t_q, t_s, t_d = [], [], []
    for _ in range(3):
        t_q.append(window(torch, stream, query, a.steps))
        t_s.append(window(torch, stream, scatter, a.steps))
        t_d.append(window(torch, stream, query_dead, a.steps))
    status = np.bincount(d_recs[0].cpu().numpy().view(F.SCATTER_REC_DTYPE)["status"], minlength=6)
    print(json.dumps({"scene": a.scene, "builder": name, "what": "step", "entries": n, "steps": a.steps,
                      "intersect_ms": round(min(t_q), 4), "scatter_ms": round(min(t_s), 4), "scatter_over_intersect": round(min(t_s) / min(t_q), 3),
                      "intersect_windows_ms": [round(x, 4) for x in t_q], "scatter_windows_ms": [round(x, 4) for x in t_s],
                      "intersect_ended_entries_ms": round(min(t_d), 4), "intersect_ended_entries_windows_ms": [round(x, 4) for x in t_d],
                      "scatter_mentries_per_s": round(n / min(t_s) / 1e3, 1), "scatter_gb_per_s": round(n * (80 + 96 + 64 + 80) / min(t_s) / 1e6, 1),
                      "status_miss_emitted_specular_diffuse_invalid_ended": status.tolist()}), flush=True)

    # ---- the whole loop beside rt_radiance_device
    def loop(sample, events=None):
        d_rays.copy_(torch.from_numpy(query_rays_of(sample).view(np.uint8)))
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for k in range(a.depth):
                if events is not None:
                    events[2 * k].record(stream)
                dev.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream.cuda_stream)
                if events is not None:
                    events[2 * k + 1].record(stream)
                dev.scatter_device(d_rays.data_ptr(), d_hits.data_ptr(), n, d_recs[k].data_ptr(), d_rays.data_ptr(), sp,
                                   d_prev_ptr=d_recs[k - 1].data_ptr() if k else None, stream_ptr=stream.cuda_stream)
            if events is not None:
                events[2 * a.depth].record(stream)
        stream.synchronize()

    d_rad_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_sums = torch.empty(n * 3, dtype=torch.float64, device="cuda")
    rp = rt.radiance_params(a.spp, bg, 0.001, a.depth)
    torch.cuda.synchronize()
    loop(0)                                                                        # warm
    dev.radiance_device(d_rad_rays.data_ptr(), n, d_sums.data_ptr(), rp, stream.cuda_stream)
    loops, engine, split, live_entries = [], [], [0.0, 0.0], 0
    total = np.zeros((n, 3))
    for r in range(3):
        st = F.rt_stats()
        dev.radiance_device(d_rad_rays.data_ptr(), n, d_sums.data_ptr(), rp, stream.cuda_stream, stats=st)
        engine.append(st.ms)
        ms = 0.0
        for sample in range(a.spp):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * a.depth + 1)]
            loop(sample, ev)
            ms += ev[0].elapsed_time(ev[-1])
            if r == 0:
                split[0] += sum(ev[2 * k].elapsed_time(ev[2 * k + 1]) for k in range(a.depth))
                split[1] += sum(ev[2 * k + 1].elapsed_time(ev[2 * k + 2]) for k in range(a.depth))
                recs = d_recs.cpu().numpy().view(F.SCATTER_REC_DTYPE)
                live = (recs["status"] == F.RT_SCATTER_SPECULAR) | (recs["status"] == F.RT_SCATTER_DIFFUSE)
                live_entries += n + int(live[:-1].sum())                           # (step k's queries are live where step k-1's records are)
                with np.errstate(all="ignore"):
                    total += rt.unwind(list(recs))
        loops.append(ms)
    want = d_sums.cpu().numpy().reshape(n, 3)
    same = bool(np.array_equal(np.isnan(total), np.isnan(want)) and np.array_equal(np.nan_to_num(total).view(np.uint64), np.nan_to_num(want).view(np.uint64)))
    queries = n * a.depth * a.spp
    print(json.dumps({"scene": a.scene, "builder": name, "what": "loop", "entries": n, "spp": a.spp, "depth": a.depth,
                      "loop_ms": round(min(loops), 2), "rt_radiance_device_ms": round(min(engine), 2), "loop_over_engine": round(min(loops) / min(engine), 3),
                      "loop_windows_ms": [round(x, 2) for x in loops], "engine_windows_ms": [round(x, 2) for x in engine],
                      "loop_intersect_ms": round(split[0], 2), "loop_scatter_ms": round(split[1], 2),
                      "query_entries": queries, "live_query_entries": live_entries, "live_share": round(live_entries / queries, 4),
                      "unwound_equals_rt_radiance": same}), flush=True)
    if not same:
        sys.exit("the unwound loop differs from rt_radiance_device")


if __name__ == "__main__":
    main()
