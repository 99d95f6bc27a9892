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

    python3 tools/query_bench.py --order [--origin-bits 10 --dir-bits 4 --layout origin_first] [--rounds 5]
    python3 tools/query_bench.py --order-grid

--order: what ray ordering buys. Per scene the workloads are (a), (a) shuffled and (b); per workload, in one process and
alternating over --rounds rounds, the unordered rt_intersect_device, rt_ray_order_device alone and rt_intersect_ordered_device
alone (under the order the second computed), --steps warm calls each between two HIP events: the median round per call, the
spread of the rounds, the sum of the last two and its ratio to the first. The ordered hits are compared with the unordered
ones byte for byte; gather_scatter_ms is the ordered call under the identity order less the unordered call: the two moves alone.
--order-grid: origin_bits {0, 5, 10, 16} x dir_bits {0, 2, 4, 6} x the three layouts on (b) of every scene
of --scenes, one line per cell, then the cells with the smallest time summed over the scenes (RAY_ORDER_DEFAULTS is the first).
Neither renders anything.
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


LAYOUT_NAMES = {"origin_first": F.RT_ORDER_ORIGIN_FIRST, "direction_first": F.RT_ORDER_DIRECTION_FIRST, "face_origin_uv": F.RT_ORDER_FACE_ORIGIN_UV}
GRID_ORIGIN_BITS, GRID_DIR_BITS = (0, 5, 10, 16), (0, 2, 4, 6)


class OrderBench:
    """The buffers of one workload for the three calls that are compared — the unordered rt_intersect_device, rt_ray_order_device
    and rt_intersect_ordered_device — all on one stream, and their times from HIP events round warm calls."""

    def __init__(self, torch, dev, rays):
        self.torch, self.dev, self.n = torch, dev, len(rays)
        self.stream = torch.cuda.Stream()
        self.d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
        self.d_hits = torch.empty(self.n * 96, dtype=torch.uint8, device="cuda")
        self.d_hits_ordered = torch.empty(self.n * 96, dtype=torch.uint8, device="cuda")
        self.d_order = torch.empty(self.n, dtype=torch.int32, device="cuda")
        self.ws_order = torch.empty(rt.ray_order_workspace_bytes(self.n), dtype=torch.uint8, device="cuda")
        self.ws = torch.empty(rt.intersect_ordered_workspace_bytes(self.n), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def plain(self):
        self.dev.intersect_device(self.d_rays.data_ptr(), self.n, self.d_hits.data_ptr(), self.stream.cuda_stream)

    def order(self, p):
        rt.ray_order_device(self.d_rays.data_ptr(), self.n, p, self.d_order.data_ptr(), self.ws_order.data_ptr(), self.ws_order.numel(),
                            stream_ptr=self.stream.cuda_stream)

    def ordered(self):
        self.dev.intersect_ordered_device(self.d_rays.data_ptr(), self.d_order.data_ptr(), self.n, self.d_hits_ordered.data_ptr(),
                                          self.ws.data_ptr(), self.ws.numel(), stream_ptr=self.stream.cuda_stream)

    def ms(self, call, steps, warmup):
        for _ in range(warmup):
            call()
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        for _ in range(steps):
            call()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    def same_hits(self):
        return bool(self.torch.equal(self.d_hits, self.d_hits_ordered))


def order_workloads(torch, dev, cam, g):
    """camera rays, the same rays shuffled, and one bounce from their hits → [(name, rays)]"""
    cam_rays = camera_workload(cam, 800, 800, 4, g)
    _, hits = time_queries(torch, dev, cam_rays, False, 1, 0)
    return [("camera", cam_rays), ("camera_shuffled", np.ascontiguousarray(cam_rays[g.permutation(len(cam_rays))])),
            ("bounce", bounce_workload(hits, g))]


def order_compare(torch, label, dev, workloads, p, steps, warmup, rounds):
    """Per workload: `rounds` rounds of (unordered, ordering, ordered) one after the other, `steps` warm calls each; the median of
    the rounds and their spread, per call. One JSON line per workload."""
    for name, rays in workloads:
        b = OrderBench(torch, dev, rays)
        b.order(p)
        t = {"unordered": [], "order": [], "ordered": []}
        for r in range(rounds):
            t["unordered"].append(b.ms(b.plain, steps, warmup if r == 0 else 1))
            t["order"].append(b.ms(lambda: b.order(p), steps, warmup if r == 0 else 1))
            t["ordered"].append(b.ms(b.ordered, steps, warmup if r == 0 else 1))
        assert b.same_hits(), "ordered hits differ from rt_intersect_device's"
        b.d_order.copy_(torch.arange(b.n, dtype=torch.int32, device="cuda"))       # the identity: the same work, plus the two moves
        torch.cuda.synchronize()
        moves = float(np.median([b.ms(b.ordered, steps, 1) - b.ms(b.plain, steps, 1) for _ in range(rounds)]))
        med = {k: float(np.median(v)) for k, v in t.items()}
        total = med["order"] + med["ordered"]
        print(json.dumps({"scene": label, "workload": name, "rays": b.n, "origin_bits": p.origin_bits, "dir_bits": p.dir_bits, "layout": p.layout,
                          "unordered_ms": round(med["unordered"], 3), "order_ms": round(med["order"], 3), "ordered_ms": round(med["ordered"], 3),
                          "order_plus_ordered_ms": round(total, 3), "gather_scatter_ms": round(moves, 3), "speedup_with_ordering": round(med["unordered"] / total, 3),
                          "speedup_order_given": round(med["unordered"] / med["ordered"], 3),
                          "unordered_mrays_per_s": round(b.n / med["unordered"] / 1e3, 1), "with_ordering_mrays_per_s": round(b.n / total / 1e3, 1),
                          "order_given_mrays_per_s": round(b.n / med["ordered"] / 1e3, 1),
                          "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()}, "hits_identical": True}), flush=True)


def order_grid(torch, label, dev, rays, steps, warmup):
    """The bounce rays of one scene under every cell of the grid: ordering + ordered query, `steps` warm calls each; the unordered
    call before, in the middle and after. One JSON line per cell and one for the unordered call. → {cell: summed ms}"""
    b = OrderBench(torch, dev, rays)
    cells = [(ob, db, name) for name in LAYOUT_NAMES for ob in GRID_ORIGIN_BITS for db in GRID_DIR_BITS]
    plain, out = [b.ms(b.plain, steps, warmup)], {}
    for i, (ob, db, name) in enumerate(cells):
        p = rt.ray_order_params(ob, db, LAYOUT_NAMES[name], 80)
        t_order = b.ms(lambda: b.order(p), steps, 1)
        t_ordered = b.ms(b.ordered, steps, 1)
        out[(ob, db, name)] = t_order + t_ordered
        print(json.dumps({"grid": label, "rays": b.n, "origin_bits": ob, "dir_bits": db, "layout": name, "order_ms": round(t_order, 3),
                          "ordered_ms": round(t_ordered, 3), "sum_ms": round(t_order + t_ordered, 3)}), flush=True)
        if i == len(cells) // 2 - 1:
            plain.append(b.ms(b.plain, steps, 1))
    plain.append(b.ms(b.plain, steps, 1))
    assert b.same_hits(), "ordered hits differ from rt_intersect_device's"
    print(json.dumps({"grid": label, "rays": b.n, "unordered_ms_before_middle_after": [round(x, 3) for x in plain]}), flush=True)
    return out


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
    ap.add_argument("--order", action="store_true", help="compare rt_intersect_device with rt_ray_order_device + rt_intersect_ordered_device")
    ap.add_argument("--order-grid", action="store_true", help="sweep origin_bits x dir_bits x layout on the bounce rays of --scenes")
    ap.add_argument("--rounds", type=int, default=5, help="--order: alternating rounds per workload")
    ap.add_argument("--origin-bits", type=int, default=rt.RAY_ORDER_DEFAULTS["origin_bits"])
    ap.add_argument("--dir-bits", type=int, default=rt.RAY_ORDER_DEFAULTS["dir_bits"])
    ap.add_argument("--layout", choices=list(LAYOUT_NAMES), default={v: k for k, v in LAYOUT_NAMES.items()}[rt.RAY_ORDER_DEFAULTS["layout"]])
    a = ap.parse_args()
    import torch
    grid_sum = {}
    for label in a.scenes.split(","):
        name, param, assets = SCENES[label]
        s = rt.HostScene(name, seed=2022, param=param, assets_dir=ASSETS if assets and os.path.isdir(ASSETS) else None)
        dev = rt.DeviceScene(s.desc)
        if a.order or a.order_grid:
            g = np.random.default_rng(a.seed)
            workloads = order_workloads(torch, dev, s.default_view(1.0)[0], g)
            if a.order:
                order_compare(torch, label, dev, workloads, rt.ray_order_params(a.origin_bits, a.dir_bits, LAYOUT_NAMES[a.layout], 80), a.steps,
                              a.warmup, a.rounds)
            if a.order_grid:
                for cell, ms in order_grid(torch, label, dev, workloads[2][1], a.steps, a.warmup).items():
                    grid_sum[cell] = grid_sum.get(cell, 0.0) + ms
            continue
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
    if grid_sum:
        ranked = sorted(grid_sum.items(), key=lambda kv: kv[1])
        for (ob, db, layout), ms in ranked[:5] + ranked[-1:]:
            print(json.dumps({"grid_total_over": a.scenes, "origin_bits": ob, "dir_bits": db, "layout": layout, "sum_ms": round(ms, 3)}), flush=True)
        (ob, db, layout), ms = ranked[0]
        print(json.dumps({"grid_best": {"origin_bits": ob, "dir_bits": db, "layout": layout}, "sum_ms": round(ms, 3), "scenes": a.scenes}), flush=True)


if __name__ == "__main__":
    main()
