#!/usr/bin/env python3
"""Build time and tree quality of the device BVH builder (rt_bvh_build_device) beside the host builder's median-split trees.

    python3 tools/bvh_bench.py [--scenes c5,s1e5,s1e6] [--steps 5] [--warmup 2] [--size 400] [--spp 16] [--seed 7]

Per scene (c5: wwscene at three subdivision levels; s1e5 / s1e6: random_scene with 158^2 * 4 / 500^2 * 4 small spheres):
  build   the leaves of the root tree and their boxes (rtb_ref_boxes); device time of rt_bvh_build_device on them (HIP events
          round `steps` calls after `warmup`, per call, upload not included) beside the wall time of ONE rtb_bvh_build call on
          the same leaves and boxes (the host mirror of BvhNode::new: random axis, sort, median split, one thread);
  tree    for the description as the host layer built it ("reference") and for rebuild_bvh's ("lbvh"): node_visits / rays and
          prim_tests / rays of an RT_FLAG_COUNTERS render (size x size, spp samples, depth 50, the scene's default view), Mrays/s
          of a timed render of the same frame (rays of the counter run over the render's device ms, and over its traversal ms),
          stack_need and the wf_trace instance the scene selects.
One JSON line per record. Nothing here asserts: the numbers are reported whichever way they fall."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import raytracer_2022_amd as rt  # noqa: E402
from raytracer_2022_amd import _ffi as F  # noqa: E402

ASSETS = os.path.join(ROOT, "assets")
SCENES = {"c5": ("wwscene", 3, True), "s1e5": ("random_scene", 158, False), "s1e6": ("random_scene", 500, False)}


def device_build_ms(torch, refs, boxes, steps, warmup):
    n = len(refs)
    d_refs = torch.from_numpy(refs.view(np.int32).copy()).cuda()
    d_boxes = torch.from_numpy(boxes.copy()).cuda()
    d_out = torch.empty(max(1, n - 1) * 64, dtype=torch.uint8, device="cuda")
    ws = torch.empty(rt.bvh_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    call = lambda: rt.bvh_build_device(d_refs.data_ptr(), d_boxes.data_ptr(), n, d_out.data_ptr(), ws.data_ptr(), ws.numel(), 0, stream.cuda_stream)
    for _ in range(warmup):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def host_build_s(refs, boxes, seed):
    out = np.zeros(2 * len(refs), dtype=F.BVH_NODE_DTYPE)
    t0 = time.perf_counter()
    n = F.check(F.lib().rtb_bvh_build(refs.ctypes.data_as(C.POINTER(C.c_uint32)), boxes.ctypes.data_as(C.POINTER(C.c_double)), len(refs), seed,
                                      out.ctypes.data_as(C.POINTER(F.rt_bvh_node)), len(out)))
    return time.perf_counter() - t0, n


def tree_record(desc, cam, bg, size, spp, seed):
    dev = rt.DeviceScene(desc)
    rows = rt.shuffled_rows(size, seed)
    p = rt.make_params(size, size, spp, 50, bg, seed=seed)
    _, st = dev.render(cam, p, rows, want_stats=True)
    p.flags |= F.RT_FLAG_KERNEL_TIMES
    rows_c = np.ascontiguousarray(rows, dtype=np.uint32)
    p.n_rows, p.row_ids = len(rows_c), rows_c.ctypes.data
    out = np.empty((size, size, 3))
    kt = F.rt_stats()
    F.check(F.lib().rt_render(dev._h, C.byref(cam), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(kt)))     # warm
    F.check(F.lib().rt_render(dev._h, C.byref(cam), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(kt)))
    rec = {"rays": st.rays, "node_visits_per_ray": round(st.node_visits / st.rays, 3), "prim_tests_per_ray": round(sum(st.prim_tests) / st.rays, 3),
           "render_ms": round(kt.ms, 3), "mrays_per_s": round(st.rays / kt.ms / 1e3, 1), "trace_ms": round(kt.trace_ms, 3),
           "trace_mrays_per_s": round(st.rays / kt.trace_ms / 1e3, 1), "stack_need": dev.info()["stack_need"], "n_nodes": desc.n_nodes}
    rec.update(dev.trace_variant())
    dev.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch
    for label in a.scenes.split(","):
        name, param, assets = SCENES[label]
        t0 = time.perf_counter()
        s = rt.HostScene(name, seed=2022, param=param, assets_dir=ASSETS if assets and os.path.isdir(ASSETS) else None)
        scene_s = time.perf_counter() - t0
        cam, bg = s.default_view(1.0)
        d0 = s.desc
        refs = rt.tree_leaves(d0)
        boxes = rt.ref_boxes(d0, refs, float(cam.time0), float(cam.time1))
        host_s, host_nodes = host_build_s(refs, boxes, a.seed)
        ms = device_build_ms(torch, refs, boxes, a.steps, a.warmup)
        print(json.dumps({"scene": label, "builder": name, "param": param, "record": "build", "leaves": len(refs), "device_build_ms": round(ms, 3),
                          "host_build_ms": round(host_s * 1e3, 1), "host_nodes": host_nodes, "host_over_device": round(host_s * 1e3 / ms, 1),
                          "workspace_mib": round(rt.bvh_workspace_bytes(len(refs)) / 2**20, 1), "scene_build_s": round(scene_s, 2)}), flush=True)
        for tree, desc in (("reference", d0), ("lbvh", rt.rebuild_bvh(d0, float(cam.time0), float(cam.time1)))):
            rec = {"scene": label, "record": "tree", "tree": tree}
            rec.update(tree_record(desc, cam, bg, a.size, a.spp, a.seed))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
