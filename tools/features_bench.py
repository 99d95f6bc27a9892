#!/usr/bin/env python3
"""Throughput of the first-hit feature buffers (rt_features_device) beside a closest-hit query on the same camera rays and
beside the render of the same view at the same spp.

    python3 tools/features_bench.py [--scenes final_scene,c2,c5,s1e5] [--spp 4,16] [--query-spp 4] [--steps 5] [--warmup 2]

Per scene and spp, one JSON line: the 800x800 default view, primary rays (= width * height * spp), ms per rt_features_device
call (HIP events around `steps` calls after `warmup`) and Mrays/s; the same for rt_intersect_device on the camera rays of
the view at --query-spp, generated once on the host with the render's own keying (so they are the rays the feature call
aims: the hits are compared as a by-product); and ms of rt_render_device (depth 50, spp_chunk 1) for the same view and spp.

    python3 tools/features_bench.py --surfaces [--scenes final_scene,cornell_smoke,c2] [--spp 4,16] [--no-render]

times the RT_FLAG_SURFACES call beside the plain one on the same view: three windows of each, alternating (plain, flagged, plain,
...), reported as "features_ms_windows" / "surfaces_ms_windows"; the spread of the plain windows is what a difference is read against.

    python3 tools/features_bench.py --specular [--scenes final_scene,c2] [--spp 4] [--no-render]

does the same for the RT_FLAG_SPECULAR call ("specular_ms_windows", "specular_over_plain"), and adds what a counter call of each
reports: "segments_per_sample" (rt_stats.rays / paths under the flag: the world.hit calls a sample makes) and the node visits of both,
so the time ratio can be read against the extra traversal work the flag asks for.

    python3 tools/features_bench.py --rays [--surfaces] [--specular] [--spp 4]

times rt_features_rays_device on the camera rays of the view — one ray per pixel, as a batch of width * height rt_radiance_ray
records at `spp` samples each — beside rt_features_device of the same view at the same spp, three windows of each, alternating
("features_rays_ms_windows", "rays_over_rows"), and rt_intersect_device on the same rays once; with --surfaces / --specular the
flagged forms of both calls as lines of their own.
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
    "cornell_smoke": ("cornell_smoke", 0, False),
}
W = H = 800
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def camera_rays(cam, rows, spp, seed):
    """The camera rays of the view as rt_features aims them, for a pinhole camera (lens_radius 0: the lens sample is
    multiplied by 0) — path_key, two jitter words, two lens words (first try accepted or not, the value does not matter at
    radius 0, but the word count does: rays whose first lens try is rejected are aimed with the pinhole direction and flagged),
    one shutter word. Returns (rays in (row, px, sample) order, mask of rays whose RNG state behind the camera is exact)."""
    with np.errstate(over="ignore"):
        G = np.uint64(0x9E3779B97F4A7C15)
        g = np.repeat(np.asarray(rows, dtype=np.uint64), W * spp)
        px = np.tile(np.repeat(np.arange(W, dtype=np.uint64), spp), len(rows))
        smp = np.tile(np.arange(spp, dtype=np.uint64), len(rows) * W)
        frame, py = g // np.uint64(H), g % np.uint64(H)
        h = mix64(np.uint64(seed) + G * (frame + np.uint64(1)))
        h = mix64(h ^ (np.uint64(0xD1B54A32D192ED03) * (py * np.uint64(W) + px + np.uint64(1))))
        key = mix64(h ^ (np.uint64(0x8CB92BA72F3D8DD7) * (smp + np.uint64(1))))
        word = lambda k: mix64(key + G * np.uint64(k))
        f64 = lambda w: (w >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        rng52 = lambda w, lo, hi: ((w >> np.uint64(12)) | np.uint64(0x3FF0000000000000)).view(np.float64) - 1.0
        u = (px.astype(np.float64) + f64(word(1))) / (W - 1)
        v = (py.astype(np.float64) + f64(word(2))) / (H - 1)
        lx, ly = rng52(word(3), -1, 1) * 2.0 - 1.0, rng52(word(4), -1, 1) * 2.0 - 1.0
        first_try = np.sqrt(lx * lx + ly * ly) < 1.0
        tm = cam.time0 + (cam.time1 - cam.time0) * rng52(word(5), 0, 1)
        o = np.array(cam.origin[:])
        d = np.array(cam.lower_left_corner[:]) + u[:, None] * np.array(cam.horizontal[:]) + v[:, None] * np.array(cam.vertical[:]) - o
        state = key + G * np.uint64(5)
    return rt.query_rays(o, d, time=tm, rng_state=state), first_try


def timed(torch, stream, call, steps, warmup):
    for _ in range(warmup):
        call()
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def rays_lines(a, torch, label, name, param, dev, cam, bg, rows, stream):
    """--rays: rt_features_rays_device on the view's camera rays (one per pixel, camera_rays at 1 spp with the pinhole direction;
    a batch of width * height rays) beside rt_features_device of the same view at the same spp and rt_intersect_device on the same
    rays. Three windows of each feature call, alternating; the reference of every line is rt_features_device of this build. The
    ray call traces one ray per pixel spp times where the row call jitters each sample, so the work is close, not equal."""
    q, _ = camera_rays(cam, rows, 1, a.seed)
    n = len(q)
    rays = rt.radiance_rays(q["origin"], q["direction"], time=q["time"], rng_state=q["rng_state"])
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    d_q = torch.from_numpy(q.view(np.uint8)).cuda()
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    d_hits = torch.empty(n * 96, dtype=torch.uint8, device="cuda")
    d_feat = torch.empty(n * 8, dtype=torch.float64, device="cuda")
    sp = stream.cuda_stream
    q_ms = timed(torch, stream, lambda: dev.intersect_device(d_q.data_ptr(), n, d_hits.data_ptr(), sp), a.steps, a.warmup)
    for spp in [int(x) for x in a.spp.split(",")]:
        p = rt.make_params(W, H, spp, 50, bg, seed=a.seed, spp_chunk=1)
        rp = rt.radiance_params(spp, bg, p.t_min, 0)
        for flag in [None] + (["surfaces"] if a.surfaces else []) + (["specular"] if a.specular else []):
            kw = {flag: True} if flag else {}
            rows_call = lambda: dev.features_device(cam, p, d_rows.data_ptr(), H, d_feat.data_ptr(), sp, **kw)
            rays_call = lambda: dev.features_rays_device(d_rays.data_ptr(), n, d_feat.data_ptr(), rp, sp, **kw)
            windows = [(timed(torch, stream, rows_call, a.steps, a.warmup), timed(torch, stream, rays_call, a.steps, a.warmup)) for _ in range(3)]
            rows_ms, rays_ms = [w[0] for w in windows], [w[1] for w in windows]
            print(json.dumps({"scene": label, "builder": name, "param": param, "spp": spp, "flag": flag or "none", "rays": n, "samples": n * spp,
                              "features_ms_windows": [round(x, 3) for x in rows_ms], "features_rays_ms_windows": [round(x, 3) for x in rays_ms],
                              "rays_over_rows": round(min(rays_ms) / min(rows_ms), 3), "rows_spread": round(max(rows_ms) / min(rows_ms) - 1.0, 3),
                              "features_rays_msamples_per_s": round(n * spp / min(rays_ms) / 1e3, 1),
                              "query_ms": round(q_ms, 3), "query_mrays_per_s": round(n / q_ms / 1e3, 1),
                              "stack_need": dev.info()["stack_need"], "lib": os.path.basename(F.LIB_PATH)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="final_scene,c2,c5,s1e5")
    ap.add_argument("--spp", default="4,16")
    ap.add_argument("--query-spp", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--surfaces", action="store_true", help="time the RT_FLAG_SURFACES call beside the plain one")
    ap.add_argument("--specular", action="store_true", help="time the RT_FLAG_SPECULAR call beside the plain one")
    ap.add_argument("--rays", action="store_true", help="time rt_features_rays_device on the view's camera rays beside rt_features_device")
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    for label in a.scenes.split(","):
        name, param, assets = SCENES[label]
        s = rt.HostScene(name, seed=2022, param=param, assets_dir=ASSETS if assets and os.path.isdir(ASSETS) else None)
        dev = rt.DeviceScene(s.desc)
        cam, bg = s.default_view(W / H)
        rows = rt.shuffled_rows(H, a.seed)
        stream = torch.cuda.Stream()
        if a.rays:
            rays_lines(a, torch, label, name, param, dev, cam, bg, rows, stream)
            continue
        d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
        d_feat = torch.empty(H * W * 8, dtype=torch.float64, device="cuda")
        d_rgb = torch.empty(H * W * 3, dtype=torch.float64, device="cuda")
        # the query on the same camera rays, at --query-spp
        q_ms = q_rate = float("nan")
        agree = None
        if a.query_spp > 0 and cam.lens_radius == 0.0:
            rays, exact = camera_rays(cam, rows, a.query_spp, a.seed)
            d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
            d_hits = torch.empty(len(rays) * 96, dtype=torch.uint8, device="cuda")
            q_ms = timed(torch, stream, lambda: dev.intersect_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), stream.cuda_stream), a.steps, a.warmup)
            q_rate = len(rays) / q_ms / 1e3
            hits = d_hits.cpu().numpy().view(rt.HIT_DTYPE)
            p = rt.make_params(W, H, a.query_spp, 50, bg, seed=a.seed)
            feat = dev.features(cam, p, rows)
            # by-product: where every ray of a pixel is exact, the summed depth of the query's hits is the feature call's
            t = np.where(hits["hit"] == 1, hits["t"], 0.0).reshape(H, W, a.query_spp)
            ok = exact.reshape(H, W, a.query_spp).all(axis=2)
            acc = np.zeros((H, W))
            for k in range(a.query_spp):
                acc = acc + t[:, :, k]
            agree = bool(np.array_equal(acc[ok], feat["depth"][ok]))
        for spp in [int(x) for x in a.spp.split(",")]:
            p = rt.make_params(W, H, spp, 50, bg, seed=a.seed, spp_chunk=1)
            f_ms = timed(torch, stream, lambda: dev.features_device(cam, p, d_rows.data_ptr(), H, d_feat.data_ptr(), stream.cuda_stream), a.steps, a.warmup)
            extra = {}
            if a.surfaces:
                call = lambda flag: timed(torch, stream, lambda: dev.features_device(cam, p, d_rows.data_ptr(), H, d_feat.data_ptr(), stream.cuda_stream,
                                                                                     surfaces=flag), a.steps, a.warmup)
                windows = [(call(False), call(True)) for _ in range(3)]
                plain_ms, surf_ms = [w[0] for w in windows], [w[1] for w in windows]
                extra = {"features_ms_windows": [round(x, 3) for x in plain_ms], "surfaces_ms_windows": [round(x, 3) for x in surf_ms],
                         "surfaces_over_plain": round(min(surf_ms) / min(plain_ms), 3),
                         "plain_spread": round(max(plain_ms) / min(plain_ms) - 1.0, 3), "media": s.desc.n_media}
            if a.specular:
                call = lambda flag: timed(torch, stream, lambda: dev.features_device(cam, p, d_rows.data_ptr(), H, d_feat.data_ptr(), stream.cuda_stream,
                                                                                     specular=flag), a.steps, a.warmup)
                windows = [(call(False), call(True)) for _ in range(3)]
                plain_ms, spec_ms = [w[0] for w in windows], [w[1] for w in windows]
                st0, st1 = F.rt_stats(), F.rt_stats()
                dev.features_device(cam, p, d_rows.data_ptr(), H, d_feat.data_ptr(), stream.cuda_stream, stats=st0)
                dev.features_device(cam, p, d_rows.data_ptr(), H, d_feat.data_ptr(), stream.cuda_stream, stats=st1, specular=True)
                extra.update({"features_ms_windows": [round(x, 3) for x in plain_ms], "specular_ms_windows": [round(x, 3) for x in spec_ms],
                              "specular_over_plain": round(min(spec_ms) / min(plain_ms), 3),
                              "plain_spread": round(max(plain_ms) / min(plain_ms) - 1.0, 3),
                              "segments_per_sample": round(st1.rays / st1.paths, 4), "node_visits_plain": st0.node_visits,
                              "node_visits_specular": st1.node_visits})
            r_ms = float("nan")
            if not a.no_render:
                st = F.rt_stats()
                dev.render_device(cam, p, d_rows.data_ptr(), H, d_rgb.data_ptr(), stream.cuda_stream, st)       # warm-up (the pool is allocated here)
                dev.wait(stream.cuda_stream)
                ms = []
                for _ in range(max(1, a.steps // 2)):
                    dev.render_device(cam, p, d_rows.data_ptr(), H, d_rgb.data_ptr(), stream.cuda_stream, st)
                    dev.wait(stream.cuda_stream)
                    ms.append(st.ms)
                r_ms = float(np.median(ms))
            n = W * H * spp
            print(json.dumps({**extra, "scene": label, "builder": name, "param": param, "spp": spp, "primary_rays": n,
                              "features_ms": round(f_ms, 3), "features_mrays_per_s": round(n / f_ms / 1e3, 1),
                              "query_spp": a.query_spp, "query_ms": round(q_ms, 3), "query_mrays_per_s": round(q_rate, 1),
                              "features_vs_query": round(n / f_ms / 1e3 / q_rate, 3), "render_ms": round(r_ms, 3),
                              "render_vs_features": round(r_ms / f_ms, 2), "query_depths_agree": agree,
                              "stack_need": dev.info()["stack_need"], "lib": os.path.basename(F.LIB_PATH)}), flush=True)


if __name__ == "__main__":
    main()
