#!/usr/bin/env python3
"""Device time of the denoiser (rt_denoise_device) beside the render and the feature call of the same frame, and what it
buys: the display-value MSE against a high-spp render before and after.

    python3 tools/denoise_bench.py [--scene final_scene] [--spp 4,16] [--ref-spp 256] [--steps 20] [--warmup 3] [--n-iter 5]

Per spp, one JSON line for the 800x800 default view: ms of rt_render_device (depth 50, spp_chunk 1, median of the calls'
own rt_stats.ms), ms per rt_features_device and per rt_denoise_device call (HIP events around `steps` calls after `warmup`,
all on one stream, three windows with NULL rows and one with the frame's shuffled row list), and the MSE of sqrt(clip(c, 0, 0.999)) against a --ref-spp render at another seed, noisy and denoised.
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
W = H = 800


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


def display(sums, spp):
    return np.sqrt(np.clip(np.where(np.isnan(sums), 0.0, sums) / spp, 0.0, 0.999))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="final_scene")
    ap.add_argument("--spp", default="4,16")
    ap.add_argument("--ref-spp", type=int, default=256)
    ap.add_argument("--n-iter", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2022)
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    s = rt.HostScene(a.scene, seed=2022, assets_dir=ASSETS if os.path.isdir(ASSETS) else None)
    dev = rt.DeviceScene(s.desc)
    cam, bg = s.default_view(W / H)
    rows = rt.shuffled_rows(H, a.seed)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    d_feat = torch.empty(H * W * 8, dtype=torch.float64, device="cuda")
    d_rgb = torch.empty(H * W * 3, dtype=torch.float64, device="cuda")
    d_out = torch.empty(H * W * 3, dtype=torch.float64, device="cuda")
    st = F.rt_stats()

    def render(p, n):
        dev.render_device(cam, p, d_rows.data_ptr(), H, d_rgb.data_ptr(), sp, st)      # warm-up (the pool is allocated here)
        dev.wait(sp)
        ms = []
        for _ in range(n):
            dev.render_device(cam, p, d_rows.data_ptr(), H, d_rgb.data_ptr(), sp, st)
            dev.wait(sp)
            ms.append(st.ms)
        return float(np.median(ms)) if ms else float("nan")

    render(rt.make_params(W, H, a.ref_spp, 50, bg, seed=7, spp_chunk=1), 0)
    target = display(d_rgb.cpu().numpy().reshape(H, W, 3), a.ref_spp)
    for spp in [int(x) for x in a.spp.split(",")]:
        p = rt.make_params(W, H, spp, 50, bg, seed=a.seed, spp_chunk=1)
        f_ms = timed(torch, stream, lambda: dev.features_device(cam, p, d_rows.data_ptr(), H, d_feat.data_ptr(), sp), a.steps, a.warmup)
        r_ms = render(p, 3)
        dp = rt.denoise_params(W, H, spp, n_iter=a.n_iter)
        d_ws = torch.empty(rt.denoise_workspace_bytes(dp), dtype=torch.uint8, device="cuda")
        call = lambda r: rt.denoise_device(d_rgb.data_ptr(), d_feat.data_ptr(), dp, d_out.data_ptr(), d_ws.data_ptr(), d_row_ids_ptr=r, stream_ptr=sp)
        ms = [timed(torch, stream, lambda: call(None), a.steps, a.warmup) for _ in range(3)]
        rows_ms = timed(torch, stream, lambda: call(d_rows.data_ptr()), a.steps, a.warmup)
        noisy = d_rgb.cpu().numpy().reshape(H, W, 3)
        den = d_out.cpu().numpy().reshape(H, W, 3)
        mse = lambda img: float(np.mean((display(img, spp) - target) ** 2))
        print(json.dumps({"scene": a.scene, "spp": spp, "n_iter": a.n_iter, "render_ms": round(r_ms, 3), "features_ms": round(f_ms, 3),
                          "denoise_ms": [round(x, 4) for x in ms], "denoise_ms_with_row_list": round(rows_ms, 4),
                          "denoise_vs_render": round(min(ms) / r_ms, 5),
                          "workspace_mb": round(d_ws.numel() / 1e6, 1), "ref_spp": a.ref_spp, "mse_noisy": round(mse(noisy), 6),
                          "mse_denoised": round(mse(den), 6), "mse_ratio": round(mse(den) / mse(noisy), 3),
                          "lib": os.path.basename(F.LIB_PATH)}), flush=True)


if __name__ == "__main__":
    main()
