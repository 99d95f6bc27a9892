#!/usr/bin/env python3
"""Device time of the denoiser (rt_denoise_device) beside the render and the feature call of the same frame, and what it
buys: the display-value MSE against a high-spp render before and after.

    python3 tools/denoise_bench.py [--scene final_scene] [--spp 4,16] [--ref-spp 256] [--steps 20] [--warmup 3] [--n-iter 5]

Per spp, one JSON line for the 800x800 default view: ms of rt_render_device (depth 50, spp_chunk 1, median of the calls'
own rt_stats.ms), ms per rt_features_device and per rt_denoise_device call (HIP events around `steps` calls after `warmup`,
all on one stream, three windows with NULL rows and one with the frame's shuffled row list), and the MSE of sqrt(clip(c, 0, 0.999)) against a --ref-spp render at another seed, noisy and denoised.

--dual: per spp (taken as the frame's total, so each half has spp / 2 samples) one more JSON line for the variance-guided filter
(rt_denoise_dual_device) at the package's defaults: the ONE two-frame render and the ONE two-frame feature call that give the
halves A and B, rt_denoise_device on A + B beside rt_denoise_dual_device on (A, B) — the same windows — and the MSE of the noisy
frame A + B, of rt_denoise's result and of the dual filter's.

--surfaces: every feature call takes RT_FLAG_SURFACES (the guides are those of the surfaces behind participating media); the
lines say "surfaces": true. Run once without and once with it to compare the MSE after the filter.

--specular: every feature call takes RT_FLAG_SPECULAR (the guides follow each sample through glass and mirrors); the lines say
"specular": true. Run once without and once with it (same seeds, same --ref-spp target) to compare the MSE of both filters under
first-hit and under specular guides.
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


def dual(a, torch, dev, cam, bg, rows, stream, spp, target, st):
    """The --dual line of a frame of `spp` samples in two halves."""
    sp, half = stream.cuda_stream, spp // 2
    n = H * W
    d_rows2 = torch.from_numpy(rt.two_frame_rows(rows, H).view(np.int32)).cuda()
    d_rows = d_rows2[:H]
    d_rgb2 = torch.empty(2 * n * 3, dtype=torch.float64, device="cuda")
    d_feat2 = torch.empty(2 * n * 8, dtype=torch.float64, device="cuda")
    d_out, d_var = torch.empty(n * 3, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    p2 = rt.make_params(W, H, half, 50, bg, seed=a.seed, n_frames=2, spp_chunk=1)
    f_ms = timed(torch, stream, lambda: dev.features_device(cam, p2, d_rows2.data_ptr(), 2 * H, d_feat2.data_ptr(), sp, surfaces=a.surfaces, specular=a.specular), a.steps, a.warmup)
    dev.render_device(cam, p2, d_rows2.data_ptr(), 2 * H, d_rgb2.data_ptr(), sp, st)       # (the pool may grow here)
    dev.wait(sp)
    ms = []
    for _ in range(3):
        dev.render_device(cam, p2, d_rows2.data_ptr(), 2 * H, d_rgb2.data_ptr(), sp, st)
        dev.wait(sp)
        ms.append(st.ms)
    r_ms = float(np.median(ms))
    d_a, d_b, d_fa, d_fb = d_rgb2[:3 * n], d_rgb2[3 * n:], d_feat2[:8 * n], d_feat2[8 * n:]
    d_sum, d_fsum = d_a + d_b, d_fa + d_fb                                                 # the 2 * half frame rt_denoise sees
    ps = rt.denoise_params(W, H, 2 * half, n_iter=a.n_iter)
    pd = rt.denoise_params(W, H, half, n_iter=a.n_iter, sigma_color=rt.DUAL_DEFAULTS["sigma_color"])
    q = rt.denoise_dual_params()
    d_ws = torch.empty(max(rt.denoise_workspace_bytes(ps), rt.denoise_dual_workspace_bytes(pd)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    single = lambda r: rt.denoise_device(d_sum.data_ptr(), d_fsum.data_ptr(), ps, d_out.data_ptr(), d_ws.data_ptr(), d_row_ids_ptr=r, stream_ptr=sp)
    both = lambda r, v=d_var.data_ptr(): rt.denoise_dual_device(d_a.data_ptr(), d_b.data_ptr(), d_fa.data_ptr(), d_fb.data_ptr(), pd, q,
                                                                d_out.data_ptr(), d_ws.data_ptr(), d_out_variance_ptr=v, d_row_ids_ptr=r, stream_ptr=sp)
    s_ms = [timed(torch, stream, lambda: single(None), a.steps, a.warmup) for _ in range(3)]
    single(d_rows.data_ptr())
    stream.synchronize()
    den_single = d_out.cpu().numpy().reshape(H, W, 3)
    d_ms = [timed(torch, stream, lambda: both(None), a.steps, a.warmup) for _ in range(3)]
    novar_ms = timed(torch, stream, lambda: both(None, None), a.steps, a.warmup)
    rows_ms = timed(torch, stream, lambda: both(d_rows.data_ptr()), a.steps, a.warmup)
    stream.synchronize()
    den_dual = d_out.cpu().numpy().reshape(H, W, 3)
    noisy = d_sum.cpu().numpy().reshape(H, W, 3)
    mse = lambda img: float(np.mean((display(img, 2 * half) - target) ** 2))
    m_noisy, m_single, m_dual = mse(noisy), mse(den_single), mse(den_dual)
    print(json.dumps({"dual": True, "scene": a.scene, "surfaces": a.surfaces, "specular": a.specular, "spp": "2 x %d" % half, "n_iter": a.n_iter, "var_iter": q.var_iter,
                      "sigma_color": pd.sigma_color, "var_floor": q.var_floor, "render_2_frames_ms": round(r_ms, 3),
                      "features_2_frames_ms": round(f_ms, 3), "denoise_ms": [round(x, 4) for x in s_ms],
                      "denoise_dual_ms": [round(x, 4) for x in d_ms], "denoise_dual_ms_without_variance_out": round(novar_ms, 4),
                      "denoise_dual_ms_with_row_list": round(rows_ms, 4), "dual_vs_single": round(min(d_ms) / min(s_ms), 3),
                      "dual_vs_render": round(min(d_ms) / r_ms, 5), "workspace_mb": round(rt.denoise_dual_workspace_bytes(pd) / 1e6, 1),
                      "ref_spp": a.ref_spp, "mse_noisy": round(m_noisy, 6), "mse_denoised": round(m_single, 6), "mse_dual": round(m_dual, 6),
                      "dual_over_noisy": round(m_dual / m_noisy, 3), "dual_over_single": round(m_dual / m_single, 3),
                      "mean_residual_variance": float(d_var.mean().item()), "lib": os.path.basename(F.LIB_PATH)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="final_scene")
    ap.add_argument("--spp", default="4,16")
    ap.add_argument("--ref-spp", type=int, default=256)
    ap.add_argument("--n-iter", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--dual", action="store_true", help="also the variance-guided filter on two half-sample frames")
    ap.add_argument("--surfaces", action="store_true", help="RT_FLAG_SURFACES on every feature call")
    ap.add_argument("--specular", action="store_true", help="RT_FLAG_SPECULAR on every feature call")
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
        f_ms = timed(torch, stream, lambda: dev.features_device(cam, p, d_rows.data_ptr(), H, d_feat.data_ptr(), sp, surfaces=a.surfaces, specular=a.specular), a.steps, a.warmup)
        r_ms = render(p, 3)
        dp = rt.denoise_params(W, H, spp, n_iter=a.n_iter)
        d_ws = torch.empty(rt.denoise_workspace_bytes(dp), dtype=torch.uint8, device="cuda")
        call = lambda r: rt.denoise_device(d_rgb.data_ptr(), d_feat.data_ptr(), dp, d_out.data_ptr(), d_ws.data_ptr(), d_row_ids_ptr=r, stream_ptr=sp)
        ms = [timed(torch, stream, lambda: call(None), a.steps, a.warmup) for _ in range(3)]
        rows_ms = timed(torch, stream, lambda: call(d_rows.data_ptr()), a.steps, a.warmup)
        noisy = d_rgb.cpu().numpy().reshape(H, W, 3)
        den = d_out.cpu().numpy().reshape(H, W, 3)
        mse = lambda img: float(np.mean((display(img, spp) - target) ** 2))
        print(json.dumps({"scene": a.scene, "surfaces": a.surfaces, "specular": a.specular, "spp": spp, "n_iter": a.n_iter, "render_ms": round(r_ms, 3), "features_ms": round(f_ms, 3),
                          "denoise_ms": [round(x, 4) for x in ms], "denoise_ms_with_row_list": round(rows_ms, 4),
                          "denoise_vs_render": round(min(ms) / r_ms, 5),
                          "workspace_mb": round(d_ws.numel() / 1e6, 1), "ref_spp": a.ref_spp, "mse_noisy": round(mse(noisy), 6),
                          "mse_denoised": round(mse(den), 6), "mse_ratio": round(mse(den) / mse(noisy), 3),
                          "lib": os.path.basename(F.LIB_PATH)}), flush=True)
        if a.dual:
            dual(a, torch, dev, cam, bg, rows, stream, spp, target, st)


if __name__ == "__main__":
    main()
