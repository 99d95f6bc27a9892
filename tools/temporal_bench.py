#!/usr/bin/env python3
"""Device time of the temporal accumulation (rt_temporal_device) beside the other calls of the same frame, and what it buys
along a camera path.

    python3 tools/temporal_bench.py [--scene final_scene] [--spp 4] [--steps 20] [--warmup 3] [--mse-size 200] [--ref-spp 512]

First one JSON line for the 800x800 default view: ms of rt_render_device (depth 50, spp_chunk 1, median of the calls' own
rt_stats.ms), ms per rt_features_device, rt_denoise_device (5 iterations), rt_denoise_dual_device and rt_temporal_device call
(HIP events around `steps` calls after `warmup`, all on one stream, NULL rows, three windows each; the accumulation also
once with the frame's shuffled row list and once as a first frame). The accumulation gathers from the state of a frame
rendered one camera step to the left.

Then, per scene of --path-scenes, one JSON line for an 8-camera path at --mse-size squared (the step of tests/temporal_ref.py
scaled to the same shift in pixels per frame), each frame two halves of spp / 2 samples from ONE two-frame render and feature
call: the display-value MSE against a --ref-spp render at the last camera of the last frame A + B, of the accumulation of the
whole frames, of rt_denoise_dual on the last frame's halves and of rt_denoise_dual on the two accumulated halves.

--surfaces: the timed calls take RT_FLAG_SURFACES records and RT_TEMPORAL_FAR_MISSES, and every path (default then: final_scene,
cornell_smoke) is run twice, without and with the two flags ("surfaces": false / true in its line).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import raytracer_2022_amd as rt  # noqa: E402
from raytracer_2022_amd import _ffi as F  # noqa: E402
import temporal_ref as R  # noqa: E402
from denoise_dual_ref import add_features  # noqa: E402

ASSETS = os.path.join(ROOT, "assets")
W = H = 800
STEPS = dict(R.PATH_STEP, **{R.HELD_OUT[0]: R.HELD_OUT[1]})


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


def timing(a, torch):
    s = rt.HostScene(a.scene, seed=2022, assets_dir=ASSETS if os.path.isdir(ASSETS) else None)
    dev = rt.DeviceScene(s.desc)
    cam, bg = s.default_view(W / H)
    prev_cam = R.camera_path(cam, STEPS.get(a.scene, 20.0) * R.PATH_W / W, 2)[0]
    rows = np.arange(H, dtype=np.uint32)                   # (buffer order is image order, so the NULL-row windows see the true geometry)
    stream = torch.cuda.Stream()
    sp, n = stream.cuda_stream, H * W
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    new = lambda k: torch.empty(n * k, dtype=torch.float64, device="cuda")
    d_feat, d_rgb, d_out, d_var, d_feat0, d_rgb0 = new(8), new(3), new(3), new(1), new(8), new(3)
    d_state = [new(8), new(8)]
    st = F.rt_stats()
    p = rt.make_params(W, H, a.spp, 50, bg, seed=a.seed, spp_chunk=1)
    # the frame before, from the camera one step to the left, and its state
    dev.render_device(prev_cam, p, d_rows.data_ptr(), H, d_rgb0.data_ptr(), sp, st)
    dev.wait(sp)
    dev.features_device(prev_cam, p, d_rows.data_ptr(), H, d_feat0.data_ptr(), sp, surfaces=a.surfaces)
    tp = rt.temporal_params(W, H, a.spp, far_misses=a.surfaces)
    d_tws = torch.empty(rt.temporal_workspace_bytes(tp), dtype=torch.uint8, device="cuda")
    rt.temporal_device(d_rgb0.data_ptr(), d_feat0.data_ptr(), prev_cam, tp, d_state[0].data_ptr(), d_out.data_ptr(), d_tws.data_ptr(),
                       d_row_ids_ptr=d_rows.data_ptr(), stream_ptr=sp)
    # this frame
    f_ms = timed(torch, stream, lambda: dev.features_device(cam, p, d_rows.data_ptr(), H, d_feat.data_ptr(), sp, surfaces=a.surfaces), a.steps, a.warmup)
    ms = []
    for _ in range(4):
        dev.render_device(cam, p, d_rows.data_ptr(), H, d_rgb.data_ptr(), sp, st)
        dev.wait(sp)
        ms.append(st.ms)
    r_ms = float(np.median(ms[1:]))
    dp = rt.denoise_params(W, H, a.spp)
    dd = rt.denoise_params(W, H, a.spp, sigma_color=rt.DUAL_DEFAULTS["sigma_color"])
    dq = rt.denoise_dual_params()
    d_ws = torch.empty(max(rt.denoise_workspace_bytes(dp), rt.denoise_dual_workspace_bytes(dd)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    single = lambda: rt.denoise_device(d_rgb.data_ptr(), d_feat.data_ptr(), dp, d_out.data_ptr(), d_ws.data_ptr(), stream_ptr=sp)
    both = lambda: rt.denoise_dual_device(d_rgb.data_ptr(), d_rgb0.data_ptr(), d_feat.data_ptr(), d_feat0.data_ptr(), dd, dq, d_out.data_ptr(),
                                          d_ws.data_ptr(), d_out_variance_ptr=d_var.data_ptr(), stream_ptr=sp)
    temporal = lambda r=None, prev=True: rt.temporal_device(d_rgb.data_ptr(), d_feat.data_ptr(), cam, tp, d_state[1].data_ptr(), d_out.data_ptr(),
                                                            d_tws.data_ptr(), d_prev_ptr=d_state[0].data_ptr() if prev else None,
                                                            prev_cam=prev_cam if prev else None, d_row_ids_ptr=r, stream_ptr=sp)
    s_ms = [timed(torch, stream, single, a.steps, a.warmup) for _ in range(3)]
    d_ms = [timed(torch, stream, both, a.steps, a.warmup) for _ in range(3)]
    t_ms = [timed(torch, stream, temporal, a.steps, a.warmup) for _ in range(3)]
    first_ms = timed(torch, stream, lambda: temporal(prev=False), a.steps, a.warmup)
    rows_ms = timed(torch, stream, lambda: temporal(d_rows.data_ptr()), a.steps, a.warmup)
    stream.synchronize()
    state = d_state[1].cpu().numpy().view(F.TEMPORAL_PIXEL_DTYPE)
    print(json.dumps({"scene": a.scene, "surfaces": a.surfaces, "size": "%dx%d" % (W, H), "spp": a.spp, "render_ms": round(r_ms, 3), "features_ms": round(f_ms, 3),
                      "denoise_ms": [round(x, 4) for x in s_ms], "denoise_dual_ms": [round(x, 4) for x in d_ms],
                      "temporal_ms": [round(x, 4) for x in t_ms], "temporal_ms_first_frame": round(first_ms, 4),
                      "temporal_ms_with_row_list": round(rows_ms, 4), "temporal_vs_denoise": round(min(t_ms) / min(s_ms), 3),
                      "temporal_vs_one_atrous_iteration": round(min(t_ms) / (min(s_ms) / dp.n_iter), 3),
                      "temporal_vs_render": round(min(t_ms) / r_ms, 5), "bytes_per_pixel": 88 + 4 * 64 + 88,
                      "gb_per_s": round(n * (88 + 4 * 64 + 88) / (min(t_ms) * 1e6), 1),
                      "pixels_with_history": round(float(np.mean(state["n"] > 1.0)), 3), "lib": os.path.basename(F.LIB_PATH)}), flush=True)
    dev.close()


def path_mse(a, name, surfaces=False):
    S, K, half = a.mse_size, R.PATH_K, a.spp // 2
    s = rt.HostScene(name, seed=2022, assets_dir=ASSETS if os.path.isdir(ASSETS) else None)
    dev = rt.DeviceScene(s.desc)
    cam, bg = s.default_view(1.0)
    cams = R.camera_path(cam, STEPS[name] * R.PATH_W / S, K)
    rows = np.arange(S, dtype=np.uint32)
    rows2 = rt.two_frame_rows(rows, S)
    target = R.display(dev.render(cam, rt.make_params(S, S, a.ref_spp, 50, bg, seed=7, spp_chunk=1), rows), a.ref_spp)
    tp_full, tp_half = rt.temporal_params(S, S, 2 * half, far_misses=surfaces), rt.temporal_params(S, S, half, far_misses=surfaces)
    full = st_a = st_b = acc = acc_a = acc_b = None
    for k in range(K):
        p2 = rt.make_params(S, S, half, 50, bg, seed=a.seed + k, n_frames=2, spp_chunk=1)
        sums, feat = dev.render(cams[k], p2, rows2), dev.features(cams[k], p2, rows2, surfaces=surfaces)
        sa, sb, fa, fb = sums[:S], sums[S:], feat[:S], feat[S:]
        before = cams[k - 1] if k else None
        acc, full = rt.temporal(sa + sb, add_features(fa, fb), cams[k], tp_full, prev=full, prev_cam=before)
        acc_a, st_a = rt.temporal(sa, fa, cams[k], tp_half, prev=st_a, prev_cam=before)
        acc_b, st_b = rt.temporal(sb, fb, cams[k], tp_half, prev=st_b, prev_cam=before)
    dd = rt.denoise_params(S, S, half, sigma_color=rt.DUAL_DEFAULTS["sigma_color"])
    dual_last = rt.denoise_dual(sa, sb, fa, fb, dd)
    dual_acc = rt.denoise_dual(acc_a, acc_b, fa, fb, dd)
    m = lambda img: R.mse(img, 2 * half, target)
    m_last, m_acc, m_dual, m_dual_acc = m(sa + sb), m(acc), m(dual_last), m(dual_acc)
    print(json.dumps({"path": name, "surfaces": surfaces, "size": "%dx%d" % (S, S), "cameras": K, "spp": "2 x %d" % half, "ref_spp": a.ref_spp,
                      "mse_last_frame": round(m_last, 6), "mse_accumulated": round(m_acc, 6), "accumulated_over_last": round(m_acc / m_last, 3),
                      "mse_dual_last_frame": round(m_dual, 6), "mse_dual_accumulated_halves": round(m_dual_acc, 6),
                      "dual_accumulated_over_dual_last": round(m_dual_acc / m_dual, 3),
                      "restarted_in_last_frame": round(float(np.mean(full["n"] == 1.0)), 3), "mean_history_length": round(float(full["n"].mean()), 2)}),
          flush=True)
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="final_scene")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--mse-size", type=int, default=200)
    ap.add_argument("--ref-spp", type=int, default=512)
    ap.add_argument("--path-scenes", default=None)
    ap.add_argument("--surfaces", action="store_true", help="RT_FLAG_SURFACES records and RT_TEMPORAL_FAR_MISSES (see above)")
    a = ap.parse_args()
    if a.path_scenes is None:
        a.path_scenes = "final_scene,cornell_smoke" if a.surfaces else "cornell_box,final_scene"
    import torch
    torch.zeros(1, device="cuda")
    timing(a, torch)
    for name in [x for x in a.path_scenes.split(",") if x]:
        path_mse(a, name)
        if a.surfaces:
            path_mse(a, name, surfaces=True)


if __name__ == "__main__":
    main()
