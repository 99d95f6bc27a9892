#!/usr/bin/env python3
"""What per-pixel adaptive sampling (rt.render_adaptive) buys at an equal total sample count, and what its stages cost.

    python3 tools/adaptive_bench.py [--scenes cornell_box,final_scene] [--spp 4] [--total-spp 32] [--rounds 2] [--max-units 4] [--ref-spp 512]
                                    [--guides initial|all|both]

Per scene, one JSON line for the 800x800 default view (the size of tools/denoise_bench.py). MSE of the display values
sqrt(clip(c, 0, 0.999)) against a --ref-spp render at another seed, all at --total-spp samples per pixel on average:
uniform sampling (two frames of total-spp / 2, the halves a dual denoise needs), raw and after rt_denoise_dual; render_adaptive,
raw and after rt_denoise_dual on its two resolved halves. --guides initial: render_adaptive(guides="initial"), the final filter
guided by the features of the INITIAL frames (2 x --spp samples, rescaled to the halves' divisor), while the uniform frame's
guides come from all its samples. --guides all: render_adaptive(guides="all"), feature records carried through the accumulators
by rt_features_pixels_device, the final filter guided by resolve_features(feat_acc, acc_n, half) — like for like with the
uniform frame. both (the default) runs the two and prints both sets of figures. The share of pixels that got extra units. Device
ms of the plan calls, the merges and the pixel render of every round (HIP events), beside rt_render_device of whole rows
holding at least as many paths at the same spp; with all guides, the ms of every round's rt_features_pixels_device beside
rt_features_device over whole rows holding at least as many pixel-samples at the same spp — both as torch events round a call
without stats, so both are the plain kernel instance with the id check's synchronisation inside the span. The numbers are printed as they
come: nothing here is tuned, and a loss is a result."""
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


def display(sums, spp):
    return np.sqrt(np.clip(np.where(np.isnan(sums), 0.0, sums) / spp, 0.0, 0.999))


def dual_denoise(torch, half_a, half_b, feat, half_spp, n_iter):
    """rt_denoise_dual_device at the package's defaults on two halves of half_spp samples each → sums of 2 * half_spp samples."""
    pd = rt.denoise_params(W, H, half_spp, n_iter=n_iter, sigma_color=rt.DUAL_DEFAULTS["sigma_color"])
    ws = torch.empty(rt.denoise_dual_workspace_bytes(pd), dtype=torch.uint8, device="cuda")
    out = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
    rt.denoise_dual_device(half_a.data_ptr(), half_b.data_ptr(), feat[0].data_ptr(), feat[1].data_ptr(), pd, rt.denoise_dual_params(),
                           out.data_ptr(), ws.data_ptr(), stream_ptr=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_box,final_scene")
    ap.add_argument("--spp", type=int, default=4, help="the unit: samples of one half in the initial frames and in every extra unit")
    ap.add_argument("--total-spp", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-units", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=512)
    ap.add_argument("--n-iter", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--guides", choices=["initial", "all", "both"], default="both",
                    help="guides of the adaptive rounds and of the final dual denoise: the initial frames', every sample's, or one run of each")
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    n = W * H
    rows = np.arange(H, dtype=np.uint32)
    d_rows2 = torch.from_numpy(rt.two_frame_rows(rows, H).view(np.int32)).cuda()
    for scene in a.scenes.split(","):
        s = rt.HostScene(scene, seed=2022, assets_dir=ASSETS if os.path.isdir(ASSETS) else None)
        dev = rt.DeviceScene(s.desc)
        cam, bg = s.default_view(W / H)
        target = display(dev.render(cam, rt.make_params(W, H, a.ref_spp, 50, bg, seed=a.seed + 77, spp_chunk=1), rows), a.ref_spp)
        mse = lambda sums, spp: float(np.mean((display(sums, spp) - target) ** 2))
        # uniform: two frames of total_spp / 2 samples
        half = a.total_spp // 2
        pu = rt.make_params(W, H, half, 50, bg, seed=a.seed, n_frames=2, spp_chunk=1)
        d_u = torch.empty((2, H, W, 3), dtype=torch.float64, device="cuda")
        d_fu = torch.empty((2, n, 8), dtype=torch.float64, device="cuda")
        st = F.rt_stats()
        dev.render_device(cam, pu, d_rows2.data_ptr(), 2 * H, d_u.data_ptr(), sp, st)
        dev.wait(sp)                                                   # (fills st)
        uniform_ms = st.ms
        dev.features_device(cam, pu, d_rows2.data_ptr(), 2 * H, d_fu.data_ptr(), sp)
        torch.cuda.synchronize()
        m_uniform = mse((d_u[0] + d_u[1]).cpu().numpy(), 2 * half)
        m_uniform_dual = mse(dual_denoise(torch, d_u[0], d_u[1], d_fu, half, a.n_iter), 2 * half)
        rnd = lambda x: round(float(x), 4)
        line = {"scene": scene, "size": "%dx%d" % (W, H), "unit_spp": a.spp, "total_spp": a.total_spp, "rounds": a.rounds,
                "max_units": a.max_units, "ref_spp": a.ref_spp, "guides": a.guides,
                "mse_uniform": round(m_uniform, 6), "mse_uniform_dual": round(m_uniform_dual, 6)}
        p = rt.make_params(W, H, a.spp, 50, bg, seed=a.seed, spp_chunk=1)
        halves = torch.empty((2, H, W, 3), dtype=torch.float64, device="cuda")
        for guides in (("initial", "all") if a.guides == "both" else (a.guides,)):
            # adaptive, once to warm the pool up and once measured
            rt.render_adaptive(dev, cam, p, a.total_spp, rounds=a.rounds, max_units=a.max_units, guides=guides)
            out, counts, log, state = rt.render_adaptive(dev, cam, p, a.total_spp, rounds=a.rounds, max_units=a.max_units, profile=True,
                                                         want_state=True, guides=guides)
            m_adaptive = mse(out.cpu().numpy(), a.total_spp)
            for h in range(2):
                rt.adaptive_resolve_device(state["acc"][h].data_ptr(), state["acc_n"][h].data_ptr(), n, half, halves[h].data_ptr(), sp)
            if guides == "all":                                        # every sample's records, as sums of `half` samples
                feat = torch.empty_like(state["feat_acc"])
                for h in range(2):
                    rt.adaptive_resolve_features_device(state["feat_acc"][h].data_ptr(), state["acc_n"][h].data_ptr(), n, half, feat[h].data_ptr(), sp)
            else:                                                      # the initial frames': sums of a.spp samples, rescaled to the halves' divisor
                feat = state["feat"] * (float(half) / float(a.spp))
            m_adaptive_dual = mse(dual_denoise(torch, halves[0], halves[1], feat, half, a.n_iter), 2 * half)
            c = counts.cpu().numpy()
            # rt_render_device of whole rows holding at least the paths of the pixel renders, at the unit's spp
            paths = sum(r["samples"] for r in log)
            n_rows = max(1, -(-paths // (W * a.spp)))
            d_same = torch.empty((n_rows, W, 3), dtype=torch.float64, device="cuda")
            d_rows_same = torch.arange(n_rows, dtype=torch.int32, device="cuda")      # whole frames, then part of one
            pr = rt.make_params(W, H, a.spp, 50, bg, seed=a.seed + 1, n_frames=-(-n_rows // H), spp_chunk=1)
            ms = []
            for _ in range(3):
                dev.render_device(cam, pr, d_rows_same.data_ptr(), n_rows, d_same.data_ptr(), sp, st)
                dev.wait(sp)
                ms.append(st.ms)
            tag = "_all_guides" if guides == "all" else ""
            line.update({"samples_spent_per_pixel" + tag: rnd(c.mean()),
                         "mse_adaptive" + tag: round(m_adaptive, 6), "mse_adaptive_dual" + tag: round(m_adaptive_dual, 6),
                         "adaptive%s_over_uniform" % tag: round(m_adaptive / m_uniform, 3),
                         "adaptive_dual%s_over_uniform_dual" % tag: round(m_adaptive_dual / m_uniform_dual, 3),
                         "pixels_with_extra_units" + tag: rnd(float(np.mean(c > 2 * a.spp))), "max_samples_of_a_pixel" + tag: int(c.max()),
                         "rounds_log" + tag: [{k: (rnd(v) if isinstance(v, float) else v) for k, v in r.items()} for r in log],
                         "plan_ms" + tag: rnd(sum(r.get("plan_ms", 0.0) for r in log)), "merge_ms" + tag: rnd(sum(r.get("merge_ms", 0.0) for r in log)),
                         "render_pixels_ms" + tag: rnd(sum(r.get("render_pixels_ms", 0.0) for r in log)), "render_pixels_paths" + tag: int(paths),
                         "render_rows_same_paths_ms" + tag: rnd(np.median(ms)), "render_rows_paths" + tag: int(n_rows * W * a.spp)})
            if guides == "all":
                # rt_features_device of whole rows holding at least the pixel-samples of the feature calls, at the unit's spp, timed as
                # render_adaptive times the pixel-list call: torch events round a call without stats — the plain kernel instance,
                # with the range check of the device ids and its synchronisation inside the span on both sides
                d_fsame = torch.empty((n_rows * W, 8), dtype=torch.float64, device="cuda")
                fms = []
                for _ in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    dev.features_device(cam, pr, d_rows_same.data_ptr(), n_rows, d_fsame.data_ptr(), sp)
                    e1.record()
                    e1.synchronize()
                    fms.append(e0.elapsed_time(e1))
                line.update({"features_pixels_ms": [rnd(r.get("features_pixels_ms", 0.0)) for r in log],
                             "features_pixels_samples": int(paths), "merge_features_ms": rnd(sum(r.get("merge_features_ms", 0.0) for r in log)),
                             "features_rows_same_samples_ms": rnd(np.median(fms)), "features_rows_samples": int(n_rows * W * a.spp)})
        line.update({"uniform_render_2_frames_ms": rnd(uniform_ms), "lib": os.path.basename(F.LIB_PATH)})
        print(json.dumps(line), flush=True)
        dev.close()


if __name__ == "__main__":
    main()
