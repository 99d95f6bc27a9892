"""The temporal accumulation (rt_temporal*) once more in numpy, and the CPU side of its evaluation. No GPU is needed:
tests/test_temporal.py compares the library with `restate` bit for bit, tests/test_temporal_ref.py holds `restate` to a plain
per-pixel loop and to closed forms, tools/temporal_grid.py chooses the Python defaults with it on the oracle's renders.

`restate` is include/rt2022.h's definition: the four taps one after the other in the header's order, the pixels of a tap
vectorised, a tap that does not count through np.where. numpy's element-wise + - * / on float64 are the IEEE operations and
nothing is fused, so the kernel (built with -ffp-contract=off) must give the same doubles."""
import math

import numpy as np

from raytracer_2022_amd import _ffi as F

from denoise_ref import display
from features_ref import oracle_features

# The camera paths of the end-to-end tests and of the grid: scene -> the step between two cameras, in world units along the
# default view's u axis (about 1.5 pixels of image shift per frame at 48 x 48 for what the view looks at). Camera K-1 is the
# scene's default view; the cameras before it lie on a line to its left. The last scene the grid never sees.
PATH_STEP = {"cornell_box": 20.0, "random_scene": 0.15, "final_scene": 20.0}
HELD_OUT = ("cornell_smoke", 20.0)
PATH_W, PATH_H, PATH_K, PATH_SPP, SEED, REF_SPP, REF_SEED = 48, 48, 8, 4, 2022, 256, 7


def vec(v):
    return np.array(v[:], dtype=np.float64)


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def restate(sums, feat, cam, p, prev=None, prev_cam=None, rows=None, geometry=False):
    """The definition in numpy. Sums (H, W, 3) and FEATURE_DTYPE records (H, W) in buffer order, the previous state (H, W) in
    image order or None -> (accumulated sums (H, W, 3), buffer order; state (H, W) of TEMPORAL_PIXEL_DTYPE, image order)
    [, {fx, fy, ze, history, sw, accepted}: the reprojection of every pixel, image order]."""
    H, W = p.height, p.width
    s = np.asarray(sums, dtype=np.float64).reshape(H, W, 3)
    f = np.asarray(feat).reshape(H, W)
    if rows is not None:                                   # buffer row i is image row rows[i]
        inv = np.empty(H, dtype=np.int64)
        inv[np.asarray(rows, dtype=np.int64)] = np.arange(H)
        s, f = s[inv], f[inv]
    one, half, zero = np.float64(1.0), np.float64(0.5), np.float64(0.0)
    geo = None
    with np.errstate(all="ignore"):
        sp = np.float64(p.spp)
        c = np.where(np.isnan(s), zero, s) / sp
        a = f["albedo"] / sp
        floor = np.float64(p.albedo_floor)
        m = np.ones_like(a) if p.flags & F.RT_TEMPORAL_NO_DEMODULATE else np.where(a > floor, a, floor)
        e = c / m
        hits = f["hits"]
        covered = hits > zero
        zb = np.where(covered, f["depth"] / hits, zero)
        nb = np.where(covered[..., None], f["normal"] / hits[..., None], zero)
        e_out, n_out = e, np.ones((H, W))
        if prev is not None:
            pv = np.asarray(prev).reshape(H, W)
            ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
            wm1, hm1 = np.float64(W - 1), np.float64(H - 1)
            sc, tc = (xs + half) / wm1, (ys + half) / hm1
            o, llc, hor, ver = vec(cam.origin), vec(cam.lower_left_corner), vec(cam.horizontal), vec(cam.vertical)
            po, pllc, phor, pver = vec(prev_cam.origin), vec(prev_cam.lower_left_corner), vec(prev_cam.horizontal), vec(prev_cam.vertical)
            G = (llc + sc[..., None] * hor) + tc[..., None] * ver
            P = o + zb[..., None] * (G - o)
            cv = -(P - po)
            r = po - pllc
            bc, rc, br = cross(pver, cv), cross(r, cv), cross(pver, r)
            det = dot(phor, bc)
            s1, t1, lam = dot(r, bc) / det, dot(phor, rc) / det, dot(phor, br) / det
            fx, fy = s1 * wm1 - half, t1 * hm1 - half
            hist = covered & (lam > zero) & (fx >= -one) & (fx < np.float64(W)) & (fy >= -one) & (fy < np.float64(H))
            ze = one / lam
            fxs, fys = np.where(hist, fx, zero), np.where(hist, fy, zero)      # (integers only after the range test)
            xf, yf = np.floor(fxs), np.floor(fys)
            wx, wy = fxs - xf, fys - yf
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            bw = [(one - wx) * (one - wy), wx * (one - wy), (one - wx) * wy, wx * wy]
            sw, sn, se = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W, 3))
            tol_d, tol_n = np.float64(p.tol_depth), np.float64(p.tol_normal)
            for t in range(4):
                qx, qy = x0 + (t & 1), y0 + (t >> 1)
                ok = hist & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                q = pv[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                pd = q["depth"]
                ok = ok & (pd > zero)
                if not math.isinf(p.tol_depth):
                    ok = ok & (np.abs(pd - ze) <= tol_d * ze)
                if not math.isinf(p.tol_normal):
                    d = nb - q["normal"]
                    ok = ok & ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= tol_n)
                sw = np.where(ok, sw + bw[t], sw)
                se = np.where(ok[..., None], se + bw[t][..., None] * q["e"], se)
                sn = np.where(ok, sn + bw[t] * q["n"], sn)
            acc = hist & (sw >= np.float64(p.w_min))
            nh = sn / sw
            tt = nh + one
            no = np.where(tt < np.float64(p.n_max), tt, np.float64(p.n_max))
            eh = se / sw[..., None]
            eo = eh + (e - eh) / no[..., None]
            e_out, n_out = np.where(acc[..., None], eo, e), np.where(acc, no, one)
            geo = {"fx": fx, "fy": fy, "ze": ze, "history": hist, "sw": sw, "accepted": acc, "eh": eh}
        state = np.zeros((H, W), dtype=F.TEMPORAL_PIXEL_DTYPE)
        state["e"], state["n"], state["depth"], state["normal"] = e_out, n_out, zb, nb
        out = (e_out * m) * sp
    if rows is not None:
        out = out[np.asarray(rows, dtype=np.int64)]
    return (out, state, geo) if geometry else (out, state)


def mse(sums, spp, target):
    return float(np.mean((display(sums, spp) - target) ** 2))


def shifted_camera(cam, d):
    """`cam` moved by the vector d without turning: origin and lower_left_corner move together."""
    out = F.rt_camera.from_buffer_copy(cam)
    for k in range(3):
        out.origin[k] = cam.origin[k] + float(d[k])
        out.lower_left_corner[k] = cam.lower_left_corner[k] + float(d[k])
    return out


def camera_path(cam, step, K=PATH_K):
    """K cameras on a line along cam's u axis, `step` apart, the last one cam itself."""
    u = vec(cam.u)
    return [shifted_camera(cam, u * (step * (k - (K - 1)))) for k in range(K)]


def frame_params(rt, W, H, spp, bg, k):
    """The render parameters of frame k of a path: a seed of its own, so that the frames' samples are independent."""
    return rt.make_params(W, H, spp, 50, bg, seed=SEED + k)


def oracle_path(rt, O, name, step, W=PATH_W, H=PATH_H, K=PATH_K, spp=PATH_SPP, threads=4, rows=None):
    """The oracle's frames along a scene's path: (cameras, [sums (H, W, 3)], [FEATURE_DTYPE records (H, W)]), in the order of
    `rows` (None: image order)."""
    s = rt.HostScene(name, seed=2022)
    cam, bg = s.default_view(W / H)
    cams = camera_path(cam, step, K)
    rows = np.arange(H, dtype=np.uint32) if rows is None else rows
    sums, feats = [], []
    for k, c in enumerate(cams):
        params = frame_params(rt, W, H, spp, bg, k)
        sums.append(O.render_cpu(s.desc, c, params, rows, n_threads=threads))
        feats.append(oracle_features(O, s.desc, c, params, rows)[0].reshape(H, W))
    return s, bg, cams, sums, feats


def oracle_target(rt, O, s, bg, cam, W=PATH_W, H=PATH_H, threads=4):
    """The display values of a REF_SPP render at `cam`, image order."""
    ref = O.render_cpu(s.desc, cam, rt.make_params(W, H, REF_SPP, 50, bg, seed=REF_SEED), np.arange(H, dtype=np.uint32), n_threads=threads)
    return display(ref, REF_SPP)


def accumulate(sums, feats, cams, p, rows=None):
    """The restatement along a path: frame 0 with no history, then each frame on the state before it -> (the last frame's
    accumulated sums, its state, the fraction of restarted pixels per frame after the first)."""
    state, out, restarts = None, None, []
    for k in range(len(cams)):
        out, state = restate(sums[k], feats[k], cams[k], p, state, cams[k - 1] if k else None, rows)
        if k:
            restarts.append(float(np.mean(state["n"] == 1.0)))
    return out, state, restarts
