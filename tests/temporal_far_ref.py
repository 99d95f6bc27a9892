"""rt_temporal* with RT_TEMPORAL_FAR_MISSES once more in numpy: temporal_ref.restate's definition with the header's far-miss
clause added. No GPU is needed. Without the flag `restate` here IS temporal_ref.restate's arithmetic, operation for operation
(tests/test_temporal_far_ref.py holds the two to equal bits on random inputs, and this one to a plain per-pixel loop);
tests/test_temporal_far.py compares the library with it bit for bit.

The clause: a pixel that is not covered takes the pixel centre's direction G - o in place of P - o' (a point at infinity), the
same Cramer solve in the same order, no ze; history needs lam > 0 and the same range tests; a tap counts if it is inside the
image and prev(q).depth == 0.0, with no depth and no normal test. Covered pixels are untouched."""
import math

import numpy as np

from raytracer_2022_amd import _ffi as F

from temporal_ref import cross, dot, vec


def restate(sums, feat, cam, p, prev=None, prev_cam=None, rows=None, geometry=False):
    """temporal_ref.restate's arguments and results; p.flags may hold RT_TEMPORAL_FAR_MISSES."""
    H, W = p.height, p.width
    far = bool(p.flags & F.RT_TEMPORAL_FAR_MISSES)
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
            cv = np.where(covered[..., None], -(P - po), -(G - o))             # D = P - o', or the direction G - o of a far miss
            r = po - pllc
            bc, rc, br = cross(pver, cv), cross(r, cv), cross(pver, r)
            det = dot(phor, bc)
            s1, t1, lam = dot(r, bc) / det, dot(phor, rc) / det, dot(phor, br) / det
            fx, fy = s1 * wm1 - half, t1 * hm1 - half
            hist = (covered | far) & (lam > zero) & (fx >= -one) & (fx < np.float64(W)) & (fy >= -one) & (fy < np.float64(H))
            ze = one / lam                                                      # (used by covered pixels only)
            fxs, fys = np.where(hist, fx, zero), np.where(hist, fy, zero)      # (integers only after the range test)
            xf, yf = np.floor(fxs), np.floor(fys)
            wx, wy = fxs - xf, fys - yf
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            bw = [(one - wx) * (one - wy), wx * (one - wy), (one - wx) * wy, wx * wy]
            sw, sn, se = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W, 3))
            tol_d, tol_n = np.float64(p.tol_depth), np.float64(p.tol_normal)
            for t in range(4):
                qx, qy = x0 + (t & 1), y0 + (t >> 1)
                inside = hist & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                q = pv[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                pd = q["depth"]
                ok = inside & (pd > zero)
                if not math.isinf(p.tol_depth):
                    ok = ok & (np.abs(pd - ze) <= tol_d * ze)
                if not math.isinf(p.tol_normal):
                    d = nb - q["normal"]
                    ok = ok & ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= tol_n)
                ok = np.where(covered, ok, inside & (pd == zero))               # a far miss: the previous state's uncovered pixels, untested
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


def accumulate(sums, feats, cams, p, rows=None):
    """temporal_ref.accumulate with this restatement: (the last frame's accumulated sums, its state, the restart share per frame)."""
    state, out, restarts = None, None, []
    for k in range(len(cams)):
        out, state = restate(sums[k], feats[k], cams[k], p, state, cams[k - 1] if k else None, rows)
        if k:
            restarts.append(float(np.mean(state["n"] == 1.0)))
    return out, state, restarts
