"""The CPU side of RT_FLAG_SURFACES and RT_TEMPORAL_FAR_MISSES: the constants, the far-miss restatement
(tests/temporal_far_ref.py) held to temporal_ref.restate, to a plain per-pixel loop and to closed forms, the oracle's feature
composition on the looked-through copy of a scene (tests/surface_ref.py), and what the surface records are for: a smaller
error of the accumulated frame on cornell_smoke's path. No GPU."""
import math
import os
import re

import numpy as np
import pytest

from raytracer_2022_amd import _ffi as F

import surface_ref as S
import temporal_cases as T
import temporal_far_ref as FR
import temporal_ref as R
from compare import assert_same_bits
from features_ref import oracle_features
from temporal_far_cases import far_cameras, more_misses, turned

f64 = np.float64
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt2022.h")
MEDIA_FREE = ["cornell_box", "earth", "random_scene", "simple_light", "two_perlin_spheres", "two_spheres", "wwscene"]


# ---- constants --------------------------------------------------------------------------------------------------------------
def test_constants_match_the_header():
    text = open(HEADER).read()
    defines = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (RT_\w+) (0x[0-9a-fA-F]+)u", text)}
    assert defines["RT_FLAG_SURFACES"] == 0x10 == F.RT_FLAG_SURFACES
    assert defines["RT_TEMPORAL_FAR_MISSES"] == 0x4 == F.RT_TEMPORAL_FAR_MISSES
    assert defines["RT_TEMPORAL_NO_DEMODULATE"] == 0x1 == F.RT_TEMPORAL_NO_DEMODULATE
    flags = [defines[k] for k in ("RT_FLAG_COUNTERS", "RT_FLAG_KERNEL_TIMES", "RT_FLAG_ASYNC", "RT_FLAG_ANY_HIT", "RT_FLAG_SURFACES")]
    assert sorted(flags) == [1, 2, 4, 8, 16]                 # one bit each, none shared
    assert "#define RT2022_ABI_VERSION 3" in text and F.RT2022_ABI_VERSION == 3


def test_temporal_params_far_misses(rt):
    assert rt.temporal_params(5, 3, 4).flags == 0
    assert rt.temporal_params(5, 3, 4, far_misses=True).flags == F.RT_TEMPORAL_FAR_MISSES
    assert rt.temporal_params(5, 3, 4, demodulate=False, far_misses=True).flags == F.RT_TEMPORAL_FAR_MISSES | F.RT_TEMPORAL_NO_DEMODULATE
    assert rt.temporal_params(5, 3, 4, demodulate=False).flags == F.RT_TEMPORAL_NO_DEMODULATE


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def loop_restate(sums, feat, cam, p, prev, prev_cam):
    """include/rt2022.h's definition with the far-miss clause, one pixel after the other with numpy scalars: image order in,
    (sums, state) out. (Written from the header, not from temporal_far_ref.)"""
    H, W = p.height, p.width
    far = bool(p.flags & F.RT_TEMPORAL_FAR_MISSES)
    out = np.zeros((H, W, 3))
    state = np.zeros((H, W), dtype=F.TEMPORAL_PIXEL_DTYPE)
    sp, floor, one = f64(p.spp), f64(p.albedo_floor), f64(1.0)
    cr = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    dt = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
    o, llc, hor, ver = ([f64(x) for x in v[:]] for v in (cam.origin, cam.lower_left_corner, cam.horizontal, cam.vertical))
    if prev is not None:
        po, pllc, phor, pver = ([f64(x) for x in v[:]] for v in (prev_cam.origin, prev_cam.lower_left_corner, prev_cam.horizontal, prev_cam.vertical))
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                S_, Fr = sums[y, x], feat[y, x]
                c = [(f64(0.0) if np.isnan(S_[j]) else f64(S_[j])) / sp for j in range(3)]
                a = [f64(Fr["albedo"][j]) / sp for j in range(3)]
                m = [one if p.flags & F.RT_TEMPORAL_NO_DEMODULATE else (a[j] if a[j] > floor else floor) for j in range(3)]
                e = [c[j] / m[j] for j in range(3)]
                hits = f64(Fr["hits"])
                covered = bool(hits > 0)
                zb = f64(Fr["depth"]) / hits if covered else f64(0.0)
                nb = [f64(Fr["normal"][j]) / hits if covered else f64(0.0) for j in range(3)]
                e_out, n_out = e, one
                if prev is not None and (covered or far):
                    sc, tc = (f64(x) + f64(0.5)) / f64(W - 1), (f64(y) + f64(0.5)) / f64(H - 1)
                    G = [(llc[k] + sc * hor[k]) + tc * ver[k] for k in range(3)]
                    if covered:
                        P = [o[k] + zb * (G[k] - o[k]) for k in range(3)]
                        D = [P[k] - po[k] for k in range(3)]
                    else:
                        D = [G[k] - o[k] for k in range(3)]
                    cv = [-D[k] for k in range(3)]
                    r = [po[k] - pllc[k] for k in range(3)]
                    bc, rc, br = cr(pver, cv), cr(r, cv), cr(pver, r)
                    det = dt(phor, bc)
                    s1, t1, lam = dt(r, bc) / det, dt(phor, rc) / det, dt(phor, br) / det
                    fx, fy = s1 * f64(W - 1) - f64(0.5), t1 * f64(H - 1) - f64(0.5)
                    if lam > 0 and math.isfinite(fx) and math.isfinite(fy) and -1.0 <= fx < W and -1.0 <= fy < H:
                        x0, y0 = math.floor(fx), math.floor(fy)
                        wx, wy = fx - f64(x0), fy - f64(y0)
                        bw = [(one - wx) * (one - wy), wx * (one - wy), (one - wx) * wy, wx * wy]
                        sw, sn, se = f64(0.0), f64(0.0), [f64(0.0)] * 3
                        for t, (qx, qy) in enumerate(((x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1))):
                            if not (0 <= qx < W and 0 <= qy < H):
                                continue
                            q = prev[qy, qx]
                            pd = f64(q["depth"])
                            if covered:
                                ze = one / lam
                                if not pd > 0:
                                    continue
                                if not math.isinf(p.tol_depth) and not abs(pd - ze) <= f64(p.tol_depth) * ze:
                                    continue
                                d = [nb[k] - f64(q["normal"][k]) for k in range(3)]
                                if not math.isinf(p.tol_normal) and not (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= f64(p.tol_normal):
                                    continue
                            elif not pd == 0.0:
                                continue
                            sw = sw + bw[t]
                            se = [se[j] + bw[t] * f64(q["e"][j]) for j in range(3)]
                            sn = sn + bw[t] * f64(q["n"])
                        if sw >= p.w_min:
                            nh = sn / sw
                            n_out = nh + one if nh + one < p.n_max else f64(p.n_max)
                            eh = [se[j] / sw for j in range(3)]
                            e_out = [eh[j] + (e[j] - eh[j]) / n_out for j in range(3)]
                state[y, x] = (e_out, n_out, zb, nb)
                out[y, x] = [(e_out[j] * m[j]) * sp for j in range(3)]
    return out, state


@pytest.mark.parametrize("W, H", [(7, 5), (1, 6)])
def test_far_restatement_equals_the_per_pixel_loop(rt, W, H):
    """Hostile records with many misses, a poisoned history (NaN, +-inf, zero and negative depths), every camera pair, both flag
    combinations and the tolerance switches."""
    accepted_far = 0
    for seed, (name, (cam, prev_cam)) in enumerate(far_cameras(rt, W, H).items()):
        s0, f0 = T.frame(W, H, seed=10 + seed)
        s1, f1 = T.frame(W, H, seed=20 + seed)
        f0, f1 = more_misses(f0, seed), more_misses(f1, 50 + seed)
        for kw in ({}, {"tol_depth": math.inf, "tol_normal": math.inf, "w_min": 1.0}, {"n_max": 1.0}, {"demodulate": False}, {"w_min": 0.01}):
            for far in (True, False):
                p = rt.temporal_params(W, H, 4, far_misses=far, **kw)
                out0, st0 = FR.restate(s0, f0, prev_cam, p)
                ref0 = loop_restate(s0, f0, prev_cam, p, None, None)
                assert_same_bits(out0, ref0[0], (name, kw, far, "first frame"))
                assert_same_bits(st0, ref0[1], (name, kw, far, "first frame, state"))
                hist = T.poisoned(st0, seed)
                hist["depth"][np.random.default_rng(seed).random((H, W)) < 0.1] = -np.inf
                for history in (st0, hist):
                    out1, st1, geo = FR.restate(s1, f1, cam, p, history, prev_cam, geometry=True)
                    ref1 = loop_restate(s1, f1, cam, p, history, prev_cam)
                    assert_same_bits(out1, ref1[0], (name, kw, far))
                    assert_same_bits(st1, ref1[1], (name, kw, far, "state"))
                    miss = ~(f1["hits"] > 0)
                    if far:
                        accepted_far += int(geo["accepted"][miss].sum())
                        assert (st1["depth"][miss] == 0.0).all() and (st1["normal"][miss] == 0.0).all()
                    else:
                        assert not geo["accepted"][miss].any()
                    if W == 1:
                        assert not geo["accepted"].any() and (st1["n"] == 1.0).all()      # sc is infinite: every pixel restarts
    assert accepted_far > 0 or W == 1, "no uncovered pixel ever took its history"


@pytest.mark.parametrize("W, H", [(7, 5), (23, 11), (1, 6), (6, 1)])
def test_without_the_flag_it_is_temporal_ref(rt, W, H):
    for seed, (name, (cam, prev_cam)) in enumerate(far_cameras(rt, W, H).items()):
        s0, f0 = T.frame(W, H, seed=30 + seed)
        s1, f1 = T.frame(W, H, seed=40 + seed)
        f1 = more_misses(f1, seed)
        for kw in ({}, {"tol_depth": math.inf}, {"tol_normal": math.inf, "demodulate": False}, {"n_max": 1.0, "w_min": 1.0}):
            p = rt.temporal_params(W, H, 4, **kw)
            a0, b0 = FR.restate(s0, f0, prev_cam, p), R.restate(s0, f0, prev_cam, p)
            assert_same_bits(a0[0], b0[0]), assert_same_bits(a0[1], b0[1])
            rows = np.random.default_rng(seed).permutation(H).astype(np.uint32)
            for history in (b0[1], T.poisoned(b0[1], seed)):
                for r in (None, rows):
                    a1 = FR.restate(s1, f1, cam, p, history, prev_cam, rows=r, geometry=True)
                    b1 = R.restate(s1, f1, cam, p, history, prev_cam, rows=r, geometry=True)
                    assert_same_bits(a1[0], b1[0], (name, kw)), assert_same_bits(a1[1], b1[1], (name, kw, "state"))
                    assert np.array_equal(a1[2]["accepted"], b1[2]["accepted"])


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def frames_with_a_fixed_hole(W, H, K, hole, seed):
    """K benign frames whose pixels under `hole` are all-zero miss records in every frame."""
    out = []
    for k in range(K):
        s, f = T.frame(W, H, seed=seed + k, hostile=False)
        f.view(np.float64).reshape(H, W, 8)[hole] = 0.0
        out.append((s, f))
    return out


def test_still_camera_gives_the_running_mean_on_uncovered_pixels(rt):
    W, H, K = 23, 11, 8
    cam = T.camera(rt, W, H)
    hole = np.random.default_rng(3).random((H, W)) < 0.4
    p = rt.temporal_params(W, H, 4, n_max=1e9, far_misses=True)
    state, es = None, []
    for k, (s, f) in enumerate(frames_with_a_fixed_hole(W, H, K, hole, 60)):
        es.append(FR.restate(s, f, cam, p)[1]["e"])
        _, state = FR.restate(s, f, cam, p, state, cam if k else None)
    assert hole.sum() > 50
    assert np.abs(state["n"][hole] - K).max() <= 1e-9
    mean = np.mean(es, axis=0)
    assert np.abs(state["e"][hole] - mean[hole]).max() <= 1e-9 * np.abs(mean).max()
    assert (state["depth"][hole] == 0.0).all()
    # ... and without the flag the same pixels restart on every frame
    _, plain = R.restate(*frames_with_a_fixed_hole(W, H, K, hole, 60)[-1], cam, rt.temporal_params(W, H, 4, n_max=1e9), state, cam)
    assert (plain["n"][hole] == 1.0).all()


def test_sideways_move_leaves_uncovered_pixels_where_they_are(rt):
    """A translation moves no point at infinity: r = o' - llc' is what it was, c = -(G - o) does not know the origin, so
    s' = sc, t' = tc to rounding: shift 0, however far the camera went."""
    W, H = 23, 11
    prev_cam = T.camera(rt, W, H)
    cam = R.shifted_camera(prev_cam, R.vec(prev_cam.u) * 37.5 + R.vec(prev_cam.v) * 2.0)
    hole = np.zeros((H, W), dtype=bool)
    hole[:, 5:17] = True
    (s0, f0), (s1, f1) = frames_with_a_fixed_hole(W, H, 2, hole, 70)
    p = rt.temporal_params(W, H, 4, far_misses=True)
    _, st0 = FR.restate(s0, f0, prev_cam, p)
    _, st1, geo = FR.restate(s1, f1, cam, p, st0, prev_cam, geometry=True)
    ys, xs = np.nonzero(hole)
    assert np.abs(geo["fx"][hole] - xs).max() <= 1e-9 and np.abs(geo["fy"][hole] - ys).max() <= 1e-9
    inner = np.zeros_like(hole)
    inner[:, 6:16] = True                                   # (a rounding below the integer reads the left neighbour at weight 1e-16)
    assert (np.abs(st1["n"][inner] - 2.0) <= 1e-9).all()
    e1 = FR.restate(s1, f1, cam, p)[1]["e"]
    want = st0["e"] + (e1 - st0["e"]) / 2.0
    assert np.abs(st1["e"][inner] - want[inner]).max() <= 1e-9 * np.abs(want).max()


def test_pan_shifts_uncovered_columns_by_the_tangent_rule(rt):
    """The camera turns about its v axis by theta; the previous camera is the unturned one. Derivation, from the cameras' own
    vectors: T.camera has focus 1, so llc - o = -hor/2 - ver/2 - w and a pixel centre's direction is
        d = G - o = a u + b v - w,   a = (sc - 1/2) |hor|,  b = (tc - 1/2) |ver|.
    The previous camera's axes are (u', v, w') with u = cos(theta) u' + sin(theta) w' and w = -sin(theta) u' + cos(theta) w'
    (asserted below on the cameras' u and w), so
        d = (a cos + sin) u' + b v - (cos - a sin) w'.
    The previous camera sees the direction a' u' + b' v - w' at s' = 1/2 + a' / |hor|, t' = 1/2 + b' / |ver|, and d scaled to
    w' component -1 is a' = (a cos + sin) / (cos - a sin) = tan(phi + theta) with a = tan(phi), b' = b / (cos - a sin). Hence
        fx = (1/2 + a' / |hor|) (W - 1) - 1/2,  fy = (1/2 + b' / |ver|) (H - 1) - 1/2,
    visible in the previous camera iff cos - a sin > 0. theta is chosen so that the image's centre column moves by 3 columns:
    tan(theta) = 3 |hor| / (W - 1)."""
    W, H = 37, 19
    prev_cam = T.camera(rt, W, H)
    hor, ver = (math.sqrt(float(R.vec(v) @ R.vec(v))) for v in (prev_cam.horizontal, prev_cam.vertical))
    theta = math.atan(3.0 * hor / (W - 1))
    cam = turned(rt, W, H, theta)                          # looking further right: what it sees lay 3 columns to the right before
    u, w, pu, pw = R.vec(cam.u), R.vec(cam.w), R.vec(prev_cam.u), R.vec(prev_cam.w)
    cs, sn = math.cos(theta), math.sin(theta)
    assert np.abs(u - (cs * pu + sn * pw)).max() <= 1e-15 and np.abs(w - (-sn * pu + cs * pw)).max() <= 1e-15
    assert np.abs(R.vec(cam.v) - R.vec(prev_cam.v)).max() <= 1e-15 and np.array_equal(R.vec(cam.origin), R.vec(prev_cam.origin))
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a, b = ((xs + 0.5) / (W - 1) - 0.5) * hor, ((ys + 0.5) / (H - 1) - 0.5) * ver
    front = cs - a * sn
    want_fx = (0.5 + (a * cs + sn) / front / hor) * (W - 1) - 0.5
    want_fy = (0.5 + b / front / ver) * (H - 1) - 0.5
    hole = np.ones((H, W), dtype=bool)                       # nothing but sky in both frames
    (s0, f0), (s1, f1) = frames_with_a_fixed_hole(W, H, 2, hole, 80)
    p = rt.temporal_params(W, H, 4, far_misses=True)
    _, st0 = FR.restate(s0, f0, prev_cam, p)
    _, st1, geo = FR.restate(s1, f1, cam, p, st0, prev_cam, geometry=True)
    assert (front > 0).all()
    print("pan: worst |fx - tangent rule| %.3g, |fy - rule| %.3g pixel" % (np.abs(geo["fx"] - want_fx).max(), np.abs(geo["fy"] - want_fy).max()))
    assert np.abs(geo["fx"] - want_fx).max() <= 1e-9 and np.abs(geo["fy"] - want_fy).max() <= 1e-9
    mid = W // 2
    assert 3.0 < want_fx[H // 2, mid] - mid < 3.1          # 3 columns at the image's centre, a little more half a pixel beside it
    # the history is the previous frame's bilinear value there, wherever all four taps are inside
    x0, y0 = np.floor(want_fx).astype(int), np.floor(want_fy).astype(int)
    inside = (x0 >= 0) & (x0 + 1 < W) & (y0 >= 0) & (y0 + 1 < H)
    assert inside.sum() > 0.6 * W * H and geo["accepted"][inside].all()
    assert (np.abs(st1["n"][inside] - 2.0) <= 1e-9).all()
    wx, wy = (want_fx - x0)[..., None], (want_fy - y0)[..., None]
    x0c, y0c = np.clip(x0, 0, W - 2), np.clip(y0, 0, H - 2)
    E = st0["e"]
    bil = (E[y0c, x0c] * (1 - wx) + E[y0c, x0c + 1] * wx) * (1 - wy) + (E[y0c + 1, x0c] * (1 - wx) + E[y0c + 1, x0c + 1] * wx) * wy
    assert np.abs(geo["eh"][inside] - bil[inside]).max() <= 1e-9 * np.abs(E).max()
    assert (st1["n"][:, W - 3:] == 1.0).all()              # the last columns look at what the previous camera never saw


def test_an_uncovered_pixel_takes_only_uncovered_taps(rt):
    """A pan of about half a column over a checkerboard of covered and uncovered previous pixels: a far miss gathers from the
    uncovered ones only (their e is <= 1, the covered ones' is 100) and restarts where all four taps are covered."""
    W, H = 24, 12
    prev_cam = T.camera(rt, W, H)
    hor = math.sqrt(float(R.vec(prev_cam.horizontal) @ R.vec(prev_cam.horizontal)))
    cam = turned(rt, W, H, -math.atan(0.5 * hor / (W - 1)))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sky = ((xs // 2 + ys // 2) % 2 == 0)                    # 2 x 2 blocks: some pixels have four covered taps, some four uncovered
    s0, f0 = T.plane_frame(W, H, 4, np.full(W, 6.0), 90)
    f0.view(np.float64).reshape(H, W, 8)[sky] = 0.0
    p = rt.temporal_params(W, H, 4, demodulate=False, w_min=0.01, far_misses=True)
    _, st0 = FR.restate(s0, f0, prev_cam, p)
    st0["e"][~sky] = 100.0
    st0["e"][sky] = np.random.default_rng(1).random((int(sky.sum()), 3))
    s1 = np.random.default_rng(2).uniform(0.0, 4.0, (H, W, 3))            # e = s / 4 in [0, 1]
    f1 = np.zeros((H, W), dtype=F.FEATURE_DTYPE)                          # the current frame: sky everywhere
    _, st1, geo = FR.restate(s1, f1, cam, p, st0, prev_cam, geometry=True)
    acc = geo["accepted"]
    assert acc.sum() > 0.4 * W * H and (~acc).sum() > 10
    assert geo["eh"][acc].max() <= 1.0 + 1e-12, "a covered tap leaked into a far miss"
    x0, y0 = np.floor(geo["fx"]).astype(int), np.floor(geo["fy"]).astype(int)
    inside = (x0 >= 0) & (x0 + 1 < W) & (y0 >= 0) & (y0 + 1 < H) & geo["history"]
    x0c, y0c = np.clip(x0, 0, W - 2), np.clip(y0, 0, H - 2)
    n_sky = sky[y0c, x0c].astype(int) + sky[y0c, x0c + 1] + sky[y0c + 1, x0c] + sky[y0c + 1, x0c + 1]
    assert (inside & (n_sky == 0)).sum() > 0 and not acc[inside & (n_sky == 0)].any()      # four covered taps: a restart
    wx, wy = geo["fx"] - x0, geo["fy"] - y0
    sky_weight = (sky[y0c, x0c] * (1 - wx) * (1 - wy) + sky[y0c, x0c + 1] * wx * (1 - wy) + sky[y0c + 1, x0c] * (1 - wx) * wy +
                  sky[y0c + 1, x0c + 1] * wx * wy)
    partial = inside & (n_sky > 0) & (n_sky < 4)
    assert partial.sum() > 0 and (sky_weight[partial] < 0.9).sum() > 10                    # the covered taps' weight is missing
    assert np.abs(geo["sw"][inside] - sky_weight[inside]).max() <= 1e-12
    # and the other way round: a covered pixel never reads an uncovered tap (depth > 0 is required), flag or no flag
    _, st2 = FR.restate(s0, f0, cam, p, st0, prev_cam)
    assert_same_bits(st2[~sky], R.restate(s0, f0, cam, rt.temporal_params(W, H, 4, demodulate=False, w_min=0.01), st0, prev_cam)[1][~sky])


# ---- the oracle on the looked-through copy ------------------------------------------------------------------------------------
def small_view(rt, name, W=48, H=32, spp=3):
    s = rt.HostScene(name, seed=2022)
    cam, bg = s.default_view(W / H)
    return s, cam, rt.make_params(W, H, spp, 50, bg, seed=2022), rt.shuffled_rows(H, 2022)


@pytest.mark.parametrize("name", MEDIA_FREE)
def test_copy_equals_the_plain_composition_without_media(rt, O, name):
    s, cam, p, rows = small_view(rt, name)
    assert s.desc.n_media == 0
    ref, st, seen = oracle_features(O, s.desc, cam, p, rows)
    got, st2, seen2, words = S.oracle_surface_features(O, s.desc, cam, p, rows)
    assert_same_bits(got, ref, name)
    assert st2.as_dict() == st.as_dict() and words == seen.draws and seen.medium_draws == 0


@pytest.mark.parametrize("name", ["cornell_smoke", "final_scene"])
def test_copy_has_no_medium_record(rt, O, name):
    s, cam, p, rows = small_view(rt, name)
    d = s.desc
    assert d.n_media > 0
    before = [d.media[i].neg_inv_density for i in range(d.n_media)]
    plain, _, seen_plain = oracle_features(O, d, cam, p, rows)
    got, st, seen, words = S.oracle_surface_features(O, d, cam, p, rows)
    assert [d.media[i].neg_inv_density for i in range(d.n_media)] == before and all(math.isfinite(v) for v in before)    # restored
    assert any(k[0] == F.RT_MAT_ISOTROPIC for k in seen_plain.kinds)                       # the view does look at a medium
    assert not any(k[0] == F.RT_MAT_ISOTROPIC for k in seen.kinds)
    # The normal (1, 0, 0) x hits is a medium's signature, and also that of a wall or a box side that faces -x: the signature
    # must be gone wherever the first-hit records had it from a medium, and what is left of it must be surfaces sample by sample.
    medium_like = lambda f: (f["hits"] > 0) & (f["normal"][:, 0] == f["hits"]) & (f["normal"][:, 1] == 0) & (f["normal"][:, 2] == 0)
    pixels = [(i, px) for i in range(len(rows)) for px in range(p.width)]
    left = np.nonzero(medium_like(got))[0]
    assert medium_like(plain).sum() > len(left)            # pixels whose every hit was a medium's (1, 0, 0)
    with S.media_looked_through(d):
        again, _, seen_left = oracle_features(O, d, cam, p, rows, pixels=[pixels[k] for k in left])
    assert_same_bits(again, got[left])
    assert all(k[0] in (F.RT_MAT_LAMBERTIAN, F.RT_MAT_METAL, F.RT_MAT_DIELECTRIC, F.RT_MAT_DIFFUSE_LIGHT) for k in seen_left.kinds)
    changed = np.any(got.view(np.uint64).reshape(len(got), 8) != plain.view(np.uint64).reshape(len(got), 8), axis=1)
    assert changed.sum() > 0 and not medium_like(got)[changed & medium_like(plain) & ~np.isin(np.arange(len(got)), left)].any()
    assert words == seen.draws - seen.medium_draws and words >= 2 * p.width * p.height * p.spp        # the two jitter words at least
    assert np.isfinite(got.view(np.float64)).all()
    assert_same_bits(oracle_features(O, d, cam, p, rows)[0], plain, "the scene is what it was")


# ---- what it is for -----------------------------------------------------------------------------------------------------------
def test_surface_records_accumulate_better_on_cornell_smoke(rt, O):
    """cornell_smoke along the grid tool's path (8 cameras, 48 x 48, 4 spp, TEMPORAL_DEFAULTS), the oracle's renders: the MSE
    ratio accumulated / last frame under surface records is below that under first-hit records (measured on the CPU: 0.1854
    against 0.2785; profiles/temporal_media_grid.log)."""
    name, step = R.HELD_OUT
    s, bg, cams, sums, feats = R.oracle_path(rt, O, name, step)
    rows = np.arange(R.PATH_H, dtype=np.uint32)
    surf = [S.oracle_surface_features(O, s.desc, c, R.frame_params(rt, R.PATH_W, R.PATH_H, R.PATH_SPP, bg, k), rows)[0].reshape(R.PATH_H, R.PATH_W)
            for k, c in enumerate(cams)]
    target = R.oracle_target(rt, O, s, bg, cams[-1])
    p = rt.temporal_params(R.PATH_W, R.PATH_H, R.PATH_SPP)
    mse_last = R.mse(sums[-1], R.PATH_SPP, target)
    first_hit = R.mse(R.accumulate(sums, feats, cams, p)[0], R.PATH_SPP, target) / mse_last
    surface = R.mse(R.accumulate(sums, surf, cams, p)[0], R.PATH_SPP, target) / mse_last
    print("cornell_smoke: MSE ratio accumulated / last frame: first-hit records %.4f, surface records %.4f" % (first_hit, surface))
    assert surface < first_hit
