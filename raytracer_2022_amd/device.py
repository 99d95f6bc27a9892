"""Device side: a scene resident in HBM and the render calls (include/rt2022.h)."""
import ctypes as C

import numpy as np

from . import _ffi as F


def query_rays(origins, directions, time=0.0, t_min=0.001, t_max=np.inf, rng_state=None):
    """An array of QUERY_RAY_DTYPE records (rt_query_ray) for rt_intersect: `origins` / `directions` are (n, 3) or (3,),
    the other fields arrays of n or scalars, all broadcast to n rays. t_min defaults to ray_color's 0.001 (main.rs:243),
    t_max to +inf. rng_state=None gives ray i the state i (the draws of a ConstantMedium on its path)."""
    o = np.asarray(origins, dtype=np.float64)
    d = np.asarray(directions, dtype=np.float64)
    if o.shape[-1:] != (3,) or d.shape[-1:] != (3,) or o.ndim > 2 or d.ndim > 2:
        raise ValueError("origins and directions must be (n, 3) or (3,)")
    n = np.broadcast_shapes(o.shape[:-1], d.shape[:-1], np.shape(time), np.shape(t_min), np.shape(t_max),
                            np.shape(rng_state) if rng_state is not None else ())
    n = n[0] if n else 1
    rays = np.zeros(n, dtype=F.QUERY_RAY_DTYPE)
    rays["origin"] = np.broadcast_to(o, (n, 3))
    rays["direction"] = np.broadcast_to(d, (n, 3))
    rays["time"] = np.broadcast_to(np.asarray(time, dtype=np.float64), (n,))
    rays["t_min"] = np.broadcast_to(np.asarray(t_min, dtype=np.float64), (n,))
    rays["t_max"] = np.broadcast_to(np.asarray(t_max, dtype=np.float64), (n,))
    rays["rng_state"] = np.arange(n, dtype=np.uint64) if rng_state is None else np.broadcast_to(np.asarray(rng_state, dtype=np.uint64), (n,))
    return rays


def radiance_rays(origins, directions, time=0.0, rng_state=None):
    """An array of RADIANCE_RAY_DTYPE records (rt_radiance_ray) for rt_radiance: `origins` / `directions` are (n, 3) or (3,),
    `time` and `rng_state` arrays of n or scalars, all broadcast to n rays. rng_state=None gives ray i the state i (its samples
    draw from path_key(i, 0, 0, s))."""
    o = np.asarray(origins, dtype=np.float64)
    d = np.asarray(directions, dtype=np.float64)
    if o.shape[-1:] != (3,) or d.shape[-1:] != (3,) or o.ndim > 2 or d.ndim > 2:
        raise ValueError("origins and directions must be (n, 3) or (3,)")
    n = np.broadcast_shapes(o.shape[:-1], d.shape[:-1], np.shape(time), np.shape(rng_state) if rng_state is not None else ())
    n = n[0] if n else 1
    rays = np.zeros(n, dtype=F.RADIANCE_RAY_DTYPE)
    rays["origin"] = np.broadcast_to(o, (n, 3))
    rays["direction"] = np.broadcast_to(d, (n, 3))
    rays["time"] = np.broadcast_to(np.asarray(time, dtype=np.float64), (n,))
    rays["rng_state"] = np.arange(n, dtype=np.uint64) if rng_state is None else np.broadcast_to(np.asarray(rng_state, dtype=np.uint64), (n,))
    return rays


def radiance_params(spp=1, background=(0.0, 0.0, 0.0), t_min=0.001, max_depth=50, flags=0):
    """rt_radiance_params: samples per ray, ray_color's background, t_min (main.rs:243) and depth, RT_FLAG_* bits."""
    p = F.rt_radiance_params()
    p.background[:] = [float(c) for c in background]
    p.t_min, p.max_depth, p.spp, p.flags = t_min, max_depth, spp, flags
    return p


def scatter_params(background=(0.0, 0.0, 0.0), t_min=0.001, flags=0):
    """rt_scatter_params: what a miss returns, the t_min of every next ray (main.rs:243), RT_FLAG_COUNTERS or 0."""
    p = F.rt_scatter_params()
    p.background[:] = [float(c) for c in background]
    p.t_min, p.flags = t_min, flags
    return p


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def path_key(seed, frame, pixel, sample):
    """The stream key of a path (rt_math.h: path_key): seed, frame, absolute pixel index, sample → the uint64 state its draws
    start from. rt_radiance keys sample s of a ray as path_key(ray.rng_state, 0, 0, s). Scalars give a Python int; arrays
    (broadcast against each other, taken modulo 2^64) give a uint64 array."""
    args = [np.asarray(a) for a in (seed, frame, pixel, sample)]
    scalar = all(a.ndim == 0 for a in args)
    s, f, p, k = (np.atleast_1d(a if a.dtype == np.uint64 else np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in a.ravel()], dtype=np.uint64).reshape(a.shape))
                  for a in args)
    one = np.uint64(1)
    with np.errstate(over="ignore"):
        h = _mix64(s + np.uint64(0x9E3779B97F4A7C15) * (f + one))
        h = _mix64(h ^ (np.uint64(0xD1B54A32D192ED03) * (p + one)))
        h = _mix64(h ^ (np.uint64(0x8CB92BA72F3D8DD7) * (k + one)))
    return int(h[0]) if scalar else h


def unwind(recs_per_step, depth_terminal=(0.0, 0.0, 0.0)):
    """The radiance of the paths whose scatter records are `recs_per_step`: a list over the steps of SCATTER_REC_DTYPE arrays of n
    entries each (entry i of every step belongs to path i; the steps chained with prev) → (n, 3) float64.
    Path i has the live records r_0 .. r_{k-1} (SPECULAR or DIFFUSE) up to its first record that is not live; T is that
    record's radiance, or `depth_terminal` when every step is live (the depth ran out: ray_color returns (0, 0, 0)). Then
    L = T and, for j = k-1 .. 0, L = 0 + (weight_j * L) / pdf_j component-wise, in plain float64: the engine's tape step."""
    steps = [np.ascontiguousarray(r, dtype=F.SCATTER_REC_DTYPE) for r in recs_per_step]
    n = len(steps[0]) if steps else 0
    live = [(r["status"] == F.RT_SCATTER_SPECULAR) | (r["status"] == F.RT_SCATTER_DIFFUSE) for r in steps]
    L = np.empty((n, 3), dtype=np.float64)
    L[:] = np.asarray(depth_terminal, dtype=np.float64)
    alive = np.ones(n, dtype=bool)                         # alive[i] at step j: every record of path i before j is live
    ended_at = np.full(n, len(steps), dtype=np.int64)
    for j, lv in enumerate(live):
        stop = alive & ~lv
        ended_at[stop] = j
        L[stop] = steps[j]["radiance"][stop]
        alive &= lv
    with np.errstate(all="ignore"):
        for j in range(len(steps) - 1, -1, -1):
            on = ended_at > j
            w, p = steps[j]["weight"][on], steps[j]["pdf"][on]
            L[on] = 0.0 + (w * L[on]) / p[:, None]
    return L


def radiance_by_steps(dev, rays, spp=1, max_depth=50, background=(0.0, 0.0, 0.0), t_min=0.001, on_step=None, want_stats=False):
    """rt_radiance's sums by the caller-driven loop intersect → scatter(prev=...), bit for bit: `rays` (RADIANCE_RAY_DTYPE) →
    (n, 3) float64 sums over spp samples, not divided by spp. Sample s of ray i starts from path_key(rays[i].rng_state, 0, 0, s);
    a sample takes up to max_depth steps and the loop stops early when no entry is live; the steps are unwound (unwind) and the
    samples added in order from 0. on_step(k, rays, hits, recs) is called after step k of every sample with the step's query rays,
    hit records and scatter records (a caller's AOVs). want_stats=True adds a dict: rng_draws and light_pdf_tests summed over
    the steps (the hits' words included) and rays, the live entries of the intersect calls."""
    r = np.ascontiguousarray(rays, dtype=F.RADIANCE_RAY_DTYPE)
    n = len(r)
    total = np.zeros((n, 3), dtype=np.float64)
    stats = {"rng_draws": 0, "light_pdf_tests": 0, "rays": 0}
    for s in range(spp):
        q = query_rays(r["origin"], r["direction"], r["time"], t_min, np.finfo(np.float64).max,
                       path_key(r["rng_state"], 0, 0, s)) if n else np.zeros(0, dtype=F.QUERY_RAY_DTYPE)
        steps, prev = [], None
        live = np.ones(n, dtype=bool)
        for k in range(max_depth):
            if not live.any():
                break
            hits = dev.intersect(q)
            out = dev.scatter(q, hits, background, t_min, prev, want_stats=want_stats)
            recs, nxt = out[0], out[1]
            if want_stats:
                stats["rays"] += int(live.sum())
                stats["rng_draws"] += int(hits["rng_draws"][live].sum()) + out[2].rng_draws
                stats["light_pdf_tests"] += out[2].light_pdf_tests
            if on_step is not None:
                on_step(k, q, hits, recs)
            steps.append(recs)
            live = (recs["status"] == F.RT_SCATTER_SPECULAR) | (recs["status"] == F.RT_SCATTER_DIFFUSE)
            q, prev = nxt, recs
        with np.errstate(all="ignore"):
            total += unwind(steps) if steps else np.zeros((n, 3))
    return (total, stats) if want_stats else total


def denoise_params(width, height, spp, n_iter=5, sigma_color=1.0, sigma_normal=0.3, sigma_depth=np.inf, sigma_albedo=0.3,
                   albedo_floor=1e-3, demodulate=True):
    """rt_denoise_params: the image, the divisor of the sums, the a-trous iterations and the edge-stopping sigmas (+inf
    switches a term off); demodulate=False sets RT_DENOISE_NO_DEMODULATE."""
    p = F.rt_denoise_params()
    p.width, p.height, p.spp, p.n_iter = width, height, spp, n_iter
    p.sigma_color, p.sigma_normal, p.sigma_depth, p.sigma_albedo = sigma_color, sigma_normal, sigma_depth, sigma_albedo
    p.albedo_floor = albedo_floor
    p.flags = 0 if demodulate else F.RT_DENOISE_NO_DEMODULATE
    return p


def denoise_workspace_bytes(params):
    """rt_denoise_workspace_bytes: device bytes denoise_device needs for params' image (0: invalid params)."""
    return int(F.lib().rt_denoise_workspace_bytes(C.byref(params)))


def _row_list(row_ids, height):
    """A host row list as the C ABI takes it: contiguous uint32, one entry per image row (None: no list)."""
    if row_ids is None:
        return None
    rows = np.ascontiguousarray(row_ids, dtype=np.uint32)
    if rows.size != height:
        raise ValueError("row_ids must hold one entry per image row")
    return rows


def _hold_pixels(params, message, *buffers):
    """width * height of params' image, once every (array, values per pixel) of `buffers` holds that many pixels; else
    ValueError(message)."""
    n = params.width * params.height
    if any(a.size != per_pixel * n for a, per_pixel in buffers):
        raise ValueError(message)
    return n


def denoise(rgb_sum, features, params, row_ids=None, want_ms=False):
    """rt_denoise with host buffers: a render's sums (height, width, 3) and its FEATURE_DTYPE records (height, width), both
    in the order of `row_ids` (None: image order; else the frame's row list, a permutation of the image's rows) -> the
    filtered sums, same shape and order [, device ms]."""
    s = np.ascontiguousarray(rgb_sum, dtype=np.float64)
    f = np.ascontiguousarray(features, dtype=F.FEATURE_DTYPE)
    _hold_pixels(params, "rgb_sum and features must hold width * height pixels", (s, 3), (f, 1))
    rows = _row_list(row_ids, params.height)
    out = np.empty_like(s)
    ms = C.c_double()
    F.check(F.lib().rt_denoise(s.ctypes.data, f.ctypes.data, rows.ctypes.data if rows is not None else None, C.byref(params),
                               out.ctypes.data, C.byref(ms)))
    return (out, ms.value) if want_ms else out


def denoise_device(d_rgb_sum_ptr, d_features_ptr, params, d_out_ptr, d_workspace_ptr, d_row_ids_ptr=None, stream_ptr=None):
    """rt_denoise_device: device pointers in (sums, rt_feature records, room for the filtered sums — it may be the input —
    and denoise_workspace_bytes(params) bytes of workspace, all 16-byte aligned; `height` row ids or None), enqueued on
    `stream_ptr` (hipStream_t as int). With no row list the call does not synchronise."""
    F.check(F.lib().rt_denoise_device(C.c_void_p(d_rgb_sum_ptr), C.c_void_p(d_features_ptr), C.c_void_p(d_row_ids_ptr or 0),
                                      C.byref(params), C.c_void_p(d_out_ptr), C.c_void_p(d_workspace_ptr), C.c_void_p(stream_ptr or 0)))


# The tuned parameters of the dual filter: the point of tools/denoise_dual_grid.py's grid with the smallest sum of the three
# views' MSE ratios (profiles/denoise_dual_grid.log). sigma_color goes into denoise_params, the others into denoise_dual_params.
DUAL_DEFAULTS = {"sigma_color": 2.0, "var_iter": 1, "var_floor": 1e-6}


def denoise_dual_params(var_iter=DUAL_DEFAULTS["var_iter"], var_floor=DUAL_DEFAULTS["var_floor"]):
    """rt_denoise_dual_params: prefilter passes over the variance estimate and the floor under the colour distance. The
    defaults, with sigma_color=DUAL_DEFAULTS["sigma_color"] in denoise_params, are the grid point of
    tools/denoise_dual_grid.py with the smallest summed MSE ratio (profiles/denoise_dual_grid.log)."""
    q = F.rt_denoise_dual_params()
    q.var_iter, q.flags, q.var_floor = var_iter, 0, var_floor
    return q


def denoise_dual_workspace_bytes(params):
    """rt_denoise_dual_workspace_bytes: device bytes denoise_dual_device needs for params' image (0: invalid params)."""
    return int(F.lib().rt_denoise_dual_workspace_bytes(C.byref(params)))


def two_frame_rows(row_ids, height):
    """The row list of a two-frame render or feature call over one frame's list: rows ++ (rows + height). The two halves of
    the call's output are the halves A and B of denoise_dual."""
    rows = np.ascontiguousarray(row_ids, dtype=np.uint32)
    return np.concatenate([rows, rows + np.uint32(height)])


def denoise_dual(sum_a, sum_b, feat_a, feat_b, params, dual_params=None, row_ids=None, want_variance=False, want_ms=False):
    """rt_denoise_dual with host buffers: two half-sample renders' sums (height, width, 3) and FEATURE_DTYPE records (height,
    width) of params.spp samples each, in the order of `row_ids` (None: image order) -> the filtered sums of 2 * spp samples,
    same shape and order [, the residual variance (height, width)] [, device ms]. params.sigma_color counts estimated
    standard deviations: DUAL_DEFAULTS["sigma_color"] is the tuned value."""
    s = [np.ascontiguousarray(x, dtype=np.float64) for x in (sum_a, sum_b)]
    f = [np.ascontiguousarray(x, dtype=F.FEATURE_DTYPE) for x in (feat_a, feat_b)]
    n = _hold_pixels(params, "both halves' rgb_sum and features must hold width * height pixels", (s[0], 3), (s[1], 3), (f[0], 1), (f[1], 1))
    rows = _row_list(row_ids, params.height)
    q = dual_params if dual_params is not None else denoise_dual_params()
    out = np.empty_like(s[0])
    var = np.empty(s[0].shape[:-1] if s[0].ndim > 1 else (n,), dtype=np.float64) if want_variance else None
    ms = C.c_double()
    F.check(F.lib().rt_denoise_dual(s[0].ctypes.data, s[1].ctypes.data, f[0].ctypes.data, f[1].ctypes.data,
                                    rows.ctypes.data if rows is not None else None, C.byref(params), C.byref(q), out.ctypes.data,
                                    var.ctypes.data if var is not None else None, C.byref(ms)))
    res = (out,) + ((var,) if want_variance else ()) + ((ms.value,) if want_ms else ())
    return res[0] if len(res) == 1 else res


def denoise_dual_device(d_sum_a_ptr, d_sum_b_ptr, d_feat_a_ptr, d_feat_b_ptr, params, dual_params, d_out_ptr, d_workspace_ptr,
                        d_out_variance_ptr=None, d_row_ids_ptr=None, stream_ptr=None):
    """rt_denoise_dual_device: device pointers in (each half's sums and rt_feature records, room for the filtered sums — it
    may be either half's — and denoise_dual_workspace_bytes(params) bytes of workspace, optionally room for width * height
    variances, all 16-byte aligned; `height` row ids or None), enqueued on `stream_ptr` (hipStream_t as int). With no row
    list the call does not synchronise."""
    F.check(F.lib().rt_denoise_dual_device(C.c_void_p(d_sum_a_ptr), C.c_void_p(d_sum_b_ptr), C.c_void_p(d_feat_a_ptr), C.c_void_p(d_feat_b_ptr),
                                           C.c_void_p(d_row_ids_ptr or 0), C.byref(params), C.byref(dual_params), C.c_void_p(d_out_ptr),
                                           C.c_void_p(d_out_variance_ptr or 0), C.c_void_p(d_workspace_ptr), C.c_void_p(stream_ptr or 0)))


# The tuned parameters of the temporal accumulation: the point of tools/temporal_grid.py's grid with the smallest sum of the
# three camera paths' MSE ratios accumulated / last frame (profiles/temporal_grid.log). The paths have 8 frames, so the grid
# cannot tell n_max 8 from 32: the first of the two stands.
TEMPORAL_DEFAULTS = {"tol_depth": 0.2, "tol_normal": 0.3, "n_max": 8.0, "w_min": 0.25}


def temporal_params(width, height, spp, tol_depth=TEMPORAL_DEFAULTS["tol_depth"], tol_normal=TEMPORAL_DEFAULTS["tol_normal"],
                    n_max=TEMPORAL_DEFAULTS["n_max"], w_min=TEMPORAL_DEFAULTS["w_min"], albedo_floor=1e-3, demodulate=True,
                    far_misses=False):
    """rt_temporal_params: the image, the divisor of the sums, the relative depth and squared normal tolerances of a history tap
    (+inf switches a test off), the cap of the history length and the least bilinear weight that still counts as history;
    demodulate=False sets RT_TEMPORAL_NO_DEMODULATE; far_misses=True sets RT_TEMPORAL_FAR_MISSES: a pixel that is not covered
    reprojects as a point at infinity and takes history from the previous state's uncovered pixels."""
    p = F.rt_temporal_params()
    p.width, p.height, p.spp = width, height, spp
    p.flags = (0 if demodulate else F.RT_TEMPORAL_NO_DEMODULATE) | (F.RT_TEMPORAL_FAR_MISSES if far_misses else 0)
    p.tol_depth, p.tol_normal, p.n_max, p.w_min, p.albedo_floor = tol_depth, tol_normal, n_max, w_min, albedo_floor
    return p


def temporal_workspace_bytes(params):
    """rt_temporal_workspace_bytes: device bytes temporal_device needs for params' image (0: invalid params)."""
    return int(F.lib().rt_temporal_workspace_bytes(C.byref(params)))


def temporal(sums, features, cam, params, prev=None, prev_cam=None, row_ids=None, want_ms=False):
    """rt_temporal with host buffers: a frame's sums (height, width, 3) and FEATURE_DTYPE records (height, width) in the order
    of `row_ids` (None: image order), its camera, and the previous frame's state (TEMPORAL_PIXEL_DTYPE, (height, width), image
    order; None: the first frame) with that frame's camera -> (the accumulated sums, same shape and order, the new state in
    image order) [, device ms]."""
    s = np.ascontiguousarray(sums, dtype=np.float64)
    f = np.ascontiguousarray(features, dtype=F.FEATURE_DTYPE)
    _hold_pixels(params, "sums and features must hold width * height pixels", (s, 3), (f, 1))
    pv = None
    if prev is not None:
        pv = np.ascontiguousarray(prev, dtype=F.TEMPORAL_PIXEL_DTYPE)
        _hold_pixels(params, "prev must hold width * height pixels", (pv, 1))
    rows = _row_list(row_ids, params.height)
    out = np.empty_like(s)
    state = np.empty((params.height, params.width), dtype=F.TEMPORAL_PIXEL_DTYPE)
    ms = C.c_double()
    F.check(F.lib().rt_temporal(s.ctypes.data, f.ctypes.data, rows.ctypes.data if rows is not None else None, C.byref(cam),
                                pv.ctypes.data if pv is not None else None, C.byref(prev_cam) if prev_cam is not None else None,
                                C.byref(params), state.ctypes.data, out.ctypes.data, C.byref(ms)))
    return (out, state, ms.value) if want_ms else (out, state)


def temporal_device(d_sums_ptr, d_features_ptr, cam, params, d_state_out_ptr, d_out_ptr, d_workspace_ptr, d_prev_ptr=None, prev_cam=None,
                    d_row_ids_ptr=None, stream_ptr=None):
    """rt_temporal_device: device pointers in (sums, rt_feature records, room for the new state and for the accumulated sums —
    these may be the input sums — temporal_workspace_bytes(params) bytes of workspace, the previous state or None, all 16-byte
    aligned; `height` row ids or None), enqueued on `stream_ptr` (hipStream_t as int). The two states must not overlap. With
    no row list the call does not synchronise."""
    F.check(F.lib().rt_temporal_device(C.c_void_p(d_sums_ptr), C.c_void_p(d_features_ptr), C.c_void_p(d_row_ids_ptr or 0), C.byref(cam),
                                       C.c_void_p(d_prev_ptr or 0), C.byref(prev_cam) if prev_cam is not None else None, C.byref(params),
                                       C.c_void_p(d_state_out_ptr), C.c_void_p(d_out_ptr), C.c_void_p(d_workspace_ptr),
                                       C.c_void_p(stream_ptr or 0)))


def pixel_ids(frame, py, px, width, height):
    """The entry ids of rt_render_pixels: frame * (width * height) + py * width + px as uint64, the arguments broadcast against
    each other (py counts upwards, as in a render's row ids)."""
    f, y, x = (np.asarray(v, dtype=np.uint64) for v in (frame, py, px))
    return np.ascontiguousarray(f * np.uint64(width * height) + y * np.uint64(width) + x, dtype=np.uint64)


def adaptive_params(width, height, scale, max_units, first_frame=0):
    """rt_adaptive_params: the image, the frame of a pixel's first new unit, the cap on units per pixel and the factor that
    turns an error into units (units = clamp(trunc(err * scale), 0, max_units))."""
    p = F.rt_adaptive_params()
    p.width, p.height, p.first_frame, p.max_units, p.scale, p.flags, p._pad = width, height, first_frame, max_units, scale, 0, 0
    return p


def adaptive_workspace_bytes(params):
    """rt_adaptive_workspace_bytes: device bytes adaptive_plan_device needs for params' image (0: invalid params)."""
    return int(F.lib().rt_adaptive_workspace_bytes(C.byref(params)))


def plan_units(err, scale, max_units):
    """The plan's own formula in numpy: units = !(t >= 1) ? 0 : (t >= max_units ? max_units : trunc(t)), t = err * scale."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(err, dtype=np.float64) * np.float64(scale)
        ok = t >= 1.0                                             # (False for NaN)
        capped = np.minimum(np.where(ok, t, 0.0), np.float64(max_units))
    return np.where(ok, capped, 0.0).astype(np.uint32)


def adaptive_scale(err, budget_units, max_units, steps=256):
    """A scale for rt_adaptive_params: a bisection (numpy, on the plan's own formula) for the largest scale it finds whose
    plan totals at most `budget_units`. Returns 0.0 when no positive scale it tries fits (a budget below one unit, or no
    finite positive error): the caller then plans nothing. The total is monotone in the scale, so the bisection keeps
    `lo` with total(lo) <= budget and `hi` with total(hi) > budget (or every pixel at max_units) and halves between them."""
    e = np.asarray(err, dtype=np.float64).ravel()
    total = lambda s: int(plan_units(e, s, max_units).sum(dtype=np.uint64))
    pos = e[np.isfinite(e) & (e > 0.0)]
    if budget_units <= 0 or pos.size == 0:
        return 0.0
    hi = float(max_units) / float(pos.min())                       # every positive finite pixel at max_units (unless it overflows)
    if not np.isfinite(hi):
        hi = np.finfo(np.float64).max
    for _ in range(4):                                             # (the quotient may round to a hair below: min * hi < max_units)
        if float(pos.min()) * hi >= float(max_units) or hi == np.finfo(np.float64).max:
            break
        hi = float(np.nextafter(hi, np.inf))
    if total(hi) <= budget_units:
        return hi
    lo = 1.0 / float(pos.max()) * 0.5                              # below one unit everywhere (+inf errors aside)
    if not (lo > 0.0) or total(lo) > budget_units:
        return 0.0
    for _ in range(steps):
        mid = lo + (hi - lo) * 0.5
        if not (lo < mid < hi):
            break
        if total(mid) <= budget_units:
            lo = mid
        else:
            hi = mid
    return lo


def adaptive_plan(err, params, row_ids=None, capacity=None):
    """rt_adaptive_plan with host buffers: the error map (height, width) in the order of `row_ids` (None: image order) ->
    (units uint32 (height, width), offsets uint64 (n + 1), entries uint64 (total) or None, total). capacity=None sizes the
    list by the plan's own formula; a capacity below the total gives entries None."""
    e = np.ascontiguousarray(err, dtype=np.float64)
    n = _hold_pixels(params, "err must hold width * height pixels", (e, 1))
    rows = _row_list(row_ids, params.height)
    if capacity is None:
        capacity = int(plan_units(e, params.scale, params.max_units).sum(dtype=np.uint64))
    units = np.zeros(e.shape, dtype=np.uint32)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    entries = np.zeros(capacity, dtype=np.uint64)
    total = C.c_uint64()
    F.check(F.lib().rt_adaptive_plan(e.ctypes.data, rows.ctypes.data if rows is not None else None, C.byref(params), units.ctypes.data,
                                     offsets.ctypes.data, entries.ctypes.data if capacity else None, capacity, C.byref(total)))
    return units, offsets, (entries[:total.value] if total.value <= capacity else None), total.value


def adaptive_plan_device(d_err_ptr, params, d_units_ptr, d_offsets_ptr, d_entries_ptr, capacity, d_workspace_ptr, d_row_ids_ptr=None,
                         stream_ptr=None):
    """rt_adaptive_plan_device: device pointers in (the error map and adaptive_workspace_bytes(params) bytes of workspace,
    16-byte aligned; n units, n + 1 offsets, room for `capacity` entries — None with capacity 0 counts only), run on
    `stream_ptr` (hipStream_t as int) -> the total. The call synchronises the stream once."""
    total = C.c_uint64()
    F.check(F.lib().rt_adaptive_plan_device(C.c_void_p(d_err_ptr), C.c_void_p(d_row_ids_ptr or 0), C.byref(params), C.c_void_p(d_units_ptr),
                                            C.c_void_p(d_offsets_ptr), C.c_void_p(d_entries_ptr or 0), capacity, C.c_void_p(d_workspace_ptr),
                                            C.c_void_p(stream_ptr or 0), C.byref(total)))
    return total.value


def adaptive_merge_device(d_entry_sums_ptr, d_units_ptr, d_offsets_ptr, n_pixels, spp, d_acc_sum_ptr, d_acc_n_ptr, stream_ptr=None):
    """rt_adaptive_merge_device: adds every pixel's units of entry sums to its accumulator (3 doubles) and units * spp to its
    sample count (1 double); a pure enqueue on `stream_ptr`."""
    F.check(F.lib().rt_adaptive_merge_device(C.c_void_p(d_entry_sums_ptr), C.c_void_p(d_units_ptr), C.c_void_p(d_offsets_ptr), n_pixels, spp,
                                             C.c_void_p(d_acc_sum_ptr), C.c_void_p(d_acc_n_ptr), C.c_void_p(stream_ptr or 0)))


def adaptive_resolve_device(d_acc_sum_ptr, d_acc_n_ptr, n_pixels, spp_out, d_out_ptr, stream_ptr=None):
    """rt_adaptive_resolve_device: out = (acc / acc_n) * spp_out, sums of spp_out samples (out may be acc); a pure enqueue."""
    F.check(F.lib().rt_adaptive_resolve_device(C.c_void_p(d_acc_sum_ptr), C.c_void_p(d_acc_n_ptr), n_pixels, spp_out, C.c_void_p(d_out_ptr),
                                               C.c_void_p(stream_ptr or 0)))


def adaptive_merge_features_device(d_entry_features_ptr, d_units_ptr, d_offsets_ptr, n_pixels, d_acc_ptr, stream_ptr=None):
    """rt_adaptive_merge_features_device: adds every pixel's units of entry rt_feature records (features_pixels_device's, 16-byte
    aligned) to its accumulated record, field by field in entry order; the sample count is adaptive_merge_device's. A pure enqueue."""
    F.check(F.lib().rt_adaptive_merge_features_device(C.c_void_p(d_entry_features_ptr), C.c_void_p(d_units_ptr), C.c_void_p(d_offsets_ptr),
                                                      n_pixels, C.c_void_p(d_acc_ptr), C.c_void_p(stream_ptr or 0)))


def adaptive_resolve_features_device(d_acc_ptr, d_acc_n_ptr, n_pixels, spp_out, d_out_ptr, stream_ptr=None):
    """rt_adaptive_resolve_features_device: out = (acc / acc_n) * spp_out on all eight fields of every record, records "of
    spp_out samples" for the denoisers (out may be acc); a pure enqueue."""
    F.check(F.lib().rt_adaptive_resolve_features_device(C.c_void_p(d_acc_ptr), C.c_void_p(d_acc_n_ptr), n_pixels, spp_out,
                                                        C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0)))


# The error metric of render_adaptive: the dual filter's residual variance relative to the squared luminance of the filtered
# demodulated mean, err = variance / (luma^2 + ADAPTIVE_LUMA_FLOOR). A documented default, not a tuned one.
ADAPTIVE_LUMA_FLOOR = 0.01


def render_adaptive(dev, cam, params, total_spp, rounds=2, max_units=4, denoise=None, dual=None, device="cuda", profile=False,
                    want_state=False, guides="initial", surfaces=False, specular=False):
    """Adaptive sampling on torch device buffers, image order, all stages in HBM:
    an initial two-frame render (halves A and B, params.spp samples per pixel each) plus their features; then per round
    denoise_dual (variance) -> err = variance / (luma^2 + 0.01) of the filtered demodulated mean -> adaptive_scale for the
    round's share of the budget -> a plan for A and one for B (the same units, frames f.. and f + max_units..) -> ONE pixel
    render of both lists -> two merges. The unit of extra work is params.spp samples of one half, so a unit costs 2 * spp
    samples; the budget is total_spp * width * height samples, the initial frames included.
    Returns (sums, counts, log): the resolved sums of A + B as a (height, width, 3) float64 tensor "of total_spp samples"
    (rt_tonemap_device / denoisers apply with spp = total_spp), the samples each pixel really got as a (height, width)
    float64 tensor, and a list of per-round dicts (budget_units, scale, total, pixels, samples).
    profile=True adds the device ms of each round's plan calls, pixel render and merges to its dict (HIP events, a
    synchronisation each). want_state=True returns a fourth value: {"acc", "acc_n", "feat"}, the halves' accumulators (2, H, W,
    3), their sample counts (2, H, W) and the initial frames' rt_feature records (2, n, 8) — what a dual denoise of the result needs.
    guides="initial" filters and ranks every round under the initial frames' records. guides="all" carries the records through the
    accumulators too: each round also makes ONE features_pixels_device call over the pixel render's entries and two feature merges
    into a (2, n, 8) accumulator that starts as the initial frames' records; at the top of each round the halves' guides are
    resolved to sums of spp samples, and those feed the dual denoise and the metric's demodulation. The state then gains
    "feat_acc", the accumulated records (their sample counts are "acc_n"); "feat" stays the initial frames' records.
    surfaces=True passes RT_FLAG_SURFACES to every feature call made here: the guides are those of the surfaces behind media.
    specular=True passes RT_FLAG_SPECULAR likewise: the guides follow each sample through glass and mirrors.
    The result depends on params.seed and the arguments only: two calls give the same bits."""
    import torch
    W, H, spp = params.width, params.height, params.spp
    n = W * H
    if spp == 0 or total_spp < 2 * spp:
        raise ValueError("total_spp must cover the two initial frames of params.spp samples each")
    if guides not in ("initial", "all"):
        raise ValueError('guides must be "initial" or "all"')
    all_guides = guides == "all"
    ptr = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    p = F.rt_params.from_buffer_copy(params)
    p.n_frames = 2
    p.progress_cb = None
    p.flags = 0
    rows = torch.from_numpy(two_frame_rows(np.arange(H, dtype=np.uint32), H).astype(np.int32)).to(device)
    acc = torch.empty((2, H, W, 3), dtype=torch.float64, device=device)          # the halves' accumulators: A, B
    feat = torch.empty((2, n, 8), dtype=torch.float64, device=device)            # rt_feature records
    dev.render_device(cam, p, ptr(rows), 2 * H, ptr(acc), stream_ptr=stream)
    dev.features_device(cam, p, ptr(rows), 2 * H, ptr(feat), stream_ptr=stream, surfaces=surfaces, specular=specular)
    acc_n = torch.full((2, H, W), float(spp), dtype=torch.float64, device=device)
    dn = denoise if denoise is not None else denoise_params(W, H, spp, sigma_color=DUAL_DEFAULTS["sigma_color"])
    dn.spp = spp
    dq = dual if dual is not None else denoise_dual_params()
    ws = torch.empty(denoise_dual_workspace_bytes(dn), dtype=torch.uint8, device=device)
    halves = torch.empty((2, H, W, 3), dtype=torch.float64, device=device)       # A and B as sums of spp samples
    filt = torch.empty((H, W, 3), dtype=torch.float64, device=device)
    var = torch.empty((H, W), dtype=torch.float64, device=device)
    units = torch.empty(n, dtype=torch.int32, device=device)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=device)
    ap0 = adaptive_params(W, H, 1.0, max_units)
    aws = torch.empty(adaptive_workspace_bytes(ap0), dtype=torch.uint8, device=device)

    def demodulator(g):                                                           # of two halves' records, sums of spp samples each
        alb = ((g[0, :, 0:3] + g[1, :, 0:3]) / float(spp + spp)).reshape(H, W, 3)
        return torch.where(alb > dn.albedo_floor, alb, torch.full_like(alb, dn.albedo_floor)) if not (dn.flags & F.RT_DENOISE_NO_DEMODULATE) \
            else torch.ones_like(alb)
    m = demodulator(feat)
    feat_acc = feat.clone() if all_guides else None                               # the halves' accumulated records
    guide = torch.empty_like(feat) if all_guides else feat                        # ... resolved to sums of spp samples
    budget = (total_spp * n - 2 * spp * n) // (2 * spp)                           # units left

    def timed(entry, key, call):
        if not profile:
            return call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = call()
        e1.record()
        e1.synchronize()
        entry[key] = entry.get(key, 0.0) + e0.elapsed_time(e1)
        return r
    frame, log = 2, []
    for rnd in range(rounds):
        share = budget // (rounds - rnd)
        if share <= 0:
            break
        for h in range(2):
            adaptive_resolve_device(ptr(acc[h]), ptr(acc_n[h]), n, spp, ptr(halves[h]), stream_ptr=stream)
        if all_guides:
            for h in range(2):
                adaptive_resolve_features_device(ptr(feat_acc[h]), ptr(acc_n[h]), n, spp, ptr(guide[h]), stream_ptr=stream)
            m = demodulator(guide)
        denoise_dual_device(ptr(halves[0]), ptr(halves[1]), ptr(guide[0]), ptr(guide[1]), dn, dq, ptr(filt), ptr(ws),
                            d_out_variance_ptr=ptr(var), stream_ptr=stream)
        e = filt / (m * float(spp + spp))
        luma = 0.2126 * e[..., 0] + 0.7152 * e[..., 1] + 0.0722 * e[..., 2]
        err = (var / (luma * luma + ADAPTIVE_LUMA_FLOOR)).contiguous()
        scale = adaptive_scale(err.cpu().numpy(), share, max_units)
        entry = {"round": rnd, "budget_units": int(share), "scale": scale, "total": 0, "pixels": 0, "samples": 0}
        log.append(entry)
        if not scale > 0.0:
            continue
        ap = adaptive_params(W, H, scale, max_units, first_frame=frame)
        total = timed(entry, "plan_ms", lambda: adaptive_plan_device(ptr(err), ap, ptr(units), ptr(offsets), None, 0, ptr(aws), stream_ptr=stream))
        if total == 0:
            continue
        entries = torch.empty(2 * total, dtype=torch.int64, device=device)
        sums = torch.empty((2 * total, 3), dtype=torch.float64, device=device)
        timed(entry, "plan_ms", lambda: adaptive_plan_device(ptr(err), ap, ptr(units), ptr(offsets), ptr(entries), total, ptr(aws), stream_ptr=stream))
        ap.first_frame = frame + max_units
        timed(entry, "plan_ms", lambda: adaptive_plan_device(ptr(err), ap, ptr(units), ptr(offsets), ptr(entries[total:]), total, ptr(aws),
                                                             stream_ptr=stream))
        frame += 2 * max_units
        p.n_frames = frame
        timed(entry, "render_pixels_ms", lambda: dev.render_pixels_device(cam, p, ptr(entries), 2 * total, ptr(sums), stream_ptr=stream))
        if all_guides:
            efeat = torch.empty((2 * total, 8), dtype=torch.float64, device=device)
            timed(entry, "features_pixels_ms", lambda: dev.features_pixels_device(cam, p, ptr(entries), 2 * total, ptr(efeat), stream_ptr=stream,
                                                                                          surfaces=surfaces, specular=specular))
            timed(entry, "merge_features_ms", lambda: [adaptive_merge_features_device(ptr(efeat[h * total:]), ptr(units), ptr(offsets), n,
                                                                                      ptr(feat_acc[h]), stream_ptr=stream) for h in range(2)])
        timed(entry, "merge_ms", lambda: [adaptive_merge_device(ptr(sums[h * total:]), ptr(units), ptr(offsets), n, spp, ptr(acc[h]), ptr(acc_n[h]),
                                                                stream_ptr=stream) for h in range(2)])
        budget -= total
        entry.update(total=int(total), pixels=int((units > 0).sum().item()), samples=int(2 * total * spp))
    counts = acc_n[0] + acc_n[1]
    both = acc[0] + acc[1]
    out = torch.empty((H, W, 3), dtype=torch.float64, device=device)
    adaptive_resolve_device(ptr(both), ptr(counts), n, total_spp, ptr(out), stream_ptr=stream)
    torch.cuda.current_stream().synchronize()
    if want_state:
        state = {"acc": acc, "acc_n": acc_n, "feat": feat}
        if all_guides:
            state["feat_acc"] = feat_acc
        return out, counts, log, state
    return out, counts, log


def bvh_workspace_bytes(n_leaves):
    """rt_bvh_workspace_bytes: device bytes bvh_build_device needs for a build over n_leaves leaves."""
    return int(F.lib().rt_bvh_workspace_bytes(n_leaves))


def bvh_build(refs, boxes6, node_base=0):
    """rt_bvh_build with host buffers: n leaf refs and their (n, 6) {min, max} boxes → the max(1, n - 1) records of the linear
    BVH built on the device (BVH_NODE_DTYPE), record j being the node ref node_base + j and record 0 the root."""
    r = np.ascontiguousarray(refs, dtype=np.uint32)
    b = np.ascontiguousarray(boxes6, dtype=np.float64)
    if b.size != 6 * r.size:
        raise ValueError("boxes6 must hold six coordinates per ref")
    out = np.zeros(max(1, r.size - 1), dtype=F.BVH_NODE_DTYPE)
    F.check(F.lib().rt_bvh_build(r.ctypes.data, b.ctypes.data, r.size, node_base, out.ctypes.data))
    return out


def bvh_build_device(d_refs_ptr, d_boxes_ptr, n_leaves, d_out_ptr, d_workspace_ptr, workspace_bytes, node_base=0, stream_ptr=None):
    """rt_bvh_build_device: device pointers in (n uint32 refs, n x 6 doubles, room for max(1, n - 1) rt_bvh_node records,
    bvh_workspace_bytes(n) bytes of workspace; nodes, boxes and workspace 16-byte aligned), ordered on `stream_ptr`
    (hipStream_t as int), which it synchronises once. With torch: tensor.data_ptr() and torch.cuda.current_stream().cuda_stream."""
    F.check(F.lib().rt_bvh_build_device(C.c_void_p(d_refs_ptr), C.c_void_p(d_boxes_ptr), n_leaves, node_base, C.c_void_p(d_out_ptr),
                                        C.c_void_p(d_workspace_ptr), workspace_bytes, C.c_void_p(stream_ptr or 0)))


# The parameters of the ray ordering: the cell of tools/query_bench.py --order-grid with the smallest summed time, ordering plus
# ordered query, over the bounce rays of its four scenes (profiles/ray_order.log, the "grid_best" line). Hardly a cell of that grid beats
# the unordered call on those rays (none by more than 3 %), so what wins is the cheapest sort: no origin word, the face and 2 bits a face axis (with no
# origin word ORIGIN_FIRST and DIRECTION_FIRST are one order). A shuffled batch of coherent rays wants a fine key instead —
# ray_order_params(16, 6) — see DESIGN.md §4.16.
RAY_ORDER_DEFAULTS = {"origin_bits": 0, "dir_bits": 2, "layout": F.RT_ORDER_ORIGIN_FIRST}


def ray_order_params(origin_bits=RAY_ORDER_DEFAULTS["origin_bits"], dir_bits=RAY_ORDER_DEFAULTS["dir_bits"],
                     layout=RAY_ORDER_DEFAULTS["layout"], stride=80):
    """rt_ray_order_params: bits per origin axis (0..16) and per face axis of the direction (0..6), the layout of the key
    (F.RT_ORDER_ORIGIN_FIRST, RT_ORDER_DIRECTION_FIRST, RT_ORDER_FACE_ORIGIN_UV) and the bytes from one ray record to the next
    (80: QUERY_RAY_DTYPE, 64: RADIANCE_RAY_DTYPE). The defaults are RAY_ORDER_DEFAULTS."""
    p = F.rt_ray_order_params()
    p.origin_bits, p.dir_bits, p.layout, p.ray_stride = origin_bits, dir_bits, layout, stride
    return p


def ray_order_workspace_bytes(n_rays):
    """rt_ray_order_workspace_bytes: device bytes ray_order_device needs for n_rays rays."""
    return int(F.lib().rt_ray_order_workspace_bytes(n_rays))


def intersect_ordered_workspace_bytes(n_rays):
    """rt_intersect_ordered_workspace_bytes: device bytes DeviceScene.intersect_ordered_device needs for n_rays rays."""
    return int(F.lib().rt_intersect_ordered_workspace_bytes(n_rays))


def ray_order(rays, params=None, stride=None):
    """rt_ray_order with host buffers: the coherence order of an array of ray records (QUERY_RAY_DTYPE, RADIANCE_RAY_DTYPE or any
    record that starts with origin[3], direction[3]) → uint32 (n,): order[w] is the index of the ray to work on w-th.
    params=None takes RAY_ORDER_DEFAULTS; the stride is `stride`, else params', else the records' item size."""
    r = np.ascontiguousarray(rays)
    step = stride if stride is not None else params.ray_stride if params is not None else r.dtype.itemsize
    p = ray_order_params(stride=step) if params is None else F.rt_ray_order_params.from_buffer_copy(params)
    p.ray_stride = step
    if step <= 0 or r.nbytes % step:
        raise ValueError("the rays must hold whole records of `stride` bytes")
    n = r.nbytes // step
    order = np.zeros(n, dtype=np.uint32)
    F.check(F.lib().rt_ray_order(r.ctypes.data if n else None, n, C.byref(p), order.ctypes.data if n else None))
    return order


def ray_order_device(d_rays_ptr, n_rays, params, d_order_ptr, d_workspace_ptr, workspace_bytes, stream_ptr=None):
    """rt_ray_order_device: device pointers in (n_rays records params.ray_stride bytes apart and ray_order_workspace_bytes(n_rays)
    bytes of workspace, 16-byte aligned; room for n_rays uint32 entries), a pure enqueue on `stream_ptr` (hipStream_t as int):
    no host synchronisation. With torch: tensor.data_ptr() and torch.cuda.current_stream().cuda_stream."""
    F.check(F.lib().rt_ray_order_device(C.c_void_p(d_rays_ptr), n_rays, C.byref(params), C.c_void_p(d_order_ptr), C.c_void_p(d_workspace_ptr),
                                        workspace_bytes, C.c_void_p(stream_ptr or 0)))


def _ref(stats):
    """An optional rt_stats as the C calls take it: a reference, or a null pointer."""
    return C.byref(stats) if stats is not None else None


def _data(a):
    """An array's buffer as the C calls take it: its address, or a null pointer for an empty one."""
    return a.ctypes.data if a.size else None


def _feature_flags(counters, surfaces, specular):
    """The flag word of the six feature calls."""
    return (F.RT_FLAG_COUNTERS if counters else 0) | (F.RT_FLAG_SURFACES if surfaces else 0) | (F.RT_FLAG_SPECULAR if specular else 0)


class DeviceScene:
    """rt_scene: the flattened scene copied into HBM on the current HIP device."""

    def __init__(self, desc):
        self._h = C.c_void_p()
        F.check(F.lib().rt_scene_create(C.byref(desc), C.byref(self._h)))

    def info(self):
        need, blocks = C.c_uint32(), C.c_int32()
        F.check(F.lib().rt_debug_scene_info(self._h, C.byref(need), C.byref(blocks)))
        return {"stack_need": need.value, "grid_blocks": blocks.value}

    def trace_variant(self):
        """The traversal kernel variant timed renders of this scene take (rt_debug_trace_variant)."""
        wg, st, nc, sp = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        F.check(F.lib().rt_debug_trace_variant(self._h, C.byref(wg), C.byref(st), C.byref(nc), C.byref(sp)))
        return {"workgroup_threads": wg.value, "stack_entries": st.value, "nodes_in_lds": nc.value, "spheres_in_lds": bool(sp.value & 1),
                "f32_slabs": bool(sp.value & 2)}

    def child_order(self):
        """Whether the scene's traversal visits the nearer child of a BVH node first (bits 2 and 3 of rt_debug_trace_variant's last
        word): {"timed": the timed instance does, "counting": the counting instance does — never}."""
        sp = C.c_uint32()
        F.check(F.lib().rt_debug_trace_variant(self._h, None, None, None, C.byref(sp)))
        return {"timed": bool(sp.value & 4), "counting": bool(sp.value & 8)}

    def set_tuning(self, node_quorum=18 | (1 << 8) | (2 << 12) | (8 << 16) | (2 << 20) | (1 << 24), vote_weights=0):
        F.check(F.lib().rt_debug_set_tuning(self._h, node_quorum, vote_weights))

    def set_engine(self, engine, max_pool_blocks=0):
        """engine: "wavefront" (default) or "mega"."""
        F.check(F.lib().rt_debug_set_engine(self._h, {"mega": 0, "wavefront": 1}[engine], max_pool_blocks))

    def set_partial_ring(self, planes):
        """Planes of the partial-sum ring: 0 automatic, -1 never, n > 0 force (rt_debug_set_partial_ring)."""
        F.check(F.lib().rt_debug_set_partial_ring(self._h, planes))

    def pass_timing(self):
        """Probe of the last render made with tuning bit 29: dict of sums over the traversal passes (ms)."""
        o = (C.c_double * 5)()
        F.check(F.lib().rt_debug_pass_timing(self._h, o))
        return {"span_ms": o[0] / 1e5, "wave_life_ms": o[1] / 1e5, "wave_dry_ms": o[2] / 1e5, "passes": int(o[3]), "waves": int(o[4])}

    def census(self):
        """Scheduler census of the last counter run: {label: (rounds, lanes, utilisation)}."""
        r, l = (C.c_uint64 * 9)(), (C.c_uint64 * 9)()
        F.check(F.lib().rt_debug_census(self._h, r, l))
        names = ["node", "sphere", "rect", "box", "medium", "misc", "ctx", "done", "node_fast"]
        return {n: (r[i], l[i], (l[i] / (64.0 * r[i])) if r[i] else 0.0) for i, n in enumerate(names)}

    def render(self, cam, params, row_ids, want_stats=False, progress=None):
        """rt_render with host buffers → (n_rows, width, 3) float64 sums [, rt_stats].
        progress: a callable (worker, paths_done, paths_total), rt_params.progress_cb."""
        rows = np.ascontiguousarray(row_ids, dtype=np.uint32)
        p = F.rt_params.from_buffer_copy(params)
        p.n_rows = len(rows)
        p.row_ids = rows.ctypes.data
        if want_stats:
            p.flags |= F.RT_FLAG_COUNTERS
        if progress is not None:
            cb = F.PROGRESS_CB(lambda user, worker, done, total: progress(worker, done, total))      # (kept alive until the call returns)
            p.progress_cb = C.cast(cb, C.c_void_p).value
        out = np.empty((len(rows), p.width, 3), dtype=np.float64)
        st = F.rt_stats()
        F.check(F.lib().rt_render(self._h, C.byref(cam), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
        return (out, st) if want_stats else out

    def render_device(self, cam, params, d_row_ids_ptr, n_rows, d_out_ptr, stream_ptr=None, stats=None, asynchronous=False):
        """rt_render_device: device pointers in, enqueue on `stream_ptr` (hipStream_t as int). asynchronous=True sets
        RT_FLAG_ASYNC: the call returns at once, a host thread of the library drives the passes, wait() joins it."""
        p = F.rt_params.from_buffer_copy(params)
        p.n_rows = n_rows
        p.row_ids = d_row_ids_ptr
        if asynchronous:
            p.flags |= F.RT_FLAG_ASYNC
        F.check(F.lib().rt_render_device(self._h, C.byref(cam), C.byref(p), C.c_void_p(d_out_ptr),
                                         C.c_void_p(stream_ptr or 0), _ref(stats)))

    def wait(self, stream_ptr=None):
        F.check(F.lib().rt_render_wait(self._h, C.c_void_p(stream_ptr or 0)))

    def intersect(self, rays, any_hit=False, want_stats=False, order=None, order_params=None):
        """rt_intersect: closest hit (or, any_hit=True, the first accepted) of every ray of `rays` (QUERY_RAY_DTYPE, see
        query_rays) → array of HIT_DTYPE records [, rt_stats with the counters].
        order=None works the rays in the order given. order="auto" (rt_intersect_ordered) computes a coherence order first, with
        `order_params` (ray_order_params; None: RAY_ORDER_DEFAULTS): the same records, sooner for a shuffled batch of coherent rays
        on a heavy scene under a fine key such as ray_order_params(16, 6), later for rays that are coherent as they come and for
        bounce rays — so it is off by default. An index array is an order of
        the caller's: entry w names the ray worked on w-th; a ray that no entry names keeps a zeroed record."""
        r = np.ascontiguousarray(rays, dtype=F.QUERY_RAY_DTYPE)
        out = np.zeros(len(r), dtype=F.HIT_DTYPE)
        flags = (F.RT_FLAG_ANY_HIT if any_hit else 0) | (F.RT_FLAG_COUNTERS if want_stats else 0)
        st = F.rt_stats()
        p_rays, p_out = (r.ctypes.data, out.ctypes.data) if len(r) else (None, None)
        if order is None:
            F.check(F.lib().rt_intersect(self._h, p_rays, len(r), flags, p_out, C.byref(st)))
        elif isinstance(order, str):
            if order != "auto":
                raise ValueError('order must be None, "auto" or an index array')
            p = order_params if order_params is not None else ray_order_params()
            F.check(F.lib().rt_intersect_ordered(self._h, p_rays, None, C.byref(p), len(r), flags, p_out, C.byref(st)))
        else:
            o = np.ascontiguousarray(order, dtype=np.uint32)
            if o.shape != (len(r),):
                raise ValueError("an order holds one entry per ray")
            # (the parameters are ignored beside an order; they only keep an empty batch, whose order is no pointer, valid)
            F.check(F.lib().rt_intersect_ordered(self._h, p_rays, _data(o), C.byref(ray_order_params()), len(r), flags, p_out,
                                                 C.byref(st)))
        return (out, st) if want_stats else out

    def intersect_ordered_device(self, d_rays_ptr, d_order_ptr, n, d_hits_ptr, d_workspace_ptr, workspace_bytes, stream_ptr=None,
                                 any_hit=False, stats=None):
        """rt_intersect_ordered_device: intersect_device's work in the order of n uint32 entries at `d_order_ptr` (ray_order_device's,
        or any list: an entry >= n does nothing, a ray that no entry names keeps its record), through
        intersect_ordered_workspace_bytes(n) bytes of 16-byte aligned workspace. stats=None returns after the enqueue; an rt_stats
        makes the call synchronise the stream and fill it: rays counts the entries < n, ms covers gather, query and scatter."""
        flags = F.RT_FLAG_ANY_HIT if any_hit else 0
        if stats is not None:
            flags |= F.RT_FLAG_COUNTERS
        F.check(F.lib().rt_intersect_ordered_device(self._h, C.c_void_p(d_rays_ptr), C.c_void_p(d_order_ptr), n, flags, C.c_void_p(d_hits_ptr),
                                                    C.c_void_p(d_workspace_ptr), workspace_bytes, C.c_void_p(stream_ptr or 0),
                                                    _ref(stats)))

    def intersect_device(self, d_rays_ptr, n, d_hits_ptr, stream_ptr=None, any_hit=False, stats=None):
        """rt_intersect_device: device pointers in (n rt_query_ray records, room for n rt_hit), enqueued on `stream_ptr`
        (hipStream_t as int). stats=None returns after the enqueue, with no host synchronisation; an rt_stats makes the
        call synchronise the stream and fill it, counters included."""
        flags = F.RT_FLAG_ANY_HIT if any_hit else 0
        if stats is not None:
            flags |= F.RT_FLAG_COUNTERS
        F.check(F.lib().rt_intersect_device(self._h, C.c_void_p(d_rays_ptr), n, flags, C.c_void_p(d_hits_ptr),
                                            C.c_void_p(stream_ptr or 0), _ref(stats)))

    def radiance(self, rays, spp=1, background=(0.0, 0.0, 0.0), t_min=0.001, max_depth=50, want_stats=False, kernel_times=False):
        """rt_radiance: the sum over spp samples of ray_color for every ray of `rays` (RADIANCE_RAY_DTYPE, see radiance_rays)
        → (n, 3) float64 sums, not divided by spp [, rt_stats with the counters]."""
        r = np.ascontiguousarray(rays, dtype=F.RADIANCE_RAY_DTYPE)
        out = np.zeros((len(r), 3), dtype=np.float64)
        flags = (F.RT_FLAG_COUNTERS if want_stats else 0) | (F.RT_FLAG_KERNEL_TIMES if kernel_times else 0)
        p = radiance_params(spp, background, t_min, max_depth, flags)
        st = F.rt_stats()
        F.check(F.lib().rt_radiance(self._h, _data(r), len(r), C.byref(p), _data(out), C.byref(st)))
        return (out, st) if want_stats else out

    def radiance_device(self, d_rays_ptr, n, d_out_ptr, params, stream_ptr=None, stats=None):
        """rt_radiance_device: device pointers in (n rt_radiance_ray records, room for 3n doubles), `params` an
        rt_radiance_params (radiance_params), run on `stream_ptr` (hipStream_t as int); returns when the sums are written.
        An rt_stats is filled (its counters with RT_FLAG_COUNTERS in params.flags)."""
        F.check(F.lib().rt_radiance_device(self._h, C.c_void_p(d_rays_ptr), n, C.byref(params), C.c_void_p(d_out_ptr),
                                           C.c_void_p(stream_ptr or 0), _ref(stats)))

    def scatter(self, rays, hits, background=(0.0, 0.0, 0.0), t_min=0.001, prev=None, want_stats=False):
        """rt_scatter: one step of ray_color between two world.hit calls for every entry: `rays` (QUERY_RAY_DTYPE) and `hits`
        (HIT_DTYPE: intersect's records of those rays, or made-up ones) → (array of SCATTER_REC_DTYPE records, array of
        QUERY_RAY_DTYPE next rays, ready for intersect) [, rt_stats with rng_draws and light_pdf_tests]. prev: the records of
        the step before (an entry that was not live there is RT_SCATTER_ENDED); None: every entry is live."""
        r = np.ascontiguousarray(rays, dtype=F.QUERY_RAY_DTYPE)
        h = np.ascontiguousarray(hits, dtype=F.HIT_DTYPE)
        if h.shape != r.shape or r.ndim != 1:
            raise ValueError("one hit record per ray")
        pv = None
        if prev is not None:
            pv = np.ascontiguousarray(prev, dtype=F.SCATTER_REC_DTYPE)
            if pv.shape != r.shape:
                raise ValueError("one previous record per ray")
        recs = np.zeros(len(r), dtype=F.SCATTER_REC_DTYPE)
        nxt = np.zeros(len(r), dtype=F.QUERY_RAY_DTYPE)
        p = scatter_params(background, t_min, F.RT_FLAG_COUNTERS if want_stats else 0)
        st = F.rt_stats()
        F.check(F.lib().rt_scatter(self._h, _data(r), _data(h), _data(pv) if pv is not None else None, len(r), C.byref(p), _data(recs),
                                   _data(nxt), C.byref(st)))
        return (recs, nxt, st) if want_stats else (recs, nxt)

    def scatter_device(self, d_rays_ptr, d_hits_ptr, n, d_recs_ptr, d_next_rays_ptr, params, d_prev_ptr=None, stream_ptr=None, stats=None):
        """rt_scatter_device: device pointers in (n rt_query_ray and n rt_hit records, optionally n rt_scatter_rec of the step
        before; room for n rt_scatter_rec and n rt_query_ray — the next rays may be the rays, the records `prev`), `params` an
        rt_scatter_params (scatter_params), enqueued on `stream_ptr` (hipStream_t as int). stats=None returns after the enqueue;
        an rt_stats makes the call synchronise the stream and fill it (its counters with RT_FLAG_COUNTERS in params.flags)."""
        F.check(F.lib().rt_scatter_device(self._h, C.c_void_p(d_rays_ptr), C.c_void_p(d_hits_ptr), C.c_void_p(d_prev_ptr or 0), n,
                                          C.byref(params), C.c_void_p(d_recs_ptr), C.c_void_p(d_next_rays_ptr),
                                          C.c_void_p(stream_ptr or 0), _ref(stats)))

    def render_pixels(self, cam, params, ids, want_stats=False, kernel_times=False):
        """rt_render_pixels with host buffers: the render's sums of a list of (frame, pixel) ids (uint64, see pixel_ids; params.n_frames
        must exceed every frame) → (n, 3) float64 [, rt_stats with the counters]. n_rows, row_ids and progress_cb are ignored."""
        e = np.ascontiguousarray(ids, dtype=np.uint64).ravel()
        p = F.rt_params.from_buffer_copy(params)
        p.n_rows, p.row_ids, p.progress_cb = 0, None, None
        p.flags = (p.flags & (F.RT_FLAG_COUNTERS | F.RT_FLAG_KERNEL_TIMES)) | (F.RT_FLAG_COUNTERS if want_stats else 0) | \
                  (F.RT_FLAG_KERNEL_TIMES if kernel_times else 0)
        out = np.zeros((len(e), 3), dtype=np.float64)
        st = F.rt_stats()
        F.check(F.lib().rt_render_pixels(self._h, C.byref(cam), C.byref(p), _data(e), len(e), _data(out), C.byref(st)))
        return (out, st) if want_stats else out

    def render_pixels_device(self, cam, params, d_ids_ptr, n_entries, d_out_ptr, stream_ptr=None, stats=None):
        """rt_render_pixels_device: device pointers in (n_entries uint64 ids, 8-byte aligned; room for 3 * n_entries doubles,
        16-byte aligned), run on `stream_ptr` (hipStream_t as int); returns when the sums are written. An rt_stats is filled
        (its counters with RT_FLAG_COUNTERS in params.flags)."""
        p = F.rt_params.from_buffer_copy(params)
        p.n_rows, p.row_ids, p.progress_cb = 0, None, None
        F.check(F.lib().rt_render_pixels_device(self._h, C.byref(cam), C.byref(p), C.c_void_p(d_ids_ptr), n_entries, C.c_void_p(d_out_ptr),
                                                C.c_void_p(stream_ptr or 0), _ref(stats)))

    def features(self, cam, params, row_ids, want_stats=False, surfaces=False, specular=False):
        """rt_features with host buffers: the first-hit guide buffers of the camera rays a render of (cam, params, row_ids)
        shoots → array of FEATURE_DTYPE records of shape (n_rows, width) — fields albedo (3), normal (3), depth, hits: sums
        over the spp samples, not divided by spp [, rt_stats]. params.max_depth, spp_chunk and progress_cb are ignored.
        surfaces=True sets RT_FLAG_SURFACES (here and in the three forms below): a ConstantMedium is looked through, the
        records are those of the first SURFACE behind it. specular=True sets RT_FLAG_SPECULAR (likewise): the sample's own path is
        followed through glass and fuzz-0 mirrors (at most RT_FEATURE_SPECULAR_BOUNCES vertices), albedo and normal are those of
        the first non-specular vertex with the followed metals' albedos multiplied on, depth and hits stay the first hit's; rt_stats.rays
        then counts every segment (with counters; 0 without). For the denoisers, not for the temporal accumulation."""
        rows = np.ascontiguousarray(row_ids, dtype=np.uint32)
        p = F.rt_params.from_buffer_copy(params)
        p.n_rows = len(rows)
        p.row_ids = rows.ctypes.data
        p.progress_cb = None
        p.flags = _feature_flags(want_stats, surfaces, specular)
        out = np.zeros((len(rows), p.width), dtype=F.FEATURE_DTYPE)
        st = F.rt_stats()
        F.check(F.lib().rt_features(self._h, C.byref(cam), C.byref(p), _data(out), C.byref(st)))
        return (out, st) if want_stats else out

    def features_device(self, cam, params, d_row_ids_ptr, n_rows, d_out_ptr, stream_ptr=None, stats=None, surfaces=False, specular=False):
        """rt_features_device: device pointers in (n_rows row ids, room for n_rows * width rt_feature records, 16-byte
        aligned), enqueued on `stream_ptr` (hipStream_t as int). stats=None returns once the kernel is enqueued; an rt_stats
        makes the call synchronise the stream and fill it, counters included."""
        p = F.rt_params.from_buffer_copy(params)
        p.n_rows = n_rows
        p.row_ids = d_row_ids_ptr
        p.progress_cb = None
        p.flags = _feature_flags(stats is not None, surfaces, specular)
        F.check(F.lib().rt_features_device(self._h, C.byref(cam), C.byref(p), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0),
                                           _ref(stats)))

    def features_pixels(self, cam, params, ids, want_stats=False, surfaces=False, specular=False):
        """rt_features_pixels with host buffers: the feature records of a list of (frame, pixel) ids (uint64, see pixel_ids;
        params.n_frames must exceed every frame) → (n,) array of FEATURE_DTYPE records, each the record features() gives that
        pixel of that frame [, rt_stats]. n_rows, row_ids, max_depth, spp_chunk and progress_cb are ignored."""
        e = np.ascontiguousarray(ids, dtype=np.uint64).ravel()
        p = F.rt_params.from_buffer_copy(params)
        p.n_rows, p.row_ids, p.progress_cb = 0, None, None
        p.flags = _feature_flags(want_stats, surfaces, specular)
        out = np.zeros(len(e), dtype=F.FEATURE_DTYPE)
        st = F.rt_stats()
        F.check(F.lib().rt_features_pixels(self._h, C.byref(cam), C.byref(p), _data(e), len(e), _data(out), C.byref(st)))
        return (out, st) if want_stats else out

    def features_pixels_device(self, cam, params, d_ids_ptr, n_entries, d_out_ptr, stream_ptr=None, stats=None, surfaces=False, specular=False):
        """rt_features_pixels_device: device pointers in (n_entries uint64 ids, 8-byte aligned; room for n_entries rt_feature
        records, 16-byte aligned), enqueued on `stream_ptr` (hipStream_t as int) behind the range check of the ids (one
        synchronisation of the stream). stats=None returns once the kernel is enqueued; an rt_stats makes the call
        synchronise the stream and fill it, counters included."""
        p = F.rt_params.from_buffer_copy(params)
        p.n_rows, p.row_ids, p.progress_cb = 0, None, None
        p.flags = _feature_flags(stats is not None, surfaces, specular)
        F.check(F.lib().rt_features_pixels_device(self._h, C.byref(cam), C.byref(p), C.c_void_p(d_ids_ptr), n_entries, C.c_void_p(d_out_ptr),
                                                  C.c_void_p(stream_ptr or 0), _ref(stats)))

    def features_rays(self, rays, spp=1, background=(0.0, 0.0, 0.0), t_min=0.001, want_stats=False, surfaces=False, specular=False):
        """rt_features_rays with host buffers: the feature records of rays the caller chooses (RADIANCE_RAY_DTYPE, see
        radiance_rays — the buffer radiance() takes) → (n,) array of FEATURE_DTYPE records: sums over the spp samples of ray i,
        sample s drawing from path_key(rng_state, 0, 0, s) as radiance()'s does, not divided by spp [, rt_stats]. surfaces and
        specular as for features(). What rt.denoise needs beside radiance()'s sums of a camera of the caller's own."""
        r = np.ascontiguousarray(rays, dtype=F.RADIANCE_RAY_DTYPE)
        flags = _feature_flags(want_stats, surfaces, specular)
        p = radiance_params(spp, background, t_min, 0, flags)
        out = np.zeros(len(r), dtype=F.FEATURE_DTYPE)
        st = F.rt_stats()
        F.check(F.lib().rt_features_rays(self._h, _data(r), len(r), C.byref(p), _data(out), C.byref(st)))
        return (out, st) if want_stats else out

    def features_rays_device(self, d_rays_ptr, n, d_out_ptr, params, stream_ptr=None, stats=None, surfaces=False, specular=False):
        """rt_features_rays_device: device pointers in (n rt_radiance_ray records, room for n rt_feature records, both 16-byte
        aligned), `params` an rt_radiance_params (radiance_params; its max_depth is ignored, its flags are replaced), enqueued on
        `stream_ptr` (hipStream_t as int). stats=None is a pure enqueue with no host synchronisation; an rt_stats makes the call
        synchronise the stream and fill it, counters included."""
        p = F.rt_radiance_params.from_buffer_copy(params)
        p.flags = _feature_flags(stats is not None, surfaces, specular)
        F.check(F.lib().rt_features_rays_device(self._h, C.c_void_p(d_rays_ptr), n, C.byref(p), C.c_void_p(d_out_ptr),
                                                C.c_void_p(stream_ptr or 0), _ref(stats)))

    def close(self):
        if self._h:
            F.lib().rt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceSceneSet:
    """rt_scene_set: a copy of the scene on every device of `device_mask`, rendered by ONE call (rt_render_multi)."""

    def __init__(self, desc, device_mask=1):
        self._h = C.c_void_p()
        F.check(F.lib().rt_scene_set_create(C.byref(desc), device_mask, C.byref(self._h)))

    def render(self, cam, params, row_ids, want_stats=False, progress=None):
        rows = np.ascontiguousarray(row_ids, dtype=np.uint32)
        p = F.rt_params.from_buffer_copy(params)
        p.n_rows = len(rows)
        p.row_ids = rows.ctypes.data
        if want_stats:
            p.flags |= F.RT_FLAG_COUNTERS
        if progress is not None:                     # (called from the devices' host threads, concurrently: ctypes takes the GIL for each call)
            cb = F.PROGRESS_CB(lambda user, worker, done, total: progress(worker, done, total))
            p.progress_cb = C.cast(cb, C.c_void_p).value
        out = np.empty((len(rows), p.width, 3), dtype=np.float64)
        st = F.rt_stats()
        F.check(F.lib().rt_render_multi(self._h, C.byref(cam), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st)))
        return (out, st) if want_stats else out

    def close(self):
        if self._h:
            F.lib().rt_scene_set_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
