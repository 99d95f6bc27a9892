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


def denoise(rgb_sum, features, params, row_ids=None, want_ms=False):
    """rt_denoise with host buffers: a render's sums (height, width, 3) and its FEATURE_DTYPE records (height, width), both
    in the order of `row_ids` (None: image order; else the frame's row list, a permutation of the image's rows) -> the
    filtered sums, same shape and order [, device ms]."""
    s = np.ascontiguousarray(rgb_sum, dtype=np.float64)
    f = np.ascontiguousarray(features, dtype=F.FEATURE_DTYPE)
    n = params.width * params.height
    if s.size != 3 * n or f.size != n:
        raise ValueError("rgb_sum and features must hold width * height pixels")
    rows = None
    if row_ids is not None:
        rows = np.ascontiguousarray(row_ids, dtype=np.uint32)
        if rows.size != params.height:
            raise ValueError("row_ids must hold one entry per image row")
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
    n = params.width * params.height
    s = [np.ascontiguousarray(x, dtype=np.float64) for x in (sum_a, sum_b)]
    f = [np.ascontiguousarray(x, dtype=F.FEATURE_DTYPE) for x in (feat_a, feat_b)]
    if any(x.size != 3 * n for x in s) or any(x.size != n for x in f):
        raise ValueError("both halves' rgb_sum and features must hold width * height pixels")
    rows = None
    if row_ids is not None:
        rows = np.ascontiguousarray(row_ids, dtype=np.uint32)
        if rows.size != params.height:
            raise ValueError("row_ids must hold one entry per image row")
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
                                         C.c_void_p(stream_ptr or 0), C.byref(stats) if stats is not None else None))

    def wait(self, stream_ptr=None):
        F.check(F.lib().rt_render_wait(self._h, C.c_void_p(stream_ptr or 0)))

    def intersect(self, rays, any_hit=False, want_stats=False):
        """rt_intersect: closest hit (or, any_hit=True, the first accepted) of every ray of `rays` (QUERY_RAY_DTYPE, see
        query_rays) → array of HIT_DTYPE records [, rt_stats with the counters]."""
        r = np.ascontiguousarray(rays, dtype=F.QUERY_RAY_DTYPE)
        out = np.zeros(len(r), dtype=F.HIT_DTYPE)
        flags = (F.RT_FLAG_ANY_HIT if any_hit else 0) | (F.RT_FLAG_COUNTERS if want_stats else 0)
        st = F.rt_stats()
        F.check(F.lib().rt_intersect(self._h, r.ctypes.data if len(r) else None, len(r), flags, out.ctypes.data if len(r) else None,
                                     C.byref(st)))
        return (out, st) if want_stats else out

    def intersect_device(self, d_rays_ptr, n, d_hits_ptr, stream_ptr=None, any_hit=False, stats=None):
        """rt_intersect_device: device pointers in (n rt_query_ray records, room for n rt_hit), enqueued on `stream_ptr`
        (hipStream_t as int). stats=None returns after the enqueue, with no host synchronisation; an rt_stats makes the
        call synchronise the stream and fill it, counters included."""
        flags = F.RT_FLAG_ANY_HIT if any_hit else 0
        if stats is not None:
            flags |= F.RT_FLAG_COUNTERS
        F.check(F.lib().rt_intersect_device(self._h, C.c_void_p(d_rays_ptr), n, flags, C.c_void_p(d_hits_ptr),
                                            C.c_void_p(stream_ptr or 0), C.byref(stats) if stats is not None else None))

    def radiance(self, rays, spp=1, background=(0.0, 0.0, 0.0), t_min=0.001, max_depth=50, want_stats=False, kernel_times=False):
        """rt_radiance: the sum over spp samples of ray_color for every ray of `rays` (RADIANCE_RAY_DTYPE, see radiance_rays)
        → (n, 3) float64 sums, not divided by spp [, rt_stats with the counters]."""
        r = np.ascontiguousarray(rays, dtype=F.RADIANCE_RAY_DTYPE)
        out = np.zeros((len(r), 3), dtype=np.float64)
        flags = (F.RT_FLAG_COUNTERS if want_stats else 0) | (F.RT_FLAG_KERNEL_TIMES if kernel_times else 0)
        p = radiance_params(spp, background, t_min, max_depth, flags)
        st = F.rt_stats()
        F.check(F.lib().rt_radiance(self._h, r.ctypes.data if len(r) else None, len(r), C.byref(p), out.ctypes.data if len(r) else None,
                                    C.byref(st)))
        return (out, st) if want_stats else out

    def radiance_device(self, d_rays_ptr, n, d_out_ptr, params, stream_ptr=None, stats=None):
        """rt_radiance_device: device pointers in (n rt_radiance_ray records, room for 3n doubles), `params` an
        rt_radiance_params (radiance_params), run on `stream_ptr` (hipStream_t as int); returns when the sums are written.
        An rt_stats is filled (its counters with RT_FLAG_COUNTERS in params.flags)."""
        F.check(F.lib().rt_radiance_device(self._h, C.c_void_p(d_rays_ptr), n, C.byref(params), C.c_void_p(d_out_ptr),
                                           C.c_void_p(stream_ptr or 0), C.byref(stats) if stats is not None else None))

    def features(self, cam, params, row_ids, want_stats=False):
        """rt_features with host buffers: the first-hit guide buffers of the camera rays a render of (cam, params, row_ids)
        shoots → array of FEATURE_DTYPE records of shape (n_rows, width) — fields albedo (3), normal (3), depth, hits: sums
        over the spp samples, not divided by spp [, rt_stats]. params.max_depth, spp_chunk and progress_cb are ignored."""
        rows = np.ascontiguousarray(row_ids, dtype=np.uint32)
        p = F.rt_params.from_buffer_copy(params)
        p.n_rows = len(rows)
        p.row_ids = rows.ctypes.data
        p.progress_cb = None
        p.flags = F.RT_FLAG_COUNTERS if want_stats else 0
        out = np.zeros((len(rows), p.width), dtype=F.FEATURE_DTYPE)
        st = F.rt_stats()
        F.check(F.lib().rt_features(self._h, C.byref(cam), C.byref(p), out.ctypes.data if out.size else None, C.byref(st)))
        return (out, st) if want_stats else out

    def features_device(self, cam, params, d_row_ids_ptr, n_rows, d_out_ptr, stream_ptr=None, stats=None):
        """rt_features_device: device pointers in (n_rows row ids, room for n_rows * width rt_feature records, 16-byte
        aligned), enqueued on `stream_ptr` (hipStream_t as int). stats=None returns once the kernel is enqueued; an rt_stats
        makes the call synchronise the stream and fill it, counters included."""
        p = F.rt_params.from_buffer_copy(params)
        p.n_rows = n_rows
        p.row_ids = d_row_ids_ptr
        p.progress_cb = None
        p.flags = F.RT_FLAG_COUNTERS if stats is not None else 0
        F.check(F.lib().rt_features_device(self._h, C.byref(cam), C.byref(p), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr or 0),
                                           C.byref(stats) if stats is not None else None))

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
