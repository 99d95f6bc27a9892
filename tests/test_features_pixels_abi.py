"""Pixel-list feature buffers (rt_features_pixels*) and the feature merge / resolve (rt_adaptive_*_features_device): the
bindings, argument checking and the numpy restatement. No compute calls: runs without a GPU (every RT_ERR_INVALID case
returns before any device call, with or without a scene)."""
import ctypes as C
import os
import re

import numpy as np

import adaptive_features_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_features_pixels", "rt_features_pixels_device", "rt_adaptive_merge_features_device", "rt_adaptive_resolve_features_device"]


def test_symbols_are_exported_bound_and_declared(rt):
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    for sym in NEW:
        assert sym in F.ABI_SYMBOLS and getattr(L, sym).argtypes, sym
    assert L.rt_abi_version() == 3 and F.RT2022_ABI_VERSION == 3
    text = open(os.path.join(ROOT, "include", "rt2022.h")).read()
    assert "#define RT2022_ABI_VERSION 3" in text
    for sym in NEW:
        assert re.search(r"\nint %s\(" % sym, text), sym
    for name in ("features_pixels", "features_pixels_device"):
        assert callable(getattr(rt.DeviceScene, name))
    assert callable(rt.adaptive_merge_features_device) and callable(rt.adaptive_resolve_features_device)


def test_pixel_list_arguments_are_checked_before_the_device(rt):
    """Every RT_ERR_INVALID case of the two entry points, with its message, and the two RT_OK cases that need no device."""
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    cam = rt.camera_new((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 5.0, 0.0, 1.0)
    ids = rt.pixel_ids(0, [0, 1, 2, 3], [3, 2, 1, 0], 4, 4)
    out = np.full(4 * 8, 7.0)
    st = F.rt_stats()

    def params(**kw):
        p = rt.make_params(4, 4, 2, 50, (0.1, 0.2, 0.3), seed=1)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def host(p, cam_=cam, ids_=ids.ctypes.data, n=4, out_=out.ctypes.data, scene=None):
        return L.rt_features_pixels(scene, C.byref(cam_) if cam_ is not None else None, C.byref(p) if p is not None else None, ids_, n, out_,
                                    C.byref(st))

    def device(p, cam_=cam, ids_=4096, n=4, out_=8192, scene=None):
        return L.rt_features_pixels_device(scene, C.byref(cam_) if cam_ is not None else None, C.byref(p) if p is not None else None, ids_, n,
                                           out_, None, None)

    err = lambda: L.rt_last_error().decode()
    # a null scene, cam or params
    assert host(params()) == F.RT_ERR_INVALID and err() == "rt_features_pixels: null scene"
    assert device(params()) == F.RT_ERR_INVALID and err() == "rt_features_pixels_device: null scene"
    assert host(params(), cam_=None) == F.RT_ERR_INVALID and "null camera" in err()
    assert device(params(), cam_=None) == F.RT_ERR_INVALID and "null camera" in err()
    assert host(None) == F.RT_ERR_INVALID and "null params" in err()
    assert device(None) == F.RT_ERR_INVALID and "null params" in err()
    assert L.rt_features_pixels(None, None, None, None, 0, None, None) == F.RT_ERR_INVALID and err()
    assert L.rt_features_pixels_device(None, None, None, None, 0, None, None, None) == F.RT_ERR_INVALID and err()
    # null ids or output with n_entries > 0 ... and with none they are not looked at
    for f in (host, device):
        assert f(params(), ids_=None) == F.RT_ERR_INVALID and "null id or output buffer" in err()
        assert f(params(), out_=None) == F.RT_ERR_INVALID and "null id or output buffer" in err()
        assert f(params(), ids_=None, out_=None, n=0) == F.RT_ERR_INVALID and "null scene" in err()
    # width, height or n_frames equal to 0; a closed shutter
    shut = rt.camera_new((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 5.0, 1.0, 1.0)
    for f in (host, device):
        for field in ("width", "height", "n_frames"):
            assert f(params(**{field: 0})) == F.RT_ERR_INVALID and "empty image" in err(), field
        assert f(params(), cam_=shut) == F.RT_ERR_INVALID and "time0 >= time1" in err()
        # a flag bit other than RT_FLAG_COUNTERS
        for bad in (F.RT_FLAG_KERNEL_TIMES, F.RT_FLAG_ASYNC, F.RT_FLAG_ANY_HIT, 0x100, F.RT_FLAG_COUNTERS | F.RT_FLAG_ASYNC):
            assert f(params(flags=bad)) == F.RT_ERR_INVALID and "flag bits" in err()
        assert f(params(flags=F.RT_FLAG_COUNTERS)) == F.RT_ERR_INVALID and "null scene" in err()
        # n_entries > 2^40 (the ids are not read: the length is refused first)
        assert f(params(), n=(1 << 40) + 1, **({"ids_": 4096, "out_": 8192} if f is host else {})) == F.RT_ERR_INVALID and "n_entries too large" in err()
    # device ids not 8-byte aligned, a device output not 16-byte aligned
    for off in (1, 2, 4):
        assert device(params(), ids_=4096 + off) == F.RT_ERR_INVALID and "8-byte aligned" in err()
    for off in (1, 4, 8):
        assert device(params(), out_=8192 + off) == F.RT_ERR_INVALID and "16-byte aligned" in err()
    assert device(params(), ids_=4096 + 8, out_=8192 + 16) == F.RT_ERR_INVALID and "null scene" in err()
    # an id >= width * height * n_frames (host ids: checked on the host; device ids need the device)
    bad = ids.copy()
    bad[2] = 16
    assert host(params(), ids_=bad.ctypes.data) == F.RT_ERR_INVALID and "pixel id out of range" in err()
    assert host(params(n_frames=2), ids_=bad.ctypes.data) == F.RT_ERR_INVALID and "null scene" in err()
    bad[2] = 32
    assert host(params(n_frames=2), ids_=bad.ctypes.data) == F.RT_ERR_INVALID and "pixel id out of range" in err()
    bad[2] = (1 << 64) - 1
    assert host(params(n_frames=0xFFFFFFFF // 4), ids_=bad.ctypes.data) == F.RT_ERR_INVALID and "pixel id out of range" in err()
    # ignored fields are ignored
    rows = np.arange(4, dtype=np.uint32)
    assert host(params(max_depth=0, spp_chunk=7, progress_cb=1234, n_rows=99, row_ids=rows.ctypes.data)) == F.RT_ERR_INVALID and "null scene" in err()
    assert np.all(out == 7.0)                                                   # nothing was written


def test_no_entries_and_no_samples_need_no_device(rt):
    """n_entries == 0 is RT_OK; spp == 0 is RT_OK with zeros (host form: no device call at all, so a scene that is only a
    non-null handle will do — it is never dereferenced on these paths)."""
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    cam = rt.camera_new((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 5.0, 0.0, 1.0)
    handle = C.create_string_buffer(4096)                                       # (stands in for a scene: not touched)
    scene = C.cast(handle, C.c_void_p)
    ids = rt.pixel_ids(0, [0, 1, 2], [3, 2, 1], 4, 4)
    out = np.full(3 * 8, 7.0)
    st = F.rt_stats()
    st.paths = st.rays = 99
    p = rt.make_params(4, 4, 2, 50, (0.1, 0.2, 0.3), seed=1)
    assert L.rt_features_pixels(scene, C.byref(cam), C.byref(p), None, 0, None, C.byref(st)) == F.RT_OK
    assert st.paths == 0 and st.rays == 0 and np.all(out == 7.0)
    assert L.rt_features_pixels_device(scene, C.byref(cam), C.byref(p), None, 0, None, None, None) == F.RT_OK
    p.spp = 0
    st.paths = st.rays = 99
    assert L.rt_features_pixels(scene, C.byref(cam), C.byref(p), ids.ctypes.data, 3, out.ctypes.data, C.byref(st)) == F.RT_OK
    assert st.paths == 0 and st.rays == 0 and st.ms == 0 and not out.view(np.uint8).any()
    ids[1] = 16                                                                 # ... but a bad id is still a bad id
    assert L.rt_features_pixels(scene, C.byref(cam), C.byref(p), ids.ctypes.data, 3, out.ctypes.data, None) == F.RT_ERR_INVALID


def test_feature_merge_and_resolve_arguments(rt):
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    err = lambda: L.rt_last_error().decode()
    M, Rz = L.rt_adaptive_merge_features_device, L.rt_adaptive_resolve_features_device
    assert M(None, None, None, 0, None, None) == F.RT_OK and Rz(None, None, 0, 1, None, None) == F.RT_OK
    big = (1 << 36) + 1
    assert M(4096, 8192, 12288, big, 16384, None) == F.RT_ERR_INVALID and "RT_DENOISE_MAX_PIXELS" in err()
    assert err().startswith("rt_adaptive_merge_features_device: ")
    assert Rz(4096, 8192, big, 1, 12288, None) == F.RT_ERR_INVALID and "RT_DENOISE_MAX_PIXELS" in err()
    assert err().startswith("rt_adaptive_resolve_features_device: ")
    want = ["16-byte aligned", "4-byte aligned", "8-byte aligned", "16-byte aligned"]       # entries, units, offsets, acc
    for k in range(4):
        a = [4096, 8192, 12288, 16384]
        a[k] = None
        assert M(a[0], a[1], a[2], 4, a[3], None) == F.RT_ERR_INVALID and "null buffer" in err(), k
        for off in ((8, 4) if k in (0, 3) else (2,) if k == 1 else (4,)):
            a[k] = 4096 * (k + 1) + off
            assert M(a[0], a[1], a[2], 4, a[3], None) == F.RT_ERR_INVALID and want[k] in err(), (k, off)
    want = ["16-byte aligned", "8-byte aligned", "16-byte aligned"]                          # acc, acc_n, out
    for k in range(3):
        a = [4096, 8192, 12288]
        a[k] = None
        assert Rz(a[0], a[1], 4, 1, a[2], None) == F.RT_ERR_INVALID and "null buffer" in err(), k
        for off in ((8, 4) if k != 1 else (4,)):
            a[k] = 4096 * (k + 1) + off
            assert Rz(a[0], a[1], 4, 1, a[2], None) == F.RT_ERR_INVALID and want[k] in err(), (k, off)


def test_restatement_agrees_with_a_plain_loop():
    """adaptive_features_ref on a 3 x 2 image against Python floats (IEEE doubles) added one at a time."""
    g = np.random.default_rng(5)
    n = 6
    units = np.array([2, 0, 1, 3, 0, 1], dtype=np.uint32)
    offsets = np.concatenate([[0], np.cumsum(units)]).astype(np.uint64)
    E = g.normal(size=(int(units.sum()), 8)) * 3.0
    E[1, 2] = np.nan
    E[4, 6] = np.inf
    acc = g.random((n, 8))
    acc_n = np.array([4.0, 4.0, 8.0, 0.0, 0.0, 4.0])
    want = [[float(v) for v in row] for row in acc]
    for b in range(n):
        for k in range(int(units[b])):
            for f in range(8):
                want[b][f] = want[b][f] + float(E[int(offsets[b]) + k, f])
    got = acc.copy()
    FR.merge(E, units, offsets, got)
    same = lambda a, b: np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a, nan=0.0).view(np.uint64),
                                                                                     np.nan_to_num(b, nan=0.0).view(np.uint64))
    assert same(got, np.array(want))
    assert np.array_equal(got[[1, 4]].view(np.uint64), acc[[1, 4]].view(np.uint64))         # 0 units: untouched
    res = FR.resolve(got, acc_n, 16)
    loop = np.empty((n, 8))
    for b in range(n):
        for f in range(8):
            d = float(acc_n[b])
            q = want[b][f] / d if d != 0.0 else (float("nan") if want[b][f] == 0.0 or want[b][f] != want[b][f] else
                                                 float("inf") if want[b][f] > 0 else float("-inf"))
            loop[b, f] = q * 16.0
    assert same(res, loop)
    assert np.isfinite(res[1]).all()                                            # a pixel with samples and no units
    assert not np.isfinite(res[3]).any() and not np.isfinite(res[4]).any()
