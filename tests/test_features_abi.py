"""First-hit feature buffers (rt_features*): the record layout, the bindings and argument checking. No compute calls:
runs without a GPU (every RT_ERR_INVALID case returns before any device call, with or without a scene)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_feature_record_layout_bindings_and_library_agree(rt):
    from raytracer_2022_amd import _ffi as F
    assert C.sizeof(F.rt_feature) == 64 and F.FEATURE_DTYPE.itemsize == 64 and rt.FEATURE_DTYPE is F.FEATURE_DTYPE
    out = (C.c_uint32 * 8)()
    n = rt.lib().rtb_features_abi_sizes(out, 8)
    assert n == len(F.FEATURES_ABI_STRUCTS) == 1
    assert [out[i] for i in range(n)] == [C.sizeof(t) for t in F.FEATURES_ABI_STRUCTS] == [64]
    assert rt.lib().rtb_features_abi_sizes(out, 0) == 1                      # (a size query writes nothing)
    offsets = {"albedo": 0, "normal": 24, "depth": 48, "hits": 56}
    assert [f[0] for f in F.rt_feature._fields_] == list(offsets) == list(F.FEATURE_DTYPE.names)
    for name, off in offsets.items():
        assert getattr(F.rt_feature, name).offset == off, name
        assert F.FEATURE_DTYPE.fields[name][1] == off, name
    # the general lists stay as they were, the ABI version too
    assert F.rt_feature not in F.ABI_STRUCTS and F.rt_feature not in F.RADIANCE_ABI_STRUCTS
    assert rt.lib().rt_abi_version() == 3
    # a numpy record and a ctypes record are the same bytes
    r = np.zeros(1, dtype=F.FEATURE_DTYPE)
    r["albedo"], r["normal"], r["depth"], r["hits"] = (1, 2, 3), (4, 5, 6), 7, 8
    c = F.rt_feature.from_buffer_copy(r.tobytes())
    assert list(c.albedo) == [1, 2, 3] and list(c.normal) == [4, 5, 6] and (c.depth, c.hits) == (7, 8)


def test_header_declares_the_record_the_bindings_mirror():
    """include/rt2022.h: the struct's fields in the bindings' order, all doubles, and both entry points."""
    text = open(os.path.join(ROOT, "include", "rt2022.h")).read()
    m = re.search(r"typedef struct rt_feature \{(.*?)\} rt_feature;", text, flags=re.S)
    assert m, "rt_feature is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"double\s+(\w+)(?:\[(\d)\])?;", body)
    assert fields == [("albedo", "3"), ("normal", "3"), ("depth", ""), ("hits", "")]
    assert re.search(r"int rt_features\(rt_scene \*scene, const rt_camera \*cam, const rt_params \*params,\s*rt_feature \*out_features, rt_stats \*stats\);", text)
    assert re.search(r"int rt_features_device\(rt_scene \*scene, const rt_camera \*cam, const rt_params \*params,\s*rt_feature \*d_out_features, void \*hip_stream, rt_stats \*stats\);", text)
    assert "#define RT2022_ABI_VERSION 3" in text


def test_feature_arguments_are_checked_before_the_device(rt):
    """Every RT_ERR_INVALID case of the two entry points, each with its own message — on a machine without a GPU too: the
    arguments are looked at before the scene, and the scene pointer is never dereferenced on the way."""
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    cam = rt.camera_new((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 5.0, 0.0, 1.0)
    rows = np.arange(4, dtype=np.uint32)
    out = np.zeros((4, 4), dtype=F.FEATURE_DTYPE)
    st = F.rt_stats()

    def params(**kw):
        p = rt.make_params(4, 4, 2, 50, (0.1, 0.2, 0.3), seed=1)
        p.n_rows, p.row_ids = 4, rows.ctypes.data
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def host(p, cam_=cam, out_=out.ctypes.data, scene=None):
        return L.rt_features(scene, C.byref(cam_) if cam_ is not None else None, C.byref(p) if p is not None else None, out_, C.byref(st))

    def device(p, cam_=cam, out_=8192, scene=None):
        return L.rt_features_device(scene, C.byref(cam_) if cam_ is not None else None, C.byref(p) if p is not None else None, out_, None, None)

    def device_params(**kw):
        kw.setdefault("row_ids", 4096)
        return params(**kw)

    err = lambda: L.rt_last_error().decode()
    # a null scene, cam or params
    assert host(params()) == F.RT_ERR_INVALID and "rt_features: null scene" in err()
    assert device(device_params()) == F.RT_ERR_INVALID and "rt_features_device: null scene" in err()
    assert host(params(), cam_=None) == F.RT_ERR_INVALID and "null camera" in err()
    assert device(device_params(), cam_=None) == F.RT_ERR_INVALID and "null camera" in err()
    assert host(None) == F.RT_ERR_INVALID and "null params" in err()
    assert device(None) == F.RT_ERR_INVALID and "null params" in err()
    assert L.rt_features(None, None, None, None, None) == F.RT_ERR_INVALID
    assert L.rt_features_device(None, None, None, None, None, None) == F.RT_ERR_INVALID
    # null rows or output with work to do
    assert host(params(row_ids=None)) == F.RT_ERR_INVALID and "null row_ids" in err()
    assert device(device_params(row_ids=None)) == F.RT_ERR_INVALID and "null row_ids" in err()
    assert host(params(), out_=None) == F.RT_ERR_INVALID and "null output" in err()
    assert device(device_params(), out_=None) == F.RT_ERR_INVALID and "null output" in err()
    # ... and without work they are not looked at: the call goes on to the scene check
    assert host(params(n_rows=0, row_ids=None), out_=None) == F.RT_ERR_INVALID and "null scene" in err()
    assert device(device_params(n_rows=0, row_ids=None), out_=None) == F.RT_ERR_INVALID and "null scene" in err()
    assert host(params(spp=0, row_ids=None)) == F.RT_ERR_INVALID and "null scene" in err()
    # a flag other than RT_FLAG_COUNTERS
    for bad in (F.RT_FLAG_KERNEL_TIMES, F.RT_FLAG_ASYNC, F.RT_FLAG_ANY_HIT, 0x100, F.RT_FLAG_COUNTERS | F.RT_FLAG_ASYNC):
        assert host(params(flags=bad)) == F.RT_ERR_INVALID and "flag bits" in err()
        assert device(device_params(flags=bad)) == F.RT_ERR_INVALID and "flag bits" in err()
    assert host(params(flags=F.RT_FLAG_COUNTERS)) == F.RT_ERR_INVALID and "null scene" in err()
    # a device output that is not 16-byte aligned, device rows that are not 4-byte aligned
    for off in (8, 4, 1):
        assert device(device_params(), out_=8192 + off) == F.RT_ERR_INVALID and "16-byte aligned" in err()
    for off in (1, 2, 3):
        assert device(device_params(row_ids=4096 + off)) == F.RT_ERR_INVALID and "4-byte aligned" in err()
    assert device(device_params(row_ids=4096 + 4), out_=8192 + 16) == F.RT_ERR_INVALID and "null scene" in err()
    # width, height or n_frames equal to 0
    for field in ("width", "height", "n_frames"):
        assert host(params(**{field: 0})) == F.RT_ERR_INVALID and "empty image" in err(), field
        assert device(device_params(**{field: 0})) == F.RT_ERR_INVALID and "empty image" in err(), field
    # a row id >= height * n_frames (host rows: checked on the host; device rows need the device)
    bad_rows = np.array([0, 1, 4, 2], dtype=np.uint32)
    assert host(params(row_ids=bad_rows.ctypes.data)) == F.RT_ERR_INVALID and "row id out of range" in err()
    two = np.array([0, 7, 4, 2], dtype=np.uint32)
    assert host(params(row_ids=two.ctypes.data, n_frames=2)) == F.RT_ERR_INVALID and "null scene" in err()
    two[1] = 8
    assert host(params(row_ids=two.ctypes.data, n_frames=2)) == F.RT_ERR_INVALID and "row id out of range" in err()
    # ignored fields are ignored: max_depth 0, any spp_chunk, a progress callback
    assert host(params(max_depth=0, spp_chunk=7, progress_cb=1234)) == F.RT_ERR_INVALID and "null scene" in err()
    assert not out.view(np.uint8).any()                                       # nothing was written
