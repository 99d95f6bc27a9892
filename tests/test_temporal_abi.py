"""Temporal accumulation (rt_temporal*): the two records' layouts, the bindings, the workspace size and argument checking.
No compute calls: runs without a GPU (every RT_ERR_INVALID case returns before any device call)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL_OFFSETS = {"e": 0, "n": 24, "depth": 32, "normal": 40}
PARAM_OFFSETS = {"width": 0, "height": 4, "spp": 8, "flags": 12, "tol_depth": 16, "tol_normal": 24, "n_max": 32, "w_min": 40,
                 "albedo_floor": 48, "_pad": 56}


def header_fields(text, name):
    """(field, offset) of a struct of uint32_t / double members as the header declares it, and its size."""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S)
    assert m, "%s is not declared" % name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields, off = [], 0
    for ctype, names in re.findall(r"(uint32_t|double)\s+([\w\s,\[\]]+);", body):
        size = 4 if ctype == "uint32_t" else 8
        for decl in [s.strip() for s in names.split(",")]:
            am = re.match(r"(\w+)\[(\d+)\]$", decl)
            count = int(am.group(2)) if am else 1
            off = (off + size - 1) // size * size
            fields.append((am.group(1) if am else decl, off))
            off += size * count
    return fields, off


def test_layouts_header_bindings_and_library_agree(rt):
    from raytracer_2022_amd import _ffi as F
    assert C.sizeof(F.rt_temporal_pixel) == 64 and C.sizeof(F.rt_temporal_params) == 64
    assert F.TEMPORAL_PIXEL_DTYPE.itemsize == 64
    out = (C.c_uint32 * 8)()
    n = rt.lib().rtb_temporal_abi_sizes(out, 8)
    assert n == len(F.TEMPORAL_ABI_STRUCTS) == 2
    assert [out[i] for i in range(n)] == [C.sizeof(t) for t in F.TEMPORAL_ABI_STRUCTS] == [64, 64]
    assert rt.lib().rtb_temporal_abi_sizes(out, 0) == 2                       # (a size query writes nothing)
    text = open(os.path.join(ROOT, "include", "rt2022.h")).read()
    for struct, offsets in ((F.rt_temporal_pixel, PIXEL_OFFSETS), (F.rt_temporal_params, PARAM_OFFSETS)):
        assert [f[0] for f in struct._fields_] == list(offsets)
        for name, off in offsets.items():
            assert getattr(struct, name).offset == off, name
        fields, size = header_fields(text, struct.__name__)
        assert fields == list(offsets.items()) and size == 64, struct.__name__
    assert {k: F.TEMPORAL_PIXEL_DTYPE.fields[k][1] for k in PIXEL_OFFSETS} == PIXEL_OFFSETS
    assert all(off % 16 in (0, 8) for off in PIXEL_OFFSETS.values())
    assert "#define RT_TEMPORAL_NO_DEMODULATE 0x1u" in text and F.RT_TEMPORAL_NO_DEMODULATE == 1
    assert re.search(r"uint64_t rt_temporal_workspace_bytes\(const rt_temporal_params \*p\);", text)
    assert re.search(r"int rt_temporal_device\(const double \*d_rgb_sum, const rt_feature \*d_features, const uint32_t \*d_row_ids,\s*"
                     r"const rt_camera \*cam, const rt_temporal_pixel \*d_prev, const rt_camera \*prev_cam,\s*"
                     r"const rt_temporal_params \*p, rt_temporal_pixel \*d_state_out, double \*d_out_rgb_sum,\s*"
                     r"void \*d_workspace, void \*hip_stream\);", text)
    assert re.search(r"int rt_temporal\(const double \*rgb_sum, const rt_feature \*features, const uint32_t \*row_ids,\s*"
                     r"const rt_camera \*cam, const rt_temporal_pixel \*prev, const rt_camera \*prev_cam,\s*"
                     r"const rt_temporal_params \*p, rt_temporal_pixel \*state_out, double \*out_rgb_sum, double \*ms\);", text)
    # what was there stays: the ABI version and every other list
    assert rt.lib().rt_abi_version() == 3 and F.RT2022_ABI_VERSION == 3
    assert len(F.ABI_STRUCTS) == 20 and rt.lib().rtb_abi_sizes(out, 0) == 20
    assert [len(l) for l in (F.RADIANCE_ABI_STRUCTS, F.FEATURES_ABI_STRUCTS, F.DENOISE_ABI_STRUCTS, F.DENOISE_DUAL_ABI_STRUCTS,
                             F.ADAPTIVE_ABI_STRUCTS)] == [2, 1, 1, 1, 1]
    assert [rt.lib().rtb_radiance_abi_sizes(out, 0), rt.lib().rtb_features_abi_sizes(out, 0), rt.lib().rtb_denoise_abi_sizes(out, 0),
            rt.lib().rtb_denoise_dual_abi_sizes(out, 0), rt.lib().rtb_adaptive_abi_sizes(out, 0)] == [2, 1, 1, 1, 1]
    for lst in (F.ABI_STRUCTS, F.RADIANCE_ABI_STRUCTS, F.FEATURES_ABI_STRUCTS, F.DENOISE_ABI_STRUCTS, F.DENOISE_DUAL_ABI_STRUCTS, F.ADAPTIVE_ABI_STRUCTS):
        assert F.rt_temporal_pixel not in lst and F.rt_temporal_params not in lst
    # the Python constructor's defaults are the package's tuned point, which is one of the grid's
    d = rt.TEMPORAL_DEFAULTS
    p = rt.temporal_params(5, 3, 4)
    assert (p.width, p.height, p.spp, p.flags) == (5, 3, 4, 0)
    assert (p.tol_depth, p.tol_normal, p.n_max, p.w_min) == (d["tol_depth"], d["tol_normal"], d["n_max"], d["w_min"])
    assert d["tol_depth"] in (0.02, 0.05, 0.1, 0.2) and d["tol_normal"] in (0.05, 0.1, 0.3) and d["n_max"] in (8, 32) and d["w_min"] == 0.25
    assert rt.temporal_params(5, 3, 4, demodulate=False).flags == F.RT_TEMPORAL_NO_DEMODULATE
    for name in ("temporal", "temporal_device", "temporal_params", "temporal_workspace_bytes", "TEMPORAL_DEFAULTS", "TEMPORAL_PIXEL_DTYPE"):
        assert name in rt.__all__ and hasattr(rt, name)


def bad_params(rt):
    """(what, message part, params) for every way the parameter block can be invalid."""
    inf, nan = math.inf, math.nan
    mk = lambda W=8, H=6, spp=4, **kw: rt.temporal_params(W, H, spp, **kw)
    cases = [("width 0", "empty image", mk(W=0)), ("height 0", "empty image", mk(H=0)), ("spp 0", "spp", mk(spp=0)),
             ("too many pixels", "RT_DENOISE_MAX_PIXELS", mk(W=1 << 19, H=(1 << 17) + 1))]
    for v in (0.0, -0.0, -1.0, nan, -inf):
        cases.append(("tol_depth = %r" % v, "tolerance", mk(tol_depth=v)))
        cases.append(("tol_normal = %r" % v, "tolerance", mk(tol_normal=v)))
    for v in (0.0, 0.999, -3.0, nan, inf, -inf):
        cases.append(("n_max = %r" % v, "n_max", mk(n_max=v)))
    for v in (0.0, -0.0, -0.5, 1.0000001, nan, inf, -inf):
        cases.append(("w_min = %r" % v, "w_min", mk(w_min=v)))
    for v in (0.0, -1.0, nan, inf, -inf):
        cases.append(("albedo_floor = %r" % v, "albedo_floor", mk(albedo_floor=v)))
    for bits in (0x2, 0x3, 0x80000000):
        p = mk()
        p.flags = bits
        cases.append(("flags %#x" % bits, "flag", p))
    return cases


def test_workspace_bytes(rt):
    """The documented formula: the inverse row map, height x uint32 rounded up to 16 bytes, and 16 bytes for its count."""
    shapes = ((1, 1), (5, 3), (67, 35), (800, 800), (1 << 16, 1 << 16), (3, 4), (3, 5))
    sizes = [rt.temporal_workspace_bytes(rt.temporal_params(w, h, 4)) for w, h in shapes]
    assert sizes == [(4 * h + 15) // 16 * 16 + 16 for w, h in shapes]
    assert all(s >= 32 and s % 16 == 0 for s in sizes)
    p = rt.temporal_params(67, 35, 1, tol_depth=math.inf, tol_normal=math.inf, n_max=1.0, w_min=1.0, demodulate=False)
    assert rt.temporal_workspace_bytes(p) == sizes[2]
    assert rt.lib().rt_temporal_workspace_bytes(None) == 0
    for what, _, p in bad_params(rt):
        assert rt.temporal_workspace_bytes(p) == 0, what


def test_temporal_arguments_are_checked_before_the_device(rt):
    """Every RT_ERR_INVALID case of the two entry points, each with a message — on a machine without a GPU too."""
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    W, H = 8, 6
    sums, feat = np.ones((H, W, 3)), np.zeros((H, W), dtype=F.FEATURE_DTYPE)
    both = np.zeros((2, H, W), dtype=F.TEMPORAL_PIXEL_DTYPE)
    prev, state = both[0], both[1]
    out = np.zeros((H, W, 3))
    cam = rt.camera_new((0, 0, 0), (0, 0, -1), (0, 1, 0), 90.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    good = rt.temporal_params(W, H, 4)
    nbytes = W * H * 64
    err = lambda: L.rt_last_error().decode()
    ref = lambda x: C.byref(x) if x is not None else None

    def host(p, s=sums.ctypes.data, f=feat.ctypes.data, rows=None, cam=cam, pv=prev.ctypes.data, pcam=cam, st=state.ctypes.data, o=out.ctypes.data):
        return L.rt_temporal(s, f, rows, ref(cam), pv, ref(pcam), ref(p), st, o, None)

    def device(p, s=1 << 20, f=2 << 20, rows=None, cam=cam, pv=3 << 20, pcam=cam, st=4 << 20, o=5 << 20, ws=6 << 20):
        return L.rt_temporal_device(s, f, rows, ref(cam), pv, ref(pcam), ref(p), st, o, ws, None)

    for what, part, p in bad_params(rt):
        assert host(p) == F.RT_ERR_INVALID and part in err() and err().startswith("rt_temporal: "), (what, err())
        assert device(p) == F.RT_ERR_INVALID and part in err() and err().startswith("rt_temporal_device: "), (what, err())
    assert host(None) == F.RT_ERR_INVALID and "null params" in err()
    assert device(None) == F.RT_ERR_INVALID and "null params" in err()
    assert L.rt_temporal(None, None, None, None, None, None, None, None, None, None) == F.RT_ERR_INVALID
    assert L.rt_temporal_device(None, None, None, None, None, None, None, None, None, None, None) == F.RT_ERR_INVALID
    for kw in ({"s": None}, {"f": None}, {"o": None}):
        assert host(good, **kw) == F.RT_ERR_INVALID and "null sums, features or output" in err(), kw
        assert device(good, **kw) == F.RT_ERR_INVALID and "null sums, features or output" in err(), kw
    assert host(good, st=None) == F.RT_ERR_INVALID and "null output state" in err()
    assert device(good, st=None) == F.RT_ERR_INVALID and "null output state" in err()
    assert host(good, cam=None) == F.RT_ERR_INVALID and "null camera" in err()
    assert device(good, cam=None) == F.RT_ERR_INVALID and "null camera" in err()
    assert device(good, ws=None) == F.RT_ERR_INVALID and "null workspace" in err()
    # a previous state needs its camera; without one the camera may be missing too (that call goes on to the device: not made here)
    assert host(good, pcam=None) == F.RT_ERR_INVALID and "without its camera" in err()
    assert device(good, pcam=None) == F.RT_ERR_INVALID and "without its camera" in err()
    # overlapping states: the same record array, and ranges that share one record at either end
    for pv, st in ((4 << 20, 4 << 20), (4 << 20, (4 << 20) + nbytes - 64), ((4 << 20) + nbytes - 64, 4 << 20), (4 << 20, (4 << 20) + 16)):
        assert device(good, pv=pv, st=st) == F.RT_ERR_INVALID and "overlaps" in err(), (pv, st)
    assert host(good, st=prev.ctypes.data) == F.RT_ERR_INVALID and "overlaps" in err()
    assert host(good, st=prev.ctypes.data + 64) == F.RT_ERR_INVALID and "overlaps" in err()
    # misalignment: every device pointer by 16, the rows by 4
    for kw in ({"s": (1 << 20) + 8}, {"f": (2 << 20) + 8}, {"pv": (3 << 20) + 8}, {"st": (4 << 20) + 8}, {"o": (5 << 20) + 8}, {"ws": (6 << 20) + 4},
               {"o": (5 << 20) + 1}):
        assert device(good, **kw) == F.RT_ERR_INVALID and "16-byte aligned" in err(), kw
    for off in (1, 2, 3):
        assert device(good, rows=(7 << 20) + off) == F.RT_ERR_INVALID and "4-byte aligned" in err()
    # host rows that are not a permutation of [0, height)
    for bad in ([0, 1, 2, 3, 4, 4], [0, 1, 2, 3, 4, 6], [5, 4, 3, 2, 1, 0xFFFFFFFF]):
        rows = np.array(bad, dtype=np.uint32)
        assert host(good, rows=rows.ctypes.data) == F.RT_ERR_INVALID and "not a permutation" in err(), bad
    assert not out.any() and not both.view(np.float64).any()                  # nothing was written
    # the Python wrapper refuses buffers of the wrong size before the library sees them
    with pytest.raises(ValueError):
        rt.temporal(sums[:-1], feat, cam, good)
    with pytest.raises(ValueError):
        rt.temporal(sums, feat[:-1], cam, good)
    with pytest.raises(ValueError):
        rt.temporal(sums, feat, cam, good, prev=prev[:-1], prev_cam=cam)
    with pytest.raises(ValueError):
        rt.temporal(sums, feat, cam, good, row_ids=np.arange(H - 1))
