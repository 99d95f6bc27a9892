"""Variance-guided denoiser (rt_denoise_dual*): the parameter block's layout, the bindings, the workspace size and argument
checking. No compute calls: runs without a GPU (every RT_ERR_INVALID case returns before any device call)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from denoise_ref import bad_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSETS = {"var_iter": 0, "flags": 4, "var_floor": 8}


def test_params_layout_header_bindings_and_library_agree(rt):
    from raytracer_2022_amd import _ffi as F
    assert C.sizeof(F.rt_denoise_dual_params) == 16
    out = (C.c_uint32 * 8)()
    n = rt.lib().rtb_denoise_dual_abi_sizes(out, 8)
    assert n == len(F.DENOISE_DUAL_ABI_STRUCTS) == 1
    assert [out[i] for i in range(n)] == [C.sizeof(t) for t in F.DENOISE_DUAL_ABI_STRUCTS] == [16]
    assert rt.lib().rtb_denoise_dual_abi_sizes(out, 0) == 1                  # (a size query writes nothing)
    assert [f[0] for f in F.rt_denoise_dual_params._fields_] == list(OFFSETS)
    for name, off in OFFSETS.items():
        assert getattr(F.rt_denoise_dual_params, name).offset == off, name
    text = open(os.path.join(ROOT, "include", "rt2022.h")).read()
    m = re.search(r"typedef struct rt_denoise_dual_params \{(.*?)\} rt_denoise_dual_params;", text, flags=re.S)
    assert m, "rt_denoise_dual_params is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields, off = [], 0
    for ctype, names in re.findall(r"(uint32_t|double)\s+([\w\s,]+);", body):
        size = 4 if ctype == "uint32_t" else 8
        for name in [s.strip() for s in names.split(",")]:
            off = (off + size - 1) // size * size
            fields.append((name, off))
            off += size
    assert fields == list(OFFSETS.items()) and off == 16
    assert "#define RT_DENOISE_MAX_VAR_ITER 8" in text and F.RT_DENOISE_MAX_VAR_ITER == 8
    assert re.search(r"uint64_t rt_denoise_dual_workspace_bytes\(const rt_denoise_params \*p\);", text)
    assert re.search(r"int rt_denoise_dual_device\(const double \*d_sum_a, const double \*d_sum_b,\s*"
                     r"const rt_feature \*d_feat_a, const rt_feature \*d_feat_b,\s*"
                     r"const uint32_t \*d_row_ids, const rt_denoise_params \*p, const rt_denoise_dual_params \*q,\s*"
                     r"double \*d_out_rgb_sum, double \*d_out_variance, void \*d_workspace, void \*hip_stream\);", text)
    assert re.search(r"int rt_denoise_dual\(const double \*sum_a, const double \*sum_b,\s*"
                     r"const rt_feature \*feat_a, const rt_feature \*feat_b,\s*"
                     r"const uint32_t \*row_ids, const rt_denoise_params \*p, const rt_denoise_dual_params \*q,\s*"
                     r"double \*out_rgb_sum, double \*out_variance, double \*ms\);", text)
    # what was there stays: the ABI version, rt_denoise's one-entry list, the general list
    assert rt.lib().rt_abi_version() == 3 and F.RT2022_ABI_VERSION == 3
    assert len(F.DENOISE_ABI_STRUCTS) == 1 and rt.lib().rtb_denoise_abi_sizes(out, 0) == 1
    assert F.rt_denoise_dual_params not in F.ABI_STRUCTS and F.rt_denoise_dual_params not in F.DENOISE_ABI_STRUCTS
    # the Python constructor's defaults are the package's tuned point, which is one of the grid's
    q = rt.denoise_dual_params()
    d = rt.DUAL_DEFAULTS
    assert (q.var_iter, q.flags, q.var_floor) == (d["var_iter"], 0, d["var_floor"])
    assert d["sigma_color"] in (0.5, 1.0, 2.0, 4.0) and d["var_iter"] in (1, 2, 3) and d["var_floor"] in (1e-6, 1e-4, 1e-2)
    q = rt.denoise_dual_params(var_iter=3, var_floor=0.25)
    assert (q.var_iter, q.flags, q.var_floor) == (3, 0, 0.25)
    assert rt.two_frame_rows([2, 0, 1], 3).tolist() == [2, 0, 1, 5, 3, 4] and rt.two_frame_rows([2, 0, 1], 3).dtype == np.uint32


def documented_bytes(w, h):
    """pt_device.h's DenoiseDualLayout: three guide planes of 16-byte pieces, a2's plane of doubles, two colour ping-pongs of two
    16-byte planes, two variance planes of doubles (a plane of doubles ends on a 16-byte piece), the row map and its count."""
    n = w * h
    plane8 = (n + 1) // 2 * 16
    return 3 * 16 * n + plane8 + 2 * (2 * 16 * n) + 2 * plane8 + (4 * h + 15) // 16 * 16 + 16


def test_workspace_bytes(rt):
    from raytracer_2022_amd import _ffi as F
    shapes = ((1, 1), (5, 3), (67, 35), (800, 800), (1 << 16, 1 << 16))
    sizes = [rt.denoise_dual_workspace_bytes(rt.denoise_params(w, h, 4)) for w, h in shapes]
    assert sizes == [documented_bytes(w, h) for w, h in shapes]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(set(sizes))
    inf = math.inf
    p = rt.denoise_params(67, 35, 1, n_iter=0, sigma_color=inf, sigma_normal=inf, sigma_depth=inf, sigma_albedo=inf, demodulate=False)
    assert rt.denoise_dual_workspace_bytes(p) == sizes[2]
    assert rt.denoise_dual_workspace_bytes(rt.denoise_params(67, 35, 4, n_iter=F.RT_DENOISE_MAX_ITER)) == sizes[2]
    assert rt.lib().rt_denoise_dual_workspace_bytes(None) == 0
    for what, p in bad_params(rt):
        assert rt.denoise_dual_workspace_bytes(p) == 0, what


def bad_dual_params(rt):
    """(what, message part, dual params) for every way the dual block can be invalid."""
    from raytracer_2022_amd import _ffi as F
    cases = [("var_iter", "var_iter", rt.denoise_dual_params(var_iter=F.RT_DENOISE_MAX_VAR_ITER + 1)),
             ("huge var_iter", "var_iter", rt.denoise_dual_params(var_iter=0xFFFFFFFF))]
    for v in (0.0, -1.0, -0.0, math.nan, math.inf, -math.inf):
        cases.append(("var_floor = %r" % v, "var_floor", rt.denoise_dual_params(var_floor=v)))
    for bits in (0x1, 0x80000000):
        q = rt.denoise_dual_params()
        q.flags = bits
        cases.append(("flags %#x" % bits, "flags", q))
    return cases


def test_denoise_dual_arguments_are_checked_before_the_device(rt):
    """Every RT_ERR_INVALID case of the two entry points, each with a message — on a machine without a GPU too."""
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    W, H = 8, 6
    sa, sb = np.ones((H, W, 3)), np.ones((H, W, 3))
    fa, fb = np.zeros((H, W), dtype=F.FEATURE_DTYPE), np.zeros((H, W), dtype=F.FEATURE_DTYPE)
    out, var = np.zeros((H, W, 3)), np.zeros((H, W))
    good, goodq = rt.denoise_params(W, H, 4), rt.denoise_dual_params()
    err = lambda: L.rt_last_error().decode()
    ref = lambda x: C.byref(x) if x is not None else None

    def host(p, q=goodq, sa=sa.ctypes.data, sb=sb.ctypes.data, fa=fa.ctypes.data, fb=fb.ctypes.data, o=out.ctypes.data, v=var.ctypes.data,
             rows=None):
        return L.rt_denoise_dual(sa, sb, fa, fb, rows, ref(p), ref(q), o, v, None)

    def device(p, q=goodq, sa=4096, sb=4096 * 2, fa=4096 * 3, fb=4096 * 4, o=4096 * 5, v=4096 * 6, ws=4096 * 7, rows=None):
        return L.rt_denoise_dual_device(sa, sb, fa, fb, rows, ref(p), ref(q), o, v, ws, None)

    # everything rt_denoise* refuses
    for what, p in bad_params(rt):
        assert host(p) == F.RT_ERR_INVALID and err().startswith("rt_denoise_dual: "), what
        assert device(p) == F.RT_ERR_INVALID and err().startswith("rt_denoise_dual_device: "), what
    assert host(rt.denoise_params(W, H, 4, n_iter=17)) == F.RT_ERR_INVALID and "n_iter" in err()
    assert device(rt.denoise_params(W, 0, 4)) == F.RT_ERR_INVALID and "empty image" in err()
    assert host(None) == F.RT_ERR_INVALID and "null params" in err()
    assert device(None) == F.RT_ERR_INVALID and "null params" in err()
    assert L.rt_denoise_dual(None, None, None, None, None, None, None, None, None, None) == F.RT_ERR_INVALID
    assert L.rt_denoise_dual_device(None, None, None, None, None, None, None, None, None, None, None) == F.RT_ERR_INVALID
    for kw in ({"sa": None}, {"fa": None}, {"o": None}):
        assert host(good, **kw) == F.RT_ERR_INVALID and "null sums, features or output" in err(), kw
        assert device(good, **kw) == F.RT_ERR_INVALID and "null sums, features or output" in err(), kw
    # the dual filter's own: a null q, sum_b or feat_b; var_iter, var_floor, flags
    assert host(good, q=None) == F.RT_ERR_INVALID and "null dual params" in err()
    assert device(good, q=None) == F.RT_ERR_INVALID and "null dual params" in err()
    for kw in ({"sb": None}, {"fb": None}):
        assert host(good, **kw) == F.RT_ERR_INVALID and "second half" in err(), kw
        assert device(good, **kw) == F.RT_ERR_INVALID and "second half" in err(), kw
    for what, part, q in bad_dual_params(rt):
        assert host(good, q=q) == F.RT_ERR_INVALID and part in err() and err().startswith("rt_denoise_dual: "), what
        assert device(good, q=q) == F.RT_ERR_INVALID and part in err() and err().startswith("rt_denoise_dual_device: "), what
    assert device(good, ws=None) == F.RT_ERR_INVALID and "null workspace" in err()
    # misalignment: every device pointer by 16 (the variance output included), the rows by 4
    for kw in ({"sa": 4096 + 8}, {"sb": 8192 + 8}, {"fa": 12288 + 8}, {"fb": 16384 + 8}, {"o": 20480 + 8}, {"v": 24576 + 8}, {"ws": 28672 + 4},
               {"v": 24576 + 1}):
        assert device(good, **kw) == F.RT_ERR_INVALID and "16-byte aligned" in err(), kw
    for off in (1, 2, 3):
        assert device(good, rows=65536 + off) == F.RT_ERR_INVALID and "4-byte aligned" in err()
    # host rows that are not a permutation of [0, height)
    for bad in ([0, 1, 2, 3, 4, 4], [0, 1, 2, 3, 4, 6], [5, 4, 3, 2, 1, 0xFFFFFFFF]):
        rows = np.array(bad, dtype=np.uint32)
        assert host(good, rows=rows.ctypes.data) == F.RT_ERR_INVALID and "not a permutation" in err(), bad
    assert not out.any() and not var.any()                                    # nothing was written
    # the Python wrapper refuses buffers of the wrong size before the library sees them
    with pytest.raises(ValueError):
        rt.denoise_dual(sa[:-1], sb, fa, fb, good)
    with pytest.raises(ValueError):
        rt.denoise_dual(sa, sb, fa, fb[:-1], good)
    with pytest.raises(ValueError):
        rt.denoise_dual(sa, sb, fa, fb, good, row_ids=np.arange(H - 1))
