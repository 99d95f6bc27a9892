"""Adaptive sampling (rt_adaptive_*): the parameter block's layout, the bindings, the workspace size, every refusal, and the
numpy scale search against the restatement. No compute calls: runs without a GPU (every RT_ERR_INVALID case returns before
any device call)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import adaptive_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSETS = {"width": 0, "height": 4, "first_frame": 8, "max_units": 12, "scale": 16, "flags": 24, "_pad": 28}


def test_params_layout_header_bindings_and_library_agree(rt):
    from raytracer_2022_amd import _ffi as F
    assert C.sizeof(F.rt_adaptive_params) == 32
    out = (C.c_uint32 * 8)()
    n = rt.lib().rtb_adaptive_abi_sizes(out, 8)
    assert n == len(F.ADAPTIVE_ABI_STRUCTS) == 1
    assert [out[i] for i in range(n)] == [C.sizeof(t) for t in F.ADAPTIVE_ABI_STRUCTS] == [32]
    assert rt.lib().rtb_adaptive_abi_sizes(out, 0) == 1
    assert [f[0] for f in F.rt_adaptive_params._fields_] == list(OFFSETS)
    for name, off in OFFSETS.items():
        assert getattr(F.rt_adaptive_params, name).offset == off, name
    text = open(os.path.join(ROOT, "include", "rt2022.h")).read()
    m = re.search(r"typedef struct rt_adaptive_params \{(.*?)\} rt_adaptive_params;", text, flags=re.S)
    assert m, "rt_adaptive_params is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields, off = [], 0
    for ctype, names in re.findall(r"(uint32_t|double)\s+([\w\s,]+);", body):
        size = 4 if ctype == "uint32_t" else 8
        for name in [s.strip() for s in names.split(",")]:
            off = (off + size - 1) // size * size
            fields.append((name, off))
            off += size
    assert fields == list(OFFSETS.items()) and off == 32
    assert rt.lib().rt_abi_version() == 3 and F.rt_adaptive_params not in F.ABI_STRUCTS
    p = rt.adaptive_params(7, 5, 2.5, 3, first_frame=9)
    assert (p.width, p.height, p.first_frame, p.max_units, p.scale, p.flags, p._pad) == (7, 5, 9, 3, 2.5, 0, 0)
    ids = rt.pixel_ids(2, [0, 1], [3, 4], 10, 6)
    assert ids.dtype == np.uint64 and ids.tolist() == [123, 134]
    assert rt.pixel_ids(1 << 25, 11, 15, 16, 12).tolist() == [(1 << 25) * 192 + 11 * 16 + 15]     # (past 2^32)


def bad_params(rt):
    """(what, message part, params) for every way the block can be invalid."""
    good = lambda **kw: rt.adaptive_params(kw.pop("width", 8), kw.pop("height", 6), kw.pop("scale", 1.0), kw.pop("max_units", 4), **kw)
    cases = [("width 0", "empty image", good(width=0)), ("height 0", "empty image", good(height=0)),
             ("too many pixels", "RT_DENOISE_MAX_PIXELS", good(width=1 << 19, height=(1 << 17) + 1)),
             ("max_units 0", "max_units", good(max_units=0)),
             ("frames overflow", "first_frame + max_units", good(first_frame=0xFFFFFFFF, max_units=1)),
             ("frames overflow 2", "first_frame + max_units", good(first_frame=5, max_units=0xFFFFFFFB))]
    for v in (0.0, -1.0, -0.0, math.nan, math.inf, -math.inf):
        cases.append(("scale = %r" % v, "scale", good(scale=v)))
    for field in ("flags", "_pad"):
        for bits in (0x1, 0x80000000):
            p = good()
            setattr(p, field, bits)
            cases.append(("%s %#x" % (field, bits), "flags", p))
    return cases


def test_workspace_bytes(rt):
    def documented(w, h):
        """pt_device.h's AdaptiveLayout: (tiles + 1) words of 8 bytes for the scan (tiles of 1024 pixels), the row kernel's count
        in a 16-byte piece, its map of `height` words — each part ends on a 16-byte piece."""
        tiles = (w * h + 1023) // 1024
        return ((tiles + 1) * 8 + 15) // 16 * 16 + 16 + (4 * h + 15) // 16 * 16
    shapes = ((1, 1), (64, 1), (65, 3), (257, 33), (800, 800), (1 << 18, 1 << 18))
    sizes = [rt.adaptive_workspace_bytes(rt.adaptive_params(w, h, 1.0, 4)) for w, h in shapes]
    assert sizes == [documented(w, h) for w, h in shapes]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert rt.adaptive_workspace_bytes(rt.adaptive_params(4, 4, 1.0, 0xFFFFFFFF)) > 0       # first_frame + max_units == 2^32 - 1
    assert rt.lib().rt_adaptive_workspace_bytes(None) == 0
    for what, _, p in bad_params(rt):
        assert rt.adaptive_workspace_bytes(p) == 0, what


def test_every_refusal_comes_before_the_device(rt):
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    W, H = 8, 6
    err_map = np.ones((H, W))
    units, offsets, entries = np.zeros(W * H, dtype=np.uint32), np.zeros(W * H + 1, dtype=np.uint64), np.zeros(W * H * 4, dtype=np.uint64)
    good = rt.adaptive_params(W, H, 1.0, 4)
    err = lambda: L.rt_last_error().decode()
    ref = lambda x: C.byref(x) if x is not None else None

    def host(p, e=err_map.ctypes.data, rows=None, u=units.ctypes.data, o=offsets.ctypes.data, en=entries.ctypes.data, cap=entries.size):
        return L.rt_adaptive_plan(e, rows, ref(p), u, o, en, cap, None)

    def device(p, e=4096, rows=None, u=4096 * 2, o=4096 * 3, en=4096 * 4, cap=16, ws=4096 * 5):
        return L.rt_adaptive_plan_device(e, rows, ref(p), u, o, en, cap, ws, None, None)

    for what, part, p in bad_params(rt):
        assert host(p) == F.RT_ERR_INVALID and part in err() and err().startswith("rt_adaptive_plan: "), what
        assert device(p) == F.RT_ERR_INVALID and part in err() and err().startswith("rt_adaptive_plan_device: "), what
    assert host(None) == F.RT_ERR_INVALID and "null params" in err()
    assert device(None) == F.RT_ERR_INVALID and "null params" in err()
    for kw in ({"e": None}, {"u": None}, {"o": None}):
        assert host(good, **kw) == F.RT_ERR_INVALID and "null error map, units or offsets" in err(), kw
        assert device(good, **kw) == F.RT_ERR_INVALID and "null error map, units or offsets" in err(), kw
    assert host(good, en=None) == F.RT_ERR_INVALID and "null entries" in err()
    assert device(good, en=None) == F.RT_ERR_INVALID and "null entries" in err()
    assert device(good, ws=None) == F.RT_ERR_INVALID and "null workspace" in err()
    for kw in ({"e": 4096 + 8}, {"ws": 4096 * 5 + 8}, {"e": 4096 + 1}):
        assert device(good, **kw) == F.RT_ERR_INVALID and "16-byte aligned" in err(), kw
    for kw in ({"o": 4096 * 3 + 4}, {"en": 4096 * 4 + 4}, {"en": 4096 * 4 + 1}):
        assert device(good, **kw) == F.RT_ERR_INVALID and "8-byte aligned" in err(), kw
    for kw in ({"u": 4096 * 2 + 2}, {"rows": 65536 + 1}, {"rows": 65536 + 2}):
        assert device(good, **kw) == F.RT_ERR_INVALID and "4-byte aligned" in err(), kw
    for bad in ([0, 1, 2, 3, 4, 4], [0, 1, 2, 3, 4, 6], [5, 4, 3, 2, 1, 0xFFFFFFFF]):
        rows = np.array(bad, dtype=np.uint32)
        assert host(good, rows=rows.ctypes.data) == F.RT_ERR_INVALID and "not a permutation" in err(), bad
    assert not units.any() and not offsets.any() and not entries.any()          # nothing was written
    # merge and resolve: null buffers, too many pixels, misalignment; no pixel is no work
    M, Rz = L.rt_adaptive_merge_device, L.rt_adaptive_resolve_device
    assert M(None, None, None, 0, 1, None, None, None) == F.RT_OK and Rz(None, None, 0, 1, None, None) == F.RT_OK
    big = (1 << 36) + 1
    assert M(4096, 8192, 12288, big, 1, 16384, 20480, None) == F.RT_ERR_INVALID and "RT_DENOISE_MAX_PIXELS" in err()
    assert Rz(4096, 8192, big, 1, 12288, None) == F.RT_ERR_INVALID and "RT_DENOISE_MAX_PIXELS" in err()
    for k in range(5):
        a = [4096, 8192, 12288, 16384, 20480]
        a[k] = None
        assert M(a[0], a[1], a[2], 4, 1, a[3], a[4], None) == F.RT_ERR_INVALID and "null buffer" in err(), k
        a[k] = 4096 * (k + 1) + (2 if k == 1 else 4)
        assert M(a[0], a[1], a[2], 4, 1, a[3], a[4], None) == F.RT_ERR_INVALID and "aligned" in err(), k
    for k in range(3):
        a = [4096, 8192, 12288]
        a[k] = None
        assert Rz(a[0], a[1], 4, 1, a[2], None) == F.RT_ERR_INVALID and "null buffer" in err(), k
        a[k] = 4096 * (k + 1) + 4
        assert Rz(a[0], a[1], 4, 1, a[2], None) == F.RT_ERR_INVALID and "8-byte aligned" in err(), k
    with pytest.raises(ValueError):
        rt.adaptive_plan(err_map[:-1], good)
    with pytest.raises(ValueError):
        rt.adaptive_plan(err_map, good, row_ids=np.arange(H - 1))


def error_maps():
    rng = np.random.default_rng(2022)
    maps = {"uniform": rng.random(500), "lognormal": rng.lognormal(-3.0, 2.0, 700), "zeros": np.zeros(64),
            "one hot": np.concatenate([np.zeros(99), [5.0]]), "equal": np.full(50, 0.25)}
    hostile = rng.random(300)
    hostile[::7] = np.nan
    hostile[3::11] = np.inf
    hostile[5::13] = -np.inf
    hostile[1::17] = -2.0
    maps["hostile"] = hostile
    return maps


@pytest.mark.parametrize("name", list(error_maps()))
@pytest.mark.parametrize("max_units", [1, 4, 1000])
def test_adaptive_scale_meets_the_budget_and_is_tight(rt, name, max_units):
    """The total of the scale found never exceeds the budget; the next representable scale above it does, or the plan is
    already at max_units wherever a pixel can get a unit at all."""
    e = error_maps()[name]
    total = lambda s: int(R.plan(e, e.size, 1, s, max_units)[3])
    assert np.array_equal(rt.plan_units(e, 0.37, max_units), R.plan(e, e.size, 1, 0.37, max_units)[0])
    can = int(np.count_nonzero(e > 0.0))                                        # (+inf included; NaN and negatives never)
    for budget in (0, 1, 7, e.size // 3, e.size * max_units, e.size * max_units * 2):
        s = rt.adaptive_scale(e, budget, max_units)
        if not s > 0.0:
            # nothing fits: no budget, no pixel that can take a unit, or infinities that alone exceed it
            assert s == 0.0
            forced = int(np.count_nonzero(e == np.inf)) * max_units
            assert budget <= 0 or can == 0 or forced > budget or total(np.nextafter(0.5 / e[np.isfinite(e) & (e > 0)].max(), np.inf)) > budget
            continue
        assert math.isfinite(s) and total(s) <= budget
        up = np.nextafter(s, np.inf)
        assert total(up) > budget or total(s) == can * max_units, (budget, s, total(s), total(up))
