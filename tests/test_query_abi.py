"""Closest-hit queries (rt_intersect*): the record layouts, the Python helpers and argument checking. No compute
calls: runs without a GPU."""
import ctypes as C

import numpy as np
import pytest


def test_query_structs_dtypes_and_library_agree(rt):
    from raytracer_2022_amd import _ffi as F
    assert C.sizeof(F.rt_query_ray) == 80 and C.sizeof(F.rt_hit) == 96
    assert F.QUERY_RAY_DTYPE.itemsize == 80 and F.HIT_DTYPE.itemsize == 96
    out = (C.c_uint32 * 64)()
    n = rt.lib().rtb_abi_sizes(out, 64)
    assert n == len(F.ABI_STRUCTS) and F.ABI_STRUCTS[-2:] == [F.rt_query_ray, F.rt_hit]
    assert [out[n - 2], out[n - 1]] == [80, 96]
    # field offsets as declared in include/rt2022.h, the same in ctypes and numpy
    ray_offsets = {"origin": 0, "direction": 24, "time": 48, "t_min": 56, "t_max": 64, "rng_state": 72}
    hit_offsets = {"t": 0, "u": 8, "v": 16, "p": 24, "normal": 48, "hit": 72, "front_face": 76, "mat": 80, "prim": 84,
                   "rng_draws": 88, "_pad": 92}
    for ctype, dtype, offsets in ((F.rt_query_ray, F.QUERY_RAY_DTYPE, ray_offsets), (F.rt_hit, F.HIT_DTYPE, hit_offsets)):
        assert [f[0] for f in ctype._fields_] == list(offsets) == list(dtype.names)
        for name, off in offsets.items():
            assert getattr(ctype, name).offset == off, name
            assert dtype.fields[name][1] == off, name
    assert F.RT_FLAG_ANY_HIT == 0x8 and F.RT_REF_NONE == 0xFFFFFFFF
    assert not F.RT_FLAG_ANY_HIT & (F.RT_FLAG_COUNTERS | F.RT_FLAG_KERNEL_TIMES | F.RT_FLAG_ASYNC)
    # a numpy record and a ctypes record are the same bytes
    r = rt.query_rays((1, 2, 3), (4, 5, 6), time=0.5, t_min=0.25, t_max=7.0, rng_state=99)
    c = F.rt_query_ray.from_buffer_copy(r.tobytes())
    assert list(c.origin) == [1, 2, 3] and list(c.direction) == [4, 5, 6]
    assert (c.time, c.t_min, c.t_max, c.rng_state) == (0.5, 0.25, 7.0, 99)


def test_query_rays_broadcasts_and_fills_defaults(rt):
    o = np.arange(12, dtype=np.float64).reshape(4, 3)
    r = rt.query_rays(o, (0, 0, -1))
    assert r.dtype == rt.QUERY_RAY_DTYPE and r.shape == (4,)
    assert np.array_equal(r["origin"], o) and np.array_equal(r["direction"], np.tile([0.0, 0.0, -1.0], (4, 1)))
    assert np.all(r["time"] == 0.0) and np.all(r["t_min"] == 0.001) and np.all(np.isposinf(r["t_max"]))
    assert np.array_equal(r["rng_state"], np.arange(4, dtype=np.uint64))        # the documented default: ray i has state i
    r = rt.query_rays((0, 0, 0), np.eye(3), time=[0.0, 0.5, 1.0], t_max=10.0, rng_state=7)
    assert r.shape == (3,) and np.array_equal(r["time"], [0.0, 0.5, 1.0]) and np.all(r["t_max"] == 10.0)
    assert np.all(r["rng_state"] == 7) and np.array_equal(r["origin"], np.zeros((3, 3)))
    assert rt.query_rays((0, 0, 0), (1, 0, 0)).shape == (1,)
    with pytest.raises(ValueError):
        rt.query_rays((0, 0), (1, 0, 0))
    with pytest.raises(ValueError):
        rt.query_rays(np.zeros((3, 3)), np.zeros((2, 3)))


def test_intersect_arguments_are_checked_before_the_device(rt):
    """Null scene / buffers and unknown flags are RT_ERR_INVALID with a message — on a machine without a GPU too."""
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    rays = rt.query_rays((0, 0, 0), (0, 0, 1))
    hits = np.zeros(1, dtype=rt.HIT_DTYPE)
    st = F.rt_stats()
    assert L.rt_intersect(None, rays.ctypes.data, 1, 0, hits.ctypes.data, C.byref(st)) == F.RT_ERR_INVALID
    assert "null scene" in L.rt_last_error().decode()
    assert L.rt_intersect_device(None, rays.ctypes.data, 1, 0, hits.ctypes.data, None, None) == F.RT_ERR_INVALID
    assert L.rt_last_error().decode()
    assert L.rt_intersect(None, None, 0, 0, None, None) == F.RT_ERR_INVALID
