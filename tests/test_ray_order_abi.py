"""rt_ray_order* and rt_intersect_ordered* at the C ABI without a GPU: the parameter block against the header's text, the
workspace sizes, and every refusal that is decided before the first device call — with the output buffers poisoned and
unchanged. The order and the hits themselves are tests/test_ray_order_gpu.py's."""
import ctypes as C
import os
import re

import numpy as np

import ray_order_cases as K
import raytracer_2022_amd as rt
from raytracer_2022_amd import _ffi as F

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt2022.h")
FAKE = 0x7000_0000_0000                                   # a device address that is never dereferenced: the call is refused first
NO_SCENE = C.create_string_buffer(4096)                   # a handle that is no scene: a refused call never looks into it
SCENE = C.addressof(NO_SCENE)
N = 8
FILL = 0xA5


def refused(rc, who, word=None):
    msg = F.lib().rt_last_error()
    return rc == F.RT_ERR_INVALID and msg.startswith(who) and (word is None or word in msg)


def params(origin_bits=10, dir_bits=4, layout=0, stride=80):
    return rt.ray_order_params(origin_bits, dir_bits, layout, stride)


def order_device(rays=FAKE, n=N, p=None, order=FAKE + 0x1000, ws=FAKE + 0x10000, ws_bytes=None, null_params=False):
    p = params() if p is None else p
    ws_bytes = rt.ray_order_workspace_bytes(n) if ws_bytes is None else ws_bytes
    return F.lib().rt_ray_order_device(rays, n, None if null_params else C.byref(p), order, ws, ws_bytes, None)


def ordered_device(scene=SCENE, rays=FAKE, order=FAKE + 0x1000, n=N, flags=0, hits=FAKE + 0x2000, ws=FAKE + 0x10000, ws_bytes=None):
    ws_bytes = rt.intersect_ordered_workspace_bytes(n) if ws_bytes is None else ws_bytes
    return F.lib().rt_intersect_ordered_device(scene, rays, order, n, flags, hits, ws, ws_bytes, None, None)


def test_symbols_version_and_parameter_block_from_the_header_text():
    for sym in ("rt_ray_order_workspace_bytes", "rt_ray_order_device", "rt_ray_order", "rt_intersect_ordered_workspace_bytes",
                "rt_intersect_ordered_device", "rt_intersect_ordered"):
        assert sym in F.ABI_SYMBOLS and getattr(F.lib(), sym)
    assert F.lib().rt_abi_version() == F.RT2022_ABI_VERSION == 3
    text = open(HEADER).read()
    assert re.search(r"#define\s+RT2022_ABI_VERSION\s+3\b", text)
    body = re.search(r"typedef struct rt_ray_order_params \{(.*?)\} rt_ray_order_params;", text, re.S).group(1)
    fields = re.findall(r"\b(uint32_t|uint64_t|double)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [("uint32_t", "origin_bits"), ("uint32_t", "dir_bits"), ("uint32_t", "layout"), ("uint32_t", "ray_stride")]
    assert [f[0] for f in F.rt_ray_order_params._fields_] == [name for _, name in fields]
    assert [getattr(F.rt_ray_order_params, name).offset for _, name in fields] == [0, 4, 8, 12] and C.sizeof(F.rt_ray_order_params) == 16
    for name, value in (("RT_ORDER_ORIGIN_FIRST", 0), ("RT_ORDER_DIRECTION_FIRST", 1), ("RT_ORDER_FACE_ORIGIN_UV", 2)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), text) and getattr(F, name) == value
    p = rt.ray_order_params()
    assert (p.origin_bits, p.dir_bits, p.layout, p.ray_stride) == (rt.RAY_ORDER_DEFAULTS["origin_bits"], rt.RAY_ORDER_DEFAULTS["dir_bits"],
                                                                   rt.RAY_ORDER_DEFAULTS["layout"], 80)
    assert F.QUERY_RAY_DTYPE.fields["origin"][1] == F.RADIANCE_RAY_DTYPE.fields["origin"][1] == 0
    assert F.QUERY_RAY_DTYPE.fields["direction"][1] == F.RADIANCE_RAY_DTYPE.fields["direction"][1] == 24


def test_workspace_sizes_are_monotone_multiples_of_16():
    sizes = [0, 1, 2, 3, 63, 64, 65, 257, 4099, 100000, 1000000, (1 << 32) - 1, 1 << 32, 1 << 33]
    for fn, per_ray in ((rt.ray_order_workspace_bytes, 100), (rt.intersect_ordered_workspace_bytes, 200)):
        got = [fn(n) for n in sizes]
        assert all(b > 0 and b % 16 == 0 for b in got)
        assert all(a <= b for a, b in zip(got, got[1:]))
        dense = [fn(n) for n in range(0, 3000)]
        assert all(b % 16 == 0 for b in dense) and all(a <= b for a, b in zip(dense, dense[1:]))
        assert fn(1000000) < per_ray * 1000000
    assert rt.intersect_ordered_workspace_bytes(1000) >= 1000 * (80 + 96)


def test_ray_order_host_form_refusals_leave_the_order_untouched():
    rays = K.random_rays(N, 1)
    order = np.full(N, 0xA5A5A5A5, dtype=np.uint32)
    call = lambda r, n, p, o: F.lib().rt_ray_order(r, n, C.byref(p) if p is not None else None, o)
    who = b"rt_ray_order:"
    assert refused(call(None, N, params(), order.ctypes.data), who, b"null")
    assert refused(call(rays.ctypes.data, N, params(), None), who, b"null")
    assert refused(call(rays.ctypes.data, N, None, order.ctypes.data), who, b"null params")
    assert refused(call(rays.ctypes.data, 1 << 32, params(), order.ctypes.data), who, b"2^32")
    assert refused(call(rays.ctypes.data, 1 << 40, params(), order.ctypes.data), who, b"2^32")
    assert refused(call(rays.ctypes.data, N, params(origin_bits=17), order.ctypes.data), who, b"origin_bits")
    assert refused(call(rays.ctypes.data, N, params(dir_bits=7), order.ctypes.data), who, b"dir_bits")
    assert refused(call(rays.ctypes.data, N, params(layout=3), order.ctypes.data), who, b"layout")
    for stride in (0, 32, 40, 56, 72, 81, 88):
        assert refused(call(rays.ctypes.data, N, params(stride=stride), order.ctypes.data), who, b"ray_stride"), stride
    assert np.all(order == 0xA5A5A5A5)
    # nothing to do is no error, whatever the pointers
    assert call(None, 0, params(), None) == F.RT_OK
    assert refused(call(None, 0, params(layout=9), None), who, b"layout")            # (the parameters are checked all the same)


def test_ray_order_device_form_refusals_come_before_any_device_call():
    who = b"rt_ray_order_device:"
    need = rt.ray_order_workspace_bytes(N)
    assert refused(order_device(rays=None), who, b"null")
    assert refused(order_device(order=None), who, b"null")
    assert refused(order_device(null_params=True), who, b"null params")
    assert refused(order_device(ws=None), who, b"null workspace")
    assert refused(order_device(n=1 << 32), who, b"2^32")
    assert refused(order_device(p=params(origin_bits=17)), who, b"origin_bits")
    assert refused(order_device(p=params(dir_bits=7)), who, b"dir_bits")
    assert refused(order_device(p=params(layout=3)), who, b"layout")
    assert refused(order_device(p=params(stride=72)), who, b"ray_stride")
    assert refused(order_device(p=params(stride=32)), who, b"ray_stride")
    assert refused(order_device(ws_bytes=need - 1), who, b"workspace")
    assert refused(order_device(ws_bytes=0), who, b"workspace")
    assert refused(order_device(ws=FAKE + 0x10008), who, b"workspace")
    assert refused(order_device(rays=FAKE + 8), who, b"aligned")
    assert refused(order_device(order=FAKE + 0x1002), who, b"4-byte")
    assert order_device(rays=None, order=None, ws=None, n=0, ws_bytes=0) == F.RT_OK  # no launch
    for stride in (48, 64, 80, 96):                                                   # accepted strides get as far as the workspace check
        assert refused(order_device(p=params(stride=stride), ws_bytes=need - 1), who, b"workspace")


def test_ordered_query_device_form_refusals_come_before_any_device_call():
    who = b"rt_intersect_ordered_device:"
    need = rt.intersect_ordered_workspace_bytes(N)
    assert refused(ordered_device(scene=None), who, b"null scene")
    assert refused(ordered_device(rays=None), who, b"null")
    assert refused(ordered_device(hits=None), who, b"null")
    assert refused(ordered_device(order=None), who, b"null")
    assert refused(ordered_device(ws=None), who, b"null workspace")
    assert refused(ordered_device(n=1 << 32), who, b"2^32")
    assert refused(ordered_device(ws_bytes=need - 1), who, b"workspace")
    assert refused(ordered_device(ws=FAKE + 0x10004), who, b"workspace")
    assert refused(ordered_device(rays=FAKE + 8), who, b"16-byte")
    assert refused(ordered_device(hits=FAKE + 0x2008), who, b"16-byte")
    assert refused(ordered_device(order=FAKE + 0x1001), who, b"4-byte")
    # the flags are rt_intersect's: the four combinations of its two bits get as far as the workspace check, any other bit does not
    for flags in (0, F.RT_FLAG_COUNTERS, F.RT_FLAG_ANY_HIT, F.RT_FLAG_COUNTERS | F.RT_FLAG_ANY_HIT):
        assert refused(ordered_device(flags=flags, ws_bytes=need - 1), who, b"workspace"), flags
    for bit in range(32):
        if (1 << bit) not in (F.RT_FLAG_COUNTERS, F.RT_FLAG_ANY_HIT):
            assert refused(ordered_device(flags=1 << bit), who, b"unknown flag"), bit
            assert refused(ordered_device(flags=(1 << bit) | F.RT_FLAG_COUNTERS, ws_bytes=need - 1), who, b"unknown flag"), bit


def test_ordered_query_host_form_refusals_leave_the_hits_untouched():
    who = b"rt_intersect_ordered:"
    rays = K.random_rays(N, 2)
    order = np.arange(N, dtype=np.uint32)
    hits = np.zeros(N, dtype=F.HIT_DTYPE)
    hits.view(np.uint8)[:] = FILL
    st = F.rt_stats()
    st.rays = 77

    def call(scene=SCENE, r=rays.ctypes.data, o=order.ctypes.data, p=None, n=N, flags=0, h=hits.ctypes.data):
        return F.lib().rt_intersect_ordered(scene, r, o, C.byref(p) if p is not None else None, n, flags, h, C.byref(st))
    assert refused(call(scene=None), who, b"null scene")
    assert refused(call(r=None), who, b"null")
    assert refused(call(h=None), who, b"null")
    assert refused(call(n=1 << 32), who, b"2^32")
    assert refused(call(flags=F.RT_FLAG_ASYNC), who, b"unknown flag")
    assert refused(call(flags=F.RT_FLAG_KERNEL_TIMES), who, b"unknown flag")
    assert refused(call(flags=0x100), who, b"unknown flag")
    # no order: it is computed, so the parameters must be there and valid, for 80-byte records
    assert refused(call(o=None, p=None), who, b"null params")
    assert refused(call(o=None, p=params(origin_bits=17)), who, b"origin_bits")
    assert refused(call(o=None, p=params(dir_bits=7)), who, b"dir_bits")
    assert refused(call(o=None, p=params(layout=3)), who, b"layout")
    assert refused(call(o=None, p=params(stride=64)), who, b"ray_stride")
    assert np.all(hits.view(np.uint8) == FILL) and st.rays == 77
    assert call(r=None, o=None, p=params(), n=0, h=None) == F.RT_OK and st.rays == 0  # nothing to do: the stats zeroed, no launch
