"""Feature buffers of caller rays (rt_features_rays*): the bindings and the argument checking. No compute calls: runs without a
GPU (every RT_ERR_INVALID case returns before any device call, with or without a scene)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rt_features_rays", "rt_features_rays_device"]


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
    for name in ("features_rays", "features_rays_device"):
        assert callable(getattr(rt.DeviceScene, name))


def callers(rt, st=None):
    """(host, device): the two entry points with four good rays, good buffers and a null scene unless told otherwise."""
    L = rt.lib()
    rays = rt.radiance_rays((0, 0, 5), [(0, 0, -1), (0, 1, -1), (1, 0, -1), (1, 1, -1)])
    out = np.full(4 * 8, 7.0)
    keep = (rays, out)

    def host(p, rays_=rays.ctypes.data, n=4, out_=out.ctypes.data, scene=None):
        return L.rt_features_rays(scene, rays_, n, C.byref(p) if p is not None else None, out_, C.byref(st) if st is not None else None)

    def device(p, rays_=4096, n=4, out_=8192, scene=None):
        return L.rt_features_rays_device(scene, rays_, n, C.byref(p) if p is not None else None, out_, None, None)

    return host, device, out, keep


def test_ray_list_arguments_are_checked_before_the_device(rt):
    """Every RT_ERR_INVALID case of the two entry points, with its message and the output untouched."""
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    st = F.rt_stats()
    host, device, out, keep = callers(rt, st)
    params = lambda **kw: rt.radiance_params(**{"spp": 2, "background": (0.1, 0.2, 0.3), **kw})
    err = lambda: L.rt_last_error().decode()
    names = {host: "rt_features_rays", device: "rt_features_rays_device"}
    # a null scene or params
    for f in (host, device):
        assert f(params()) == F.RT_ERR_INVALID and err() == names[f] + ": null scene"
        assert f(None) == F.RT_ERR_INVALID and err() == names[f] + ": null params"
    assert L.rt_features_rays(None, None, 0, None, None, None) == F.RT_ERR_INVALID and err().startswith("rt_features_rays: ")
    assert L.rt_features_rays_device(None, None, 0, None, None, None, None) == F.RT_ERR_INVALID and err().startswith("rt_features_rays_device: ")
    for f in (host, device):
        # null rays or output with n_rays > 0 ... and with none they are not looked at
        assert f(params(), rays_=None) == F.RT_ERR_INVALID and err() == names[f] + ": null ray or output buffer"
        assert f(params(), out_=None) == F.RT_ERR_INVALID and err() == names[f] + ": null ray or output buffer"
        assert f(params(), rays_=None, out_=None, n=0) == F.RT_ERR_INVALID and "null scene" in err()
        # a flag bit other than the three
        for bad in (F.RT_FLAG_KERNEL_TIMES, F.RT_FLAG_ASYNC, F.RT_FLAG_ANY_HIT, 0x20, 0x100, 0x80000000,
                    F.RT_FLAG_COUNTERS | F.RT_FLAG_KERNEL_TIMES, F.RT_FLAG_SPECULAR | F.RT_FLAG_ASYNC):
            assert f(params(flags=bad)) == F.RT_ERR_INVALID and "flag bits" in err() and err().startswith(names[f] + ": "), bad
        # ... every combination of the three falls through to the scene
        for c in range(8):
            good = (F.RT_FLAG_COUNTERS if c & 1 else 0) | (F.RT_FLAG_SURFACES if c & 2 else 0) | (F.RT_FLAG_SPECULAR if c & 4 else 0)
            assert f(params(flags=good)) == F.RT_ERR_INVALID and err() == names[f] + ": null scene", good
        # n_rays > 2^40 (the rays are not read: the length is refused first)
        kw = {"rays_": 4096, "out_": 8192} if f is host else {}
        assert f(params(), n=(1 << 40) + 1, **kw) == F.RT_ERR_INVALID and err() == names[f] + ": n_rays too large"
        assert f(params(), n=1 << 40, **kw) == F.RT_ERR_INVALID and "null scene" in err()
        # max_depth is ignored
        for depth in (0, 1, 0xFFFFFFFF):
            assert f(params(max_depth=depth)) == F.RT_ERR_INVALID and "null scene" in err()
    # a device buffer that is not 16-byte aligned
    for off in (1, 4, 8):
        assert device(params(), rays_=4096 + off) == F.RT_ERR_INVALID and err() == "rt_features_rays_device: the ray buffer must be 16-byte aligned"
        assert device(params(), out_=8192 + off) == F.RT_ERR_INVALID and err() == "rt_features_rays_device: the output must be 16-byte aligned"
    assert device(params(), rays_=4096 + 16, out_=8192 + 48) == F.RT_ERR_INVALID and "null scene" in err()
    assert device(params(), rays_=4096 + 8, out_=8192 + 8, n=0) == F.RT_ERR_INVALID and "null scene" in err()       # (nothing to align)
    assert np.all(out == 7.0)                                                   # nothing was written


def test_no_rays_and_no_samples_need_no_device(rt):
    """n_rays == 0 is RT_OK with nothing written; spp == 0 is RT_OK with zeros (host form: no device call at all, so a scene
    that is only a non-null handle will do — it is never dereferenced on these paths)."""
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    st = F.rt_stats()
    host, device, out, keep = callers(rt, st)
    handle = C.create_string_buffer(4096)                                       # (stands in for a scene: not touched)
    scene = C.cast(handle, C.c_void_p)
    p = rt.radiance_params(spp=2, background=(0.1, 0.2, 0.3), flags=F.RT_FLAG_COUNTERS | F.RT_FLAG_SPECULAR)
    st.paths = st.rays = st.rng_draws = 99
    assert host(p, rays_=None, n=0, out_=None, scene=scene) == F.RT_OK
    assert st.paths == 0 and st.rays == 0 and st.rng_draws == 0 and np.all(out == 7.0)
    assert host(p, n=0, scene=scene) == F.RT_OK and np.all(out == 7.0)          # buffers given, still nothing written
    assert device(p, rays_=None, n=0, out_=None, scene=scene) == F.RT_OK
    p.spp = 0
    st.paths = st.rays = st.rng_draws = 99
    assert host(p, n=3, scene=scene) == F.RT_OK
    assert st.paths == 0 and st.rays == 0 and st.rng_draws == 0 and st.ms == 0
    assert not out[:24].view(np.uint8).any() and np.all(out[24:] == 7.0)        # three records of zeros, no more
    p.flags = F.RT_FLAG_ANY_HIT                                                 # ... but a bad flag is still a bad flag
    assert host(p, n=3, scene=scene) == F.RT_ERR_INVALID


def test_radiance_still_refuses_the_feature_flags(rt):
    from raytracer_2022_amd import _ffi as F
    L = rt.lib()
    rays = rt.radiance_rays((0, 0, 5), [(0, 0, -1)] * 4)
    out = np.full(12, 7.0)
    for flag in (F.RT_FLAG_SURFACES, F.RT_FLAG_SPECULAR, F.RT_FLAG_COUNTERS | F.RT_FLAG_SPECULAR):
        p = rt.radiance_params(spp=2, flags=flag)
        assert L.rt_radiance(None, rays.ctypes.data, 4, C.byref(p), out.ctypes.data, None) == F.RT_ERR_INVALID
        assert "flag" in L.rt_last_error().decode()
        assert L.rt_radiance_device(None, 4096, 4, C.byref(p), 8192, None, None) == F.RT_ERR_INVALID
        assert "flag" in L.rt_last_error().decode()
    assert np.all(out == 7.0)
