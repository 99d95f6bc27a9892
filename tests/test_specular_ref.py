"""The CPU side of RT_FLAG_SPECULAR: the restatement by oracle calls (tests/specular_ref.py) held to rto_ray_color on a scene
of specular surfaces only, to the first-hit composition on scenes without followed materials, and the flag check of every
entry point. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from raytracer_2022_amd import _ffi as F

import specular_ref as SP
from compare import assert_same_bits
from features_ref import oracle_features

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt2022.h")
UNFOLLOWED = ["cornell_box", "cornell_smoke", "earth", "simple_light", "two_perlin_spheres", "two_spheres"]


def test_constants_match_the_header():
    text = open(HEADER).read()
    assert re.search(r"#define RT_FLAG_SPECULAR 0x40u", text) and F.RT_FLAG_SPECULAR == 0x40
    assert re.search(r"#define RT_FEATURE_SPECULAR_BOUNCES 8\b", text) and F.RT_FEATURE_SPECULAR_BOUNCES == 8
    assert "#define RT2022_ABI_VERSION 3" in text and F.RT2022_ABI_VERSION == 3
    flags = [F.RT_FLAG_COUNTERS, F.RT_FLAG_KERNEL_TIMES, F.RT_FLAG_ASYNC, F.RT_FLAG_ANY_HIT, F.RT_FLAG_SURFACES, F.RT_FLAG_SPECULAR]
    assert sorted(flags) == [1, 2, 4, 8, 16, 64]             # one bit each; 0x20 stays "not a flag"


# ---- (a) the flagged albedo of a sample IS ray_color of that sample ----------------------------------------------------------
@pytest.fixture(scope="module")
def hall(rt, O):
    b, d, cam, p = SP.mirror_hall(rt)
    ref, st, info = SP.oracle_specular_features(O, d, cam, p, np.arange(SP.HALL_H, dtype=np.uint32))
    return b, d, cam, p, ref, st, info


def test_mirror_hall_albedo_is_ray_color(O, hall):
    b, d, cam, p, ref, st, info = hall
    n = SP.HALL_W * SP.HALL_H * SP.HALL_SPP
    lengths = np.bincount(info.lengths.reshape(-1), minlength=SP.BOUNCES + 1)
    print("chain lengths 0..8:", lengths.tolist(), "ended by the cap:", int(info.capped.sum()), "of", n)
    assert len(lengths) == SP.BOUNCES + 1 and (lengths >= 20).all(), lengths
    assert info.capped.sum() <= 0.02 * n
    assert len(info.samples) == n and info.segments == int((info.lengths + 1).sum())
    checked = 0
    for r in info.samples:
        if r.capped:
            continue
        st1 = F.rt_stats()
        rgb = O.ray_color(d, r.ray0[:3], r.ray0[3:6], r.ray0[6], p.background, p.t_min, 9, SP.state_after(r.key, r.camera_words), st1)
        assert_same_bits(np.array(r.f[:3]), rgb, ("albedo against ray_color", r.length))
        assert r.words - r.camera_words == st1.rng_draws, (r.length, r.words, r.camera_words, st1.rng_draws)
        assert st1.rays == r.segments
        checked += 1
    assert checked == n - info.capped.sum()
    two_metals = [r for r in info.samples if not r.capped and r.length >= 2]
    assert len(two_metals) > 100
    # depth and hits are primary visibility: the unflagged composition's
    first, _, _ = oracle_features(O, d, cam, p, np.arange(SP.HALL_H, dtype=np.uint32))
    assert_same_bits(ref["depth"], first["depth"], "depth")
    assert_same_bits(ref["hits"], first["hits"], "hits")
    assert np.any(ref["albedo"] != first["albedo"]) and np.any(ref["normal"] != first["normal"])


# ---- (b) nothing to follow: the first-hit composition ------------------------------------------------------------------------
def builder_view(rt, name, W, H, spp):
    s = rt.HostScene(name, seed=2022)
    cam, bg = s.default_view(W / H)
    return s, cam, rt.make_params(W, H, spp, 50, bg, seed=2022)


@pytest.mark.parametrize("name", UNFOLLOWED)
def test_restatement_is_the_first_hit_composition_without_followed_materials(rt, O, name):
    W, H, spp = 24, 16, 2
    s, cam, p = builder_view(rt, name, W, H, spp)
    d = s.desc
    assert not any(SP.followed(d.materials[i]) for i in range(d.n_materials))
    rows = rt.shuffled_rows(H, 3)
    ref, st_ref, seen = oracle_features(O, d, cam, p, rows)
    got, st, info = SP.oracle_specular_features(O, d, cam, p, rows)
    assert_same_bits(got, ref, name)
    assert st.as_dict() == st_ref.as_dict() and info.words == seen.draws and info.segments == W * H * spp
    assert not info.lengths.any() and not info.capped.any()


def test_wwscene_one_pixel(rt, O):
    """wwscene's mesh makes the oracle slow, and some of its small spheres are glass: one pixel whose samples meet none of them."""
    W, H = 12, 8
    s, cam, p = builder_view(rt, "wwscene", W, H, 2)
    rows = np.array([H // 2], dtype=np.uint32)
    ref, st_ref, seen = oracle_features(O, s.desc, cam, p, rows, pixels=[(0, W // 2)])
    got, st, info = SP.specular_pixels(O, s.desc, cam, p, [(0, H // 2, W // 2)])
    assert_same_bits(got, ref, "wwscene")
    assert st.as_dict() == st_ref.as_dict() and info.words == seen.draws and not info.lengths.any()
    assert ref["hits"][0] > 0


@pytest.mark.parametrize("name, least", [("random_scene", 100), ("final_scene", 30)])
def test_builders_with_glass_and_mirrors_are_followed(rt, O, name, least):
    W, H, spp = 24, 16, 2
    s, cam, p = builder_view(rt, name, W, H, spp)
    rows = np.arange(H, dtype=np.uint32)
    got, st, info = SP.oracle_specular_features(O, s.desc, cam, p, rows)
    first, _, _ = oracle_features(O, s.desc, cam, p, rows)
    n_followed = int((info.lengths > 0).sum())
    print(name, "samples followed:", n_followed, "of", W * H * spp)
    assert n_followed >= least
    assert_same_bits(got["depth"], first["depth"], "depth")
    assert_same_bits(got["hits"], first["hits"], "hits")
    same = info.lengths.sum(axis=1) == 0                     # pixels with no followed sample keep their first-hit record
    assert_same_bits(got[same], first[same], "unfollowed pixels")
    assert np.any(got["albedo"][~same] != first["albedo"][~same])


# ---- (c) the flag check, through the library with a null scene ------------------------------------------------------------------
def test_flag_check_of_every_entry_point(rt):
    L = rt.lib()
    err = lambda: L.rt_last_error().decode()
    cam = rt.camera_new((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 5.0, 0.0, 1.0)
    rows = np.arange(4, dtype=np.uint32)
    ids = np.arange(4, dtype=np.uint64)
    out = np.full(16 * 8, 7.0)

    def params(flags):
        p = rt.make_params(4, 4, 2, 50, (0.1, 0.2, 0.3), seed=1, flags=flags)
        p.n_rows, p.row_ids = 4, rows.ctypes.data
        return p

    calls = {
        "rt_features": lambda p, scene=None: L.rt_features(scene, C.byref(cam), C.byref(p), out.ctypes.data, None),
        "rt_features_device": lambda p, scene=None: L.rt_features_device(scene, C.byref(cam), C.byref(p), C.c_void_p(8192), None, None),
        "rt_features_pixels": lambda p, scene=None: L.rt_features_pixels(scene, C.byref(cam), C.byref(p), ids.ctypes.data, 4, out.ctypes.data, None),
        "rt_features_pixels_device": lambda p, scene=None: L.rt_features_pixels_device(scene, C.byref(cam), C.byref(p), C.c_void_p(4096), 4,
                                                                                       C.c_void_p(8192), None, None),
    }
    S_, Cn, Sf = F.RT_FLAG_SPECULAR, F.RT_FLAG_COUNTERS, F.RT_FLAG_SURFACES
    for name, f in calls.items():
        for flags in (S_, S_ | Cn, S_ | Sf, S_ | Cn | Sf):
            p = params(flags)
            if name == "rt_features_device":
                p.row_ids = 4096                            # (a device pointer: only its alignment is looked at)
            assert f(p) == F.RT_ERR_INVALID and err() == name + ": null scene", (name, flags, err())
        for bad in (0x20, 0x100, S_ | F.RT_FLAG_ANY_HIT, S_ | 0x20, S_ | F.RT_FLAG_KERNEL_TIMES, S_ | F.RT_FLAG_ASYNC):
            p = params(bad)
            assert f(p) == F.RT_ERR_INVALID and "flag bits" in err(), (name, bad, err())
    # every other call refuses the bit. (A handle that is no scene where the scene is asked for first: the flag check comes
    # before anything reads it.)
    handle = C.create_string_buffer(4096)
    scene = C.cast(handle, C.c_void_p)
    rgb = np.full(16 * 3, 7.0)
    for flags in (S_, S_ | Cn):
        p = params(flags)
        assert L.rt_render(scene, C.byref(cam), C.byref(p), rgb.ctypes.data_as(C.POINTER(C.c_double)), None) == F.RT_ERR_INVALID and "flag bits" in err()
        assert L.rt_render_device(scene, C.byref(cam), C.byref(p), C.c_void_p(8192), None, None) == F.RT_ERR_INVALID and "flag bits" in err()
        assert L.rt_render_pixels(None, C.byref(cam), C.byref(p), ids.ctypes.data, 4, rgb.ctypes.data, None) == F.RT_ERR_INVALID and "flag bits" in err()
        assert L.rt_render_pixels_device(None, C.byref(cam), C.byref(p), C.c_void_p(4096), 4, C.c_void_p(8192), None, None) == F.RT_ERR_INVALID
        assert "flag bits" in err()
        rays = rt.radiance_rays(np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1)))
        rp = rt.radiance_params(1, (0.1, 0.2, 0.3), flags=flags)
        assert L.rt_radiance(None, rays.ctypes.data, 4, C.byref(rp), rgb.ctypes.data, None) == F.RT_ERR_INVALID and "flag bits" in err()
        assert L.rt_radiance_device(None, C.c_void_p(4096), 4, C.byref(rp), C.c_void_p(8192), None, None) == F.RT_ERR_INVALID and "flag bits" in err()
        q = rt.query_rays(np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1)))
        hits = np.zeros(4, dtype=F.HIT_DTYPE)
        assert L.rt_intersect(scene, q.ctypes.data, 4, flags, hits.ctypes.data, None) == F.RT_ERR_INVALID and "flag bits" in err()
        assert L.rt_intersect_device(scene, C.c_void_p(4096), 4, flags, C.c_void_p(8192), None, None) == F.RT_ERR_INVALID and "flag bits" in err()
    assert np.all(out == 7.0) and np.all(rgb == 7.0)        # nothing was written


def test_python_arguments(rt):
    import inspect
    for name in ("features", "features_device", "features_pixels", "features_pixels_device"):
        sig = inspect.signature(getattr(rt.DeviceScene, name))
        assert sig.parameters["specular"].default is False and sig.parameters["surfaces"].default is False
    assert inspect.signature(rt.render_adaptive).parameters["specular"].default is False
