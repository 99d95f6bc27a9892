"""The CPU side of rt_features_rays*: the restatement by oracle calls (tests/features_rays_ref.py) held to the oracle itself —
to rto_ray_color on a scene of specular surfaces only, to features_ref's camera composition on media-free builders, and to
rto_hit's own word count inside a medium. No GPU."""
import numpy as np
import pytest

from raytracer_2022_amd import _ffi as F

import features_rays_ref as R
import specular_ref as SP
from compare import assert_same_bits
from features_ref import Seen, oracle_sample


def test_python_arguments(rt):
    """The two methods take what the reference here is called with: rays, spp, background, t_min and the two flags."""
    import inspect
    host = inspect.signature(rt.DeviceScene.features_rays).parameters
    assert list(host)[:2] == ["self", "rays"] and host["spp"].default == 1 and host["t_min"].default == 0.001
    assert tuple(host["background"].default) == (0.0, 0.0, 0.0) and host["want_stats"].default is False
    device = inspect.signature(rt.DeviceScene.features_rays_device).parameters
    assert list(device)[:5] == ["self", "d_rays_ptr", "n", "d_out_ptr", "params"] and device["stream_ptr"].default is None
    for sig in (host, device):
        assert sig["surfaces"].default is False and sig["specular"].default is False
    assert "max_depth" not in host                                               # ignored by the call: not offered


# ---- (a) the flagged albedo of a sample IS ray_color of that sample ----------------------------------------------------------
def test_mirror_hall_albedo_is_ray_color(rt, O):
    b, d, rays, p = R.hall_case(rt, O)
    ref, st, info = R.oracle_features_rays(O, d, rays, p, specular=True)
    n = len(rays) * p.spp
    lengths = np.bincount(info.lengths.reshape(-1), minlength=SP.BOUNCES + 1)
    print("chain lengths 0..8:", lengths.tolist(), "ended by the cap:", int(info.capped.sum()), "of", n)
    assert len(lengths) == SP.BOUNCES + 1 and (lengths > 0).all(), lengths       # every chain length from 0 up to the cap
    assert info.capped.any() and not info.capped.all()                           # capped and uncapped samples both occur
    assert info.segments == int((info.lengths + 1).sum())
    key = O.lib().rto_path_key
    checked, words, rays_traced = 0, 0, 0
    for i, r in enumerate(rays):
        for s in range(p.spp):
            if info.capped[i, s]:
                continue
            st1 = F.rt_stats()
            rgb = O.ray_color(d, r["origin"], r["direction"], tm=float(r["time"]), background=p.background, t_min=p.t_min, depth=50,
                              rng_state=key(int(r["rng_state"]), 0, 0, s), stats=st1)
            assert_same_bits(info.samples[i, s, :3], np.array(rgb), ("albedo against ray_color", i, s))
            assert st1.rays == info.lengths[i, s] + 1
            words += st1.rng_draws
            rays_traced += st1.rays
            checked += 1
    assert checked == n - info.capped.sum() > 0
    # the words of the uncapped chains are ray_color's: with none capped the two totals would be equal
    assert words <= info.words and rays_traced == int((info.lengths + 1)[~info.capped].sum())
    # depth and hits are primary visibility: the unflagged reference's
    first, _, info0 = R.oracle_features_rays(O, d, rays, p)
    assert_same_bits(ref["depth"], first["depth"], "depth")
    assert_same_bits(ref["hits"], first["hits"], "hits")
    assert np.any(ref["albedo"] != first["albedo"]) and np.any(ref["normal"] != first["normal"])
    assert info0.words == 0 and info0.segments == n                              # no medium, no camera: nothing is drawn


# ---- (b) the ray rt_features aims gives rt_features' record ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_box", "random_scene"])
def test_aimed_ray_gives_the_camera_record(rt, O, name):
    W, H = 12, 8
    s = rt.HostScene(name, seed=2022)
    d = s.desc
    assert d.n_media == 0
    cam, bg = s.default_view(W / H)
    if name == "random_scene":                                                   # an open shutter and a lens
        cam = rt.camera_new((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.3, 10.0, 0.0, 1.0)
    p = rt.make_params(W, H, 1, 50, bg, seed=5, n_frames=2)
    pixels = [(frame, py, px) for frame in range(2) for py in range(H) for px in range(W)]
    rays = R.aimed_rays(rt, O, cam, p, pixels, np.random.default_rng(3))
    rp = rt.radiance_params(1, bg, p.t_min, 0)
    ref, st, info = R.oracle_features_rays(O, d, rays, rp)
    st_cam, seen = F.rt_stats(), Seen()
    want = np.array([oracle_sample(O, d, cam, p, px, py, frame, 0, st_cam, seen) for frame, py, px in pixels], dtype=np.float64)
    assert_same_bits(ref.view(np.float64).reshape(-1, 8), 0.0 + want, name)
    assert st.as_dict() == st_cam.as_dict() and info.kinds == seen.kinds
    assert info.words == 0 and seen.draws >= 2 * len(pixels)                     # the camera's words are the camera's
    assert 0 < ref["hits"].sum()


# ---- (c) a medium draws, and only the hits draw --------------------------------------------------------------------------------
def test_cornell_smoke_samples_differ_and_only_the_hits_draw(rt, O):
    W, H = 12, 8
    s = rt.HostScene("cornell_smoke", seed=2022)
    d = s.desc
    cam, bg = s.default_view(W / H)
    p = rt.make_params(W, H, 1, 50, bg, seed=5)
    rays = R.aimed_rays(rt, O, cam, p, [(0, py, px) for py in range(H) for px in range(W)], np.random.default_rng(4))
    rp = rt.radiance_params(2, bg, p.t_min, 0)
    ref, st, info = R.oracle_features_rays(O, d, rays, rp)
    differ = np.any(info.samples[:, 0] != info.samples[:, 1], axis=1)
    assert differ.any() and not differ.all()                                     # the medium draws; a wall beside it does not
    # rng_draws is what rto_hit reports, ray by ray and sample by sample
    key = O.lib().rto_path_key
    words = 0
    for r in rays:
        for smp in range(2):
            rec = O.hit(d, d.root, r["origin"], r["direction"], tm=float(r["time"]), t_min=rp.t_min, t_max=R.F64_MAX,
                        rng_state=key(int(r["rng_state"]), 0, 0, smp))
            words += rec.rng_draws
    assert info.words == info.medium_words == words > 0
    # looked through: nothing draws, all samples of a ray are equal, and the fog is gone from the records
    surf, _, info_s = R.oracle_features_rays(O, d, rays, rp, surfaces=True)
    assert info_s.words == 0 and np.array_equal(info_s.samples[:, 0], info_s.samples[:, 1])
    assert surf.tobytes() != ref.tobytes()
    assert_same_bits(surf[~differ]["hits"], ref[~differ]["hits"])
