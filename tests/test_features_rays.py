"""Feature buffers of caller rays (rt_features_rays*) against the CPU oracle, bit for bit.

The reference is tests/features_rays_ref.py: rto_path_key(rng_state, 0, 0, s) -> rto_hit -> the material rule, under
RT_FLAG_SPECULAR specular_ref.chain_from from the caller's ray, under RT_FLAG_SURFACES on surface_ref's looked-through copy.
Every record is compared on the uint64 view of its doubles (NaN where the reference has NaN), every counter with the
reference's. What a batch shows — hits and misses, both faces, media draws, chains — is asserted on the reference."""
import os

import numpy as np
import pytest

from raytracer_2022_amd import _ffi as F

import denoise_ref as DN
import features_rays_ref as R
import specular_ref as SP
import trace_scenes as TS
from compare import assert_same_bits
from features_ref import BUILDERS
from gpu_first import torch_first  # noqa: F401
from query_scenes import every_kind_scene

pytestmark = pytest.mark.gpu

ASSETS_SMALL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "assets_small")
FLAGS = R.FLAGS
M = 4099                                                   # the base batch past the grid: distinct rays, a prime


def check(rt, O, dev, d, rays, spp, flags="first hit", background=(0.25, 0.5, 0.75), t_min=0.001, ref=None, what=""):
    """The counting and the plain instance of one flag combination against the reference -> (records, reference triple)."""
    surfaces, specular = FLAGS[flags]
    p = rt.radiance_params(spp, background, t_min, 0)
    ref = ref or R.oracle_features_rays(O, d, rays, p, surfaces, specular)
    records, st_ref, info = ref
    got, st = dev.features_rays(rays, spp, background, t_min, want_stats=True, surfaces=surfaces, specular=specular)
    assert got.shape == (len(rays),) and got.dtype == F.FEATURE_DTYPE
    assert_same_bits(got, records, (what, flags, "counter instance"))
    R.check_counters(st, st_ref, info, len(rays) * spp, d, surfaces, specular)
    plain = dev.features_rays(rays, spp, background, t_min, surfaces=surfaces, specular=specular)
    assert_same_bits(plain, records, (what, flags, "plain instance"))
    return got, ref


# ---- 1. every scene builder --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BUILDERS)
def test_every_scene_builder(rt, O, name):
    s = rt.HostScene(name, seed=2022, assets_dir=ASSETS_SMALL if name in ("wwscene", "earth") else None)
    d = s.desc
    cam, bg = s.default_view(1.5)
    rays = R.mixed_batch(rt, O, d, cam, 300, seed=len(name))
    assert 200 <= len(rays) <= 300
    dev = rt.DeviceScene(d)
    got, (ref, st_ref, info) = check(rt, O, dev, d, rays, 3, background=tuple(bg), what=name)
    hits = ref["hits"]
    assert (hits > 0).sum() > 20 and (hits == 0).any()                           # hits and misses
    assert {front for _, _, front in info.kinds} == {True, False}               # both faces
    assert info.segments == 3 * len(rays) and (info.words > 0) == (d.n_media > 0)     # the media draw, and only they
    dev.close()


# ---- 2. every shape of trav_dispatch -----------------------------------------------------------------------------------------
def shape_scene(rt, which):
    if which == "every_kind":
        b, d, cam = every_kind_scene(rt)
        return b, d, cam, None
    need = int(which.split()[1])
    d, cam, _, _ = TS.stack_need_scene(need)
    return d, d, cam, need


@pytest.mark.parametrize("which", ["need 16", "need 22", "need 30", "need 64", "every_kind"])
def test_every_traversal_shape_under_every_flag(rt, O, which):
    keep, d, cam, need = shape_scene(rt, which)
    dev = rt.DeviceScene(d)
    assert need is None or dev.info()["stack_need"] == need
    rays = R.mixed_batch(rt, O, d, cam, 240, seed=len(which))
    first = None
    for flags in FLAGS:
        got, (ref, _, info) = check(rt, O, dev, d, rays, 2, flags, what=which)
        first = ref if first is None else first
        assert (ref["hits"] > 0).sum() > 10 and (ref["hits"] == 0).any()
        if which == "every_kind" and flags != "first hit":
            assert ref.tobytes() != first.tobytes()                               # a medium to look through, glass to follow
    dev.close()


# ---- 3. the flags ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_smoke", "final_scene"])
def test_surfaces_against_the_looked_through_copy(rt, O, name):
    s = rt.HostScene(name, seed=2022)
    d = s.desc
    cam, bg = s.default_view(1.5)
    rays = R.aimed_rays(rt, O, cam, rt.make_params(24, 16, 1, 50, bg, seed=3), [(0, py, px) for py in range(16) for px in range(24)],
                        np.random.default_rng(8))
    dev = rt.DeviceScene(d)
    _, (first, _, info0) = check(rt, O, dev, d, rays, 3, "first hit", tuple(bg), what=name)
    got, (ref, _, info) = check(rt, O, dev, d, rays, 3, "surfaces", tuple(bg), what=name)
    assert info0.words > 0 and info.words == 0 and ref.tobytes() != first.tobytes()
    _, st = dev.features_rays(rays, 3, tuple(bg), want_stats=True, surfaces=True)
    assert st.prim_tests[F.RT_KIND_MEDIUM] == 0 and st.rng_draws == 0
    dev.close()


def test_specular_on_the_mirror_hall_and_the_radiance_identity(rt, O):
    """RT_FLAG_SPECULAR with its counters, and identity (a): on a scene of specular surfaces, lights and background only, the
    flagged albedo of a ray whose chains are all uncapped is rt_radiance's sum of that ray, bit for bit."""
    b, d, rays, p = R.hall_case(rt, O)
    dev = rt.DeviceScene(d)
    got, (ref, _, info) = check(rt, O, dev, d, rays, p.spp, "specular", SP.HALL_BACKGROUND, what="mirror hall")
    lengths = np.bincount(info.lengths.reshape(-1), minlength=SP.BOUNCES + 1)
    assert (lengths > 0).all() and info.capped.any()
    check(rt, O, dev, d, rays, p.spp, "surfaces and specular", SP.HALL_BACKGROUND, what="mirror hall")
    uncapped = ~info.capped.any(axis=1)
    assert 100 < uncapped.sum() < len(rays)
    sums = dev.radiance(rays, p.spp, SP.HALL_BACKGROUND, p.t_min, max_depth=50)
    assert_same_bits(got["albedo"][uncapped], sums[uncapped], "identity (a)")
    assert np.any(got["albedo"][~uncapped] != sums[~uncapped])                   # ... and a capped chain is not ray_color
    dev.close()


def test_specular_on_random_scene(rt, O):
    s = rt.HostScene("random_scene", seed=2022)
    cam, bg = s.default_view(1.5)
    rays = R.mixed_batch(rt, O, s.desc, cam, 300, seed=4)
    dev = rt.DeviceScene(s.desc)
    _, (first, _, _) = check(rt, O, dev, s.desc, rays, 3, "first hit", tuple(bg))
    _, (ref, _, info) = check(rt, O, dev, s.desc, rays, 3, "specular", tuple(bg))
    assert (info.lengths > 0).sum() > 30 and ref.tobytes() != first.tobytes()
    assert_same_bits(ref["depth"], first["depth"])                               # primary visibility stays
    dev.close()


def test_flags_change_nothing_where_nothing_is_looked_through_or_followed(rt, O):
    s = rt.HostScene("cornell_box", seed=2022)
    d = s.desc
    assert d.n_media == 0 and not any(SP.followed(d.materials[i]) for i in range(d.n_materials))
    cam, bg = s.default_view(1.0)
    rays = R.mixed_batch(rt, O, d, cam, 300, seed=2)
    dev = rt.DeviceScene(d)
    want, st0 = dev.features_rays(rays, 3, tuple(bg), want_stats=True)
    count = lambda st: {k: v for k, v in st.as_dict().items() if k not in ("ms", "trace_ms", "shade_ms")}
    assert st0.paths == st0.rays == 3 * len(rays) and st0.rng_draws == 0
    for flags, (surfaces, specular) in FLAGS.items():
        got, st = dev.features_rays(rays, 3, tuple(bg), want_stats=True, surfaces=surfaces, specular=specular)
        assert_same_bits(got, want, flags)
        assert count(st) == count(st0), flags
    dev.close()


# ---- 4. identity (b): the ray rt_features aims ---------------------------------------------------------------------------------
def test_aimed_rays_give_the_features_of_the_view(rt, O):
    W, H = 24, 16
    s = rt.HostScene("cornell_box", seed=2022)
    cam, bg = s.default_view(W / H)
    p = rt.make_params(W, H, 1, 50, bg, seed=9, n_frames=2)
    rows = np.arange(2 * H, dtype=np.uint32)
    dev = rt.DeviceScene(s.desc)
    whole = dev.features(cam, p, rows).reshape(-1)
    rays = R.aimed_rays(rt, O, cam, p, [(g // H, g % H, px) for g in rows for px in range(W)], np.random.default_rng(1))
    assert_same_bits(dev.features_rays(rays, 1, tuple(bg), p.t_min), whole, "identity (b)")
    assert 0 < (whole["hits"] == 0).sum() < whole.size
    dev.close()


# ---- 5. order and length --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [1, 5])
def test_lengths_and_orders(rt, O, spp):
    s = rt.HostScene("cornell_smoke", seed=2022)
    d = s.desc
    cam, bg = s.default_view(1.0)
    base = R.mixed_batch(rt, O, d, cam, 300, seed=7)
    dev = rt.DeviceScene(d)
    p = rt.radiance_params(spp, bg, 0.001, 0)
    ref, _, info = R.oracle_features_rays(O, d, base, p)
    assert info.words > 0
    g = np.random.default_rng(spp)
    for n in (1, 63, 64, 65, 4099):
        idx = g.integers(0, len(base), n)                                        # (with repeats)
        got = dev.features_rays(base[idx], spp, tuple(bg))
        assert got.shape == (n,)
        assert_same_bits(got, ref[idx], "length %d" % n)
        perm = g.permutation(n)
        assert_same_bits(dev.features_rays(base[idx][perm], spp, tuple(bg)), got[perm], "shuffled, length %d" % n)
    empty, st = dev.features_rays(base[:0], spp, tuple(bg), want_stats=True)
    assert empty.shape == (0,) and st.paths == 0 and st.rays == 0
    zeros, st = dev.features_rays(base[:5], 0, tuple(bg), want_stats=True)
    assert not zeros.view(np.uint8).any() and st.paths == 0 and st.rays == 0
    dev.close()


# ---- 6. hostile rays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ["first hit", "specular"])
def test_hostile_rays(rt, O, flags):
    """Rays no camera makes: zero direction components, a zero direction, +-inf and NaN components, origins inside the medium's
    boundary, inside the dielectric ball and inside the box, huge origins. (RT_FLAG_SURFACES is not held to these rays: its
    reference, the looked-through copy, is the definition only while every distance inside a boundary is finite.)"""
    _, d, _ = every_kind_scene(rt)
    dev = rt.DeviceScene(d)
    rays = []
    for o in [(0, 1, 8), (0.0, 0.5, 0.0), (4.5, 0.5, 2.0), (-4, 1, 2), (-2.5, 1, 0), (0, 0, 0), (0, 3, 0)]:
        for dv in [(0, 0, -1), (0, -1, 0), (1, 0, 0), (0, 0, 1), (0, 0, 0), (1e-300, 0, -1), (-0.0, -1, 0), (np.nan, 0, -1),
                   (0, np.nan, 0), (np.inf, 0, 0), (-np.inf, 1, 0), (1, 1, 1), (0, 1, 0)]:
            rays.append((o, dv))
    rays += [((np.nan, 0, 0), (0, 0, -1)), ((0, np.inf, 0), (0, -1, 0)), ((1e308, 0, 0), (-1, 0, 0)), ((1e300, 1, 1e300), (-1, 0, -1))]
    r = np.concatenate([rt.radiance_rays(o, dv, time=0.3, rng_state=1000 + i) for i, (o, dv) in enumerate(rays)])
    got, (ref, _, info) = check(rt, O, dev, d, r, 3, flags, (0.5, 0.5, 0.5), what="hostile")
    v = ref.view(np.float64)
    assert np.isnan(v).any() and np.isfinite(v).any() and info.words > 0
    dev.close()


# ---- 7. past the grid ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_cases(rt, O):
    """which -> (scene, desc, device scene, the M base rays, reference(flags)): built on first use, computed once, never changed."""
    made = {}

    def get(which):
        if which not in made:
            if which == "mirror hall":                                           # a tiny stack, and chains of every length
                keep, d, cam, _ = SP.mirror_hall(rt)
                bg = SP.HALL_BACKGROUND
            else:
                keep = rt.HostScene(which, seed=2022)
                d = keep.desc
                cam, bg = keep.default_view(1.5)
            rays = R.mixed_batch(rt, O, d, cam, 3 * 1500, seed=len(which))
            rays = rays[:M] if len(rays) >= M else np.concatenate([rays, R.mixed_batch(rt, O, d, cam, 600, seed=1)])[:M]
            assert len(rays) == M and len(np.unique(rays["rng_state"])) == M
            p = rt.radiance_params(2, bg, 0.001, 0)
            refs = {}

            def reference(flags):
                if flags not in refs:
                    refs[flags] = R.oracle_features_rays(O, d, rays, p, *FLAGS[flags])
                return refs[flags]
            made[which] = (keep, d, rt.DeviceScene(d), np.ascontiguousarray(rays), tuple(bg), reference)
        return made[which]
    yield get
    for case in made.values():
        case[2].close()


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("which", ["mirror hall", "final_scene"])
def test_ray_lists_beyond_one_grid(rt, grid_cases, which, flags):
    """test_beyond_one_grid's recipe: no persistent grid has more than L = CUs x 2048 lanes, so a call of more than 2 L rays makes
    some lane take a third ray and most a second — f_take's split of the entry index, f_add's first-sample branch on a lane that
    has written another record. K permutations of M distinct rays, concatenated: successive items of a lane differ."""
    import torch
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 2048
    keep, d, dev, base, bg, reference = grid_cases(which)
    surfaces, specular = FLAGS[flags]
    assert which != "mirror hall" or dev.info()["stack_need"] <= 16             # (the tiny-stack instances)
    ref, st_ref, info = reference(flags)
    assert (ref["hits"] > 0).sum() > 100 and (ref["hits"] == 0).any()
    if which == "final_scene":
        assert reference("first hit")[2].words > 0 and (reference("specular")[2].lengths > 0).sum() > 30
    else:
        assert (np.bincount(reference("specular")[2].lengths.reshape(-1), minlength=SP.BOUNCES + 1) > 0).all()
    k = (2 * lanes + 1 + M - 1) // M
    g = np.random.default_rng(k + len(flags))
    idx = np.concatenate([g.permutation(M) for _ in range(k)])
    assert idx.size == k * M > 2 * lanes
    rays = base[idx]
    got, st = dev.features_rays(rays, 2, bg, want_stats=True, surfaces=surfaces, specular=specular)
    assert_same_bits(got, ref[idx], (which, flags, "counter instance"))
    R.check_counters(st, st_ref, info, M * 2, d, surfaces, specular, k=k)
    assert_same_bits(dev.features_rays(rays, 2, bg, surfaces=surfaces, specular=specular), ref[idx], (which, flags, "plain instance"))


# ---- 8. torch buffers, streams and engines -----------------------------------------------------------------------------------
def test_torch_buffers_beside_an_asynchronous_render_and_either_engine(rt, O):
    import torch
    W, H, spp = 24, 16, 3
    s = rt.HostScene("final_scene", seed=2022)
    cam, bg = s.default_view(W / H)
    p = rt.make_params(W, H, spp, 50, bg, seed=2022, spp_chunk=1)
    dev = rt.DeviceScene(s.desc)
    rows = rt.shuffled_rows(H, 3)
    rays = R.mixed_batch(rt, O, s.desc, cam, 600, seed=12)
    n = len(rays)
    rp = rt.radiance_params(spp, bg, 0.001, 50)
    want = dev.features_rays(rays, spp, tuple(bg))
    ref_render = dev.render(cam, p, rows)
    a_stream, b_stream = torch.cuda.Stream(), torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.float64).copy()).cuda()
    d_out = torch.full((n * 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")
    d_copy = torch.zeros_like(d_out)
    torch.cuda.synchronize()
    dev.features_rays_device(d_rays.data_ptr(), n, d_out.data_ptr(), rp, b_stream.cuda_stream)      # stats=None: enqueued, not waited for
    with torch.cuda.stream(b_stream):
        d_copy.copy_(d_out, non_blocking=True)                                   # a dependent copy behind the call, same stream
    b_stream.synchronize()
    out = d_copy.cpu().numpy()
    assert_same_bits(out[: n * 8].view(F.FEATURE_DTYPE), want, "non-default stream")
    assert np.isnan(out[n * 8:]).all()                                           # nothing past the last record
    st = F.rt_stats()
    d_out.fill_(float("nan"))
    torch.cuda.synchronize()
    dev.features_rays_device(d_rays.data_ptr(), n, d_out.data_ptr(), rp, b_stream.cuda_stream, stats=st)
    assert_same_bits(d_out.cpu().numpy()[: n * 8].view(F.FEATURE_DTYPE), want, "with stats")      # (the call has synchronised)
    assert st.paths == st.rays == n * spp and st.node_visits > st.rays and st.rng_draws > 0 and st.ms > 0
    # beside an RT_FLAG_ASYNC render of the same scene on another stream
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    image = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda")
    feats = [torch.full((n * 8,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    dev.render_device(cam, p, d_rows.data_ptr(), H, image.data_ptr(), a_stream.cuda_stream, None, asynchronous=True)
    for k, f_ in enumerate(feats):
        dev.features_rays_device(d_rays.data_ptr(), n, f_.data_ptr(), rp, b_stream.cuda_stream, specular=k == 2)
    b_stream.synchronize()
    dev.wait(a_stream.cuda_stream)
    assert np.array_equal(image.cpu().numpy().view(np.uint64), ref_render.view(np.uint64))
    for f_ in feats[:2]:
        assert_same_bits(f_.cpu().numpy().view(F.FEATURE_DTYPE), want, "beside a render")
    assert_same_bits(feats[2].cpu().numpy().view(F.FEATURE_DTYPE), dev.features_rays(rays, spp, tuple(bg), specular=True), "specular, beside a render")
    assert np.array_equal(dev.render(cam, p, rows).view(np.uint64), ref_render.view(np.uint64))         # the render's workspace is untouched
    # the call uses neither engine
    dev.set_engine("mega")
    assert_same_bits(dev.features_rays(rays, spp, tuple(bg)), want, "megakernel engine selected")
    dev.close()


# ---- 9. what it is for -------------------------------------------------------------------------------------------------------
def test_a_panorama_is_denoised_with_its_ray_features(rt):
    """A 96 x 48 equirectangular panorama from the centre of the Cornell box, a camera rt_camera cannot describe: rt_radiance at
    8 spp, rt_features_rays of the same rays, rt_denoise. Against the same rays at 512 spp the filtered display values are closer
    than the unfiltered ones. (On the CPU — the oracle's radiance, features_rays_ref's records, denoise_ref.restate — the same
    inequality: MSE 0.017310 before, 0.001228 after.)"""
    W, H, spp, spp_ref = 96, 48, 8, 512
    s = rt.HostScene("cornell_box", seed=2022)
    _, bg = s.default_view(1.0)
    dev = rt.DeviceScene(s.desc)
    rays = R.equirect_rays(rt, (278.0, 278.0, 278.0), W, H)
    far = rays.copy()
    far["rng_state"] += np.uint64(1 << 32)                                       # the reference draws from streams of its own
    noisy = dev.radiance(rays, spp, tuple(bg))
    feat = dev.features_rays(rays, spp, tuple(bg))
    truth = dev.radiance(far, spp_ref, tuple(bg))
    assert 0 < (feat["hits"] == 0).sum() < W * H // 4                            # the box is open towards -z: those rays see the background
    clean = rt.denoise(noisy.reshape(H, W, 3), feat.reshape(H, W), rt.denoise_params(W, H, spp))
    want = DN.display(truth, spp_ref).reshape(H, W, 3)
    before = float(np.mean((DN.display(noisy, spp).reshape(H, W, 3) - want) ** 2))
    after = float(np.mean((DN.display(clean, spp) - want) ** 2))
    print("panorama MSE of display values against %d spp: %.6f before the filter, %.6f after" % (spp_ref, before, after))
    assert after < before
    dev.close()
