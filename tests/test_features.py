"""First-hit feature buffers (rt_features / rt_features_device) against the CPU oracle, bit for bit.

The reference value of a sample is a composition of oracle calls: rto_path_key -> rto_rng_f64 (the two jitter draws) ->
rto_get_ray (it returns the words it drew) -> rto_hit on the scene's root from the state key + (2 + draws) * 0x9E3779B97F4A7C15
mod 2^64 (the render's RNG stream, continued) -> the material rule of include/rt2022.h with rto_texture_value. A pixel's
record is 0 + f_0 + f_1 + ... in sample order with plain f64 adds. Every comparison is on the uint64 view of the doubles
(NaN where the oracle has NaN)."""
import ctypes as C
import os

import numpy as np
import pytest

from raytracer_2022_amd import _ffi as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ASSETS = os.path.join(os.path.dirname(HERE), "assets")
BUILDERS = ["cornell_box", "cornell_smoke", "earth", "final_scene", "random_scene", "simple_light", "two_perlin_spheres",
            "two_spheres", "wwscene"]
GOLDEN = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
F64_MAX = float(np.finfo(np.float64).max)
FIELDS = ("albedo", "normal", "depth", "hits")


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """Bring torch's HIP context up before the library's first call, as the other GPU test modules do."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU: the HIP path has no fallback"
    torch.zeros(1, device="cuda")


class Seen:
    """What the oracle composition met: (material kind, texture kind or -1, front_face) of every hit, material indices."""

    def __init__(self):
        self.kinds, self.mats, self.draws, self.medium_draws = set(), set(), 0, 0


def oracle_sample(O, desc, cam, p, px, py, frame, s, st, seen):
    """One sample's (albedo[3], normal[3], depth, hits) by the composition of oracle calls."""
    L = O.lib()
    key = L.rto_path_key(p.seed, frame, py * p.width + px, s)
    uv = (C.c_double * 2)()
    L.rto_rng_f64(key, uv, 2)
    with np.errstate(all="ignore"):
        u = float((np.float64(px) + np.float64(uv[0])) / np.float64(p.width - 1))
        v = float((np.float64(py) + np.float64(uv[1])) / np.float64(p.height - 1))
    ray = (C.c_double * 7)()
    draws = L.rto_get_ray(C.byref(cam), u, v, (key + 2 * GOLDEN) & MASK64, ray)
    rec = O.rto_hit_record()
    L.rto_hit(C.byref(desc), desc.root, ray, p.t_min, F64_MAX, (key + (2 + draws) * GOLDEN) & MASK64, C.byref(rec), C.byref(st))
    seen.draws += 2 + draws + rec.rng_draws
    seen.medium_draws += rec.rng_draws
    if not rec.hit:
        return list(p.background) + [0.0, 0.0, 0.0, 0.0, 0.0]
    m = desc.materials[rec.mat]
    front = bool(rec.front_face)
    tex_kind = desc.textures[m.tex].kind if m.kind in (F.RT_MAT_LAMBERTIAN, F.RT_MAT_ISOTROPIC, F.RT_MAT_DIFFUSE_LIGHT) else -1
    seen.kinds.add((m.kind, tex_kind, front))
    seen.mats.add(rec.mat)
    if m.kind == F.RT_MAT_METAL:
        alb = list(m.albedo)
    elif m.kind == F.RT_MAT_DIELECTRIC:
        alb = [1.0, 1.0, 1.0]
    elif m.kind == F.RT_MAT_DIFFUSE_LIGHT and not front:
        alb = [0.0, 0.0, 0.0]
    else:
        alb = list(O.texture_value(desc, m.tex, rec.u, rec.v, rec.p[:]))
    return alb + list(rec.normal) + [rec.t, 1.0]


def oracle_features(O, desc, cam, params, rows, pixels=None):
    """The reference records of the pixels [(row index, px)] (default: all) → (FEATURE_DTYPE array of len(pixels), summed
    rt_stats of the hits, Seen)."""
    rows = np.asarray(rows, dtype=np.uint32)
    if pixels is None:
        pixels = [(i, px) for i in range(len(rows)) for px in range(params.width)]
    out = np.zeros(len(pixels), dtype=F.FEATURE_DTYPE)
    flat = out.view(np.float64).reshape(len(pixels), 8)
    st, seen = F.rt_stats(), Seen()
    for k, (i, px) in enumerate(pixels):
        g = int(rows[i])
        frame, py = divmod(g, params.height)
        acc = [0.0] * 8
        for s in range(params.spp):
            f = oracle_sample(O, desc, cam, params, int(px), py, frame, s, st, seen)
            acc = [a + float(b) for a, b in zip(acc, f)]               # plain f64 adds, in sample order
        flat[k] = acc
    return out, st, seen


def bits(a):
    a = np.ascontiguousarray(a)
    v = a.view(np.float64) if a.dtype == F.FEATURE_DTYPE else np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(v), np.float64(0), v).view(np.uint64), np.isnan(v)


def assert_same_bits(got, ref, what=""):
    (gb, gn), (rb, rn) = bits(got), bits(ref)
    assert gb.shape == rb.shape, what
    assert np.array_equal(gn, rn), (what, "NaN pattern")
    bad = np.argwhere(gb != rb)
    assert len(bad) == 0, (what, "first differing doubles", bad[:5].tolist(), len(bad))


def check_view(rt, O, desc, cam, params, rows, dev=None, counters=True):
    dev = dev or rt.DeviceScene(desc)
    got, st = dev.features(cam, params, rows, want_stats=True)
    assert got.shape == (len(rows), params.width) and got.dtype == F.FEATURE_DTYPE
    ref, st_ref, seen = oracle_features(O, desc, cam, params, rows)
    assert_same_bits(got.reshape(-1), ref)
    n = len(rows) * params.width * params.spp
    assert st.paths == st.rays == n
    if counters:
        assert st.node_visits == st_ref.node_visits and list(st.prim_tests) == list(st_ref.prim_tests)
        assert st.rng_draws == seen.draws
    assert st.light_pdf_tests == 0 and st.passes == 0 and st.pool_slots == 0 and st.partial_bytes == 0 and st.spp_chunk == 0
    assert st.trace_ms == 0 and st.shade_ms == 0 and st.ms > 0
    plain = dev.features(cam, params, rows)                                # the plain (non-counter) kernel instance
    assert_same_bits(plain.reshape(-1), ref, "plain instance")
    return got, seen, dev


# ---- 1. scene builders ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BUILDERS)
def test_every_scene_builder_matches_the_oracle(rt, O, name):
    W, H, spp = 48, 32, 3
    s = rt.HostScene(name, seed=2022)
    cam, bg = s.default_view(W / H)
    p = rt.make_params(W, H, spp, 50, bg, seed=2022)
    got, seen, _ = check_view(rt, O, s.desc, cam, p, rt.shuffled_rows(H, 2022))
    assert got["hits"].sum() > 100 and got["hits"].max() == spp


# ---- 2. camera draws --------------------------------------------------------------------------------------------------
def every_kind_scene(rt):
    """Every material kind x every texture kind, a back-faced and a flipped light, movers at depth 4, a triangle, a ring,
    media, a moving sphere; no light list (n_lights == 0)."""
    b = rt.DescBuilder()
    g = np.random.default_rng(11)
    vec = g.normal(size=(256, 3))
    vec /= np.linalg.norm(vec, axis=1, keepdims=True)
    pl = b.perlin(vec, g.permutation(256), g.permutation(256), g.permutation(256))
    img = (np.arange(8 * 4 * 3, dtype=np.uint8).reshape(4, 8, 3) * 7) % 251
    textures = lambda: [b.solid((0.7, 0.3, 0.2)), b.checker(b.solid((0.2, 0.3, 0.1)), b.solid((0.9, 0.9, 0.9))), b.noise(pl, 4.0), b.image(img)]
    mats = ([b.lambertian(tex=t) for t in textures()] + [b.diffuse_light(tex=t) for t in textures()] +
            [b.metal((0.8, 0.7, 0.6), 0.3), b.dielectric(1.5)])
    refs = []
    for i, m in enumerate(mats):
        refs.append(b.sphere(((i % 5 - 2) * 1.2, (i // 5) * 1.2, 0.0), 0.45, m))
    glass = b.dielectric(1.5)
    for i, t in enumerate(textures()):                                      # isotropic x every texture: dense media
        refs.append(b.medium(b.sphere(((i - 1.5) * 1.2, 3.6, 0.0), 0.45, glass), 8.0, b.isotropic(tex=t)))
    floor_tex = b.checker(b.noise(pl, 2.0), b.image(img))                   # a checker of a noise and an image
    refs.append(b.rect(F.RT_RECT_XZ, -30, 30, -30, 30, -0.6, b.lambertian(tex=floor_tex)))
    refs.append(b.rect(F.RT_RECT_XZ, -3, 3, -4, 2, 4.3, b.diffuse_light((8, 8, 8))))               # seen from below: back face
    refs.append(b.rect(F.RT_RECT_XY, -6, -3.2, 0, 3, -1.0, b.diffuse_light((4, 5, 6)), flip=True))  # FlipFace ref
    tri_mat, ring_mat, box_mat = b.metal((0.1, 0.9, 0.5), 0.0), b.lambertian((0.9, 0.1, 0.9)), b.lambertian((0.3, 0.6, 0.9))
    refs.append(b.triangle((-4.2, -0.5, 1), (-3.0, -0.5, 1), (-3.6, 0.9, 1.5), tri_mat))
    refs.append(b.translate(b.ring(0.9, 0.3, ring_mat), (3.6, -0.3, 3.0)))
    deep = b.translate(b.rotate_y(b.zoom(b.translate(b.box((-0.4, 0, -0.4), (0.4, 0.8, 0.4), box_mat), (0.1, 0.0, 0.1)), 1.3),
                                  0.5, 0.8660254037844386), (3.8, 1.0, 0.5))
    refs.append(deep)
    mover_mat = b.lambertian((0.5, 0.5, 0.1))
    refs.append(b.moving_sphere((-3.8, 2.2, 0), (-3.8, 3.0, 0), 0, 1, 0.45, mover_mat))
    b.set_root(b.list(refs))
    named = {"triangle": tri_mat, "ring": ring_mat, "box": box_mat, "moving": mover_mat}
    return b, b.desc(), named


def test_lens_and_shutter_draws_on_moving_spheres(rt, O):
    """Aperture > 0 (the lens disk's rejection loop) and time0 < time1 on a scene with a moving sphere and media."""
    b, d, named = every_kind_scene(rt)
    assert d.n_lights == 0 and d.n_moving_spheres == 1
    W, H = 54, 36
    cam = rt.camera_new((0, 1.8, 10), (0, 1.6, 0), (0, 1, 0), 40.0, W / H, 0.4, 10.0, 0.0, 1.0)
    p = rt.make_params(W, H, 3, 50, (0.5, 0.7, 1.0), seed=77)
    got, seen, _ = check_view(rt, O, d, cam, p, rt.shuffled_rows(H, 5))
    assert named["moving"] in seen.mats
    assert seen.draws > 5 * W * H * 3                                       # two jitter words, at least two lens words, the shutter's
    assert seen.medium_draws > 0


@pytest.mark.parametrize("name", ["cornell_smoke", "final_scene"])
def test_medium_draws_follow_the_cameras(rt, O, name):
    """The media of cornell_smoke and of the final scene draw from the camera's stream, after its words."""
    W, H = 40, 40
    s = rt.HostScene(name, seed=2022)
    cam, bg = s.default_view(1.0)
    p = rt.make_params(W, H, 4, 50, bg, seed=9)
    got, seen, _ = check_view(rt, O, s.desc, cam, p, rt.shuffled_rows(H, 1))
    assert seen.medium_draws > 50
    assert any(k[0] == F.RT_MAT_ISOTROPIC for k in seen.kinds)


# ---- 3. material and texture kinds ------------------------------------------------------------------------------------
def test_every_material_and_texture_kind(rt, O):
    b, d, named = every_kind_scene(rt)
    W, H = 60, 40
    cam = rt.camera_new((0, 1.8, 10), (0, 1.6, 0), (0, 1, 0), 40.0, W / H, 0.0, 10.0, 0.0, 1.0)
    p = rt.make_params(W, H, 2, 50, (0.25, 0.5, 0.75), seed=3)
    got, seen, _ = check_view(rt, O, d, cam, p, rt.shuffled_rows(H, 8))
    for mk in (F.RT_MAT_LAMBERTIAN, F.RT_MAT_DIFFUSE_LIGHT, F.RT_MAT_ISOTROPIC):
        for tk in (F.RT_TEX_SOLID, F.RT_TEX_CHECKER, F.RT_TEX_NOISE, F.RT_TEX_IMAGE):
            assert any(k[0] == mk and k[1] == tk for k in seen.kinds), (mk, tk)
    assert (F.RT_MAT_METAL, -1, True) in seen.kinds and (F.RT_MAT_DIELECTRIC, -1, True) in seen.kinds
    assert (F.RT_MAT_DIFFUSE_LIGHT, F.RT_TEX_SOLID, False) in seen.kinds    # a light seen from behind: albedo 0
    for what, m in named.items():
        assert m in seen.mats, what
    assert (got["hits"] == 0).sum() > 0                                     # and some sky


# ---- 4. row list ------------------------------------------------------------------------------------------------------
def test_row_lists_frames_strips_and_orders(rt, O):
    W, H, spp = 40, 30, 2
    s = rt.HostScene("cornell_box", seed=2022)
    cam, bg = s.default_view(W / H)
    dev = rt.DeviceScene(s.desc)
    p2 = rt.make_params(W, H, spp, 50, bg, seed=5, n_frames=2)
    both = np.random.default_rng(4).permutation(2 * H).astype(np.uint32)
    got = dev.features(cam, p2, both)
    for frame in (0, 1):
        rows = np.arange(frame * H, (frame + 1) * H, dtype=np.uint32)
        alone = dev.features(cam, p2, rows)
        where = np.array([int(np.nonzero(both == r)[0][0]) for r in rows])
        assert_same_bits(got[where], alone, "frame %d" % frame)
    p1 = rt.make_params(W, H, spp, 50, bg, seed=5)
    frame0 = dev.features(cam, p1, np.arange(H, dtype=np.uint32))          # n_frames = 1: frame 0 again
    assert_same_bits(frame0, dev.features(cam, p2, np.arange(H, dtype=np.uint32)))
    assert not np.array_equal(bits(frame0)[0], bits(dev.features(cam, p2, np.arange(H, 2 * H, dtype=np.uint32)))[0])    # frame 1 has its own key
    strip = np.array([7, 8, 9, 21], dtype=np.uint32)
    assert_same_bits(dev.features(cam, p1, strip), frame0[strip], "strip")
    order = np.random.default_rng(6).permutation(H).astype(np.uint32)
    assert_same_bits(dev.features(cam, p1, order), frame0[order], "order")
    doubled = np.array([3, 3, 11, 3], dtype=np.uint32)                     # a row may come twice: each entry has its own records
    assert_same_bits(dev.features(cam, p1, doubled), frame0[doubled], "repeated row")
    ref, _, _ = oracle_features(O, s.desc, cam, p2, both, pixels=[(i, px) for i in (0, 17, 59) for px in range(W)])
    assert_same_bits(got[[0, 17, 59]].reshape(-1), ref)


# ---- 5. tie to the render, on the GPU alone ---------------------------------------------------------------------------
def test_render_at_depth_one_sees_the_same_rays(rt):
    """Light-free scene, max_depth = 1: a path that hits returns black, a miss the background, so the render's sum is
    (spp - hits) * background exactly (every addend is representable): render and features aim the same rays."""
    W, H, spp = 64, 48, 4
    s = rt.HostScene("random_scene", seed=2022)
    d = s.desc
    assert d.n_lights == 0 and all(d.materials[i].kind != F.RT_MAT_DIFFUSE_LIGHT for i in range(d.n_materials))
    cam, _ = s.default_view(W / H)
    bg = (0.5, 0.75, 1.0)
    rows = rt.shuffled_rows(H, 12)
    dev = rt.DeviceScene(d)
    feat = dev.features(cam, rt.make_params(W, H, spp, 0, bg, seed=31), rows)       # (max_depth is ignored)
    rgb = dev.render(cam, rt.make_params(W, H, spp, 1, bg, seed=31, spp_chunk=1), rows)
    want = (spp - feat["hits"])[..., None] * np.array(bg)
    assert np.array_equal(rgb, want)
    assert 0 < feat["hits"].sum() < W * H * spp and np.any((feat["hits"] > 0) & (feat["hits"] < spp))


# ---- 6. degenerate sizes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 8), (8, 1), (1, 1)])
def test_one_pixel_wide_or_high_divides_by_zero_like_the_render(rt, O, W, H):
    s = rt.HostScene("cornell_box", seed=2022)
    cam, bg = s.default_view(1.0)
    p = rt.make_params(W, H, 3, 50, (0.1, 0.2, 0.3), seed=2)
    got, seen, _ = check_view(rt, O, s.desc, cam, p, np.arange(H, dtype=np.uint32))
    assert np.isnan(got.view(np.float64)).any() or (got["hits"] == 0).any()


def test_no_samples_and_no_rows(rt):
    s = rt.HostScene("cornell_box", seed=2022)
    cam, bg = s.default_view(1.0)
    dev = rt.DeviceScene(s.desc)
    rows = np.arange(6, dtype=np.uint32)
    got, st = dev.features(cam, rt.make_params(8, 6, 0, 50, bg), rows, want_stats=True)
    assert got.shape == (6, 8) and not got.view(np.uint8).any()
    assert st.paths == 0 and st.rays == 0 and st.ms == 0
    got, st = dev.features(cam, rt.make_params(8, 6, 5, 50, bg), rows[:0], want_stats=True)
    assert got.shape == (0, 8) and st.paths == 0
    import torch
    buf = torch.full((6 * 8 * 8,), 7.0, dtype=torch.float64, device="cuda")
    d_rows = torch.arange(6, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev.features_device(cam, rt.make_params(8, 6, 5, 50, bg), d_rows.data_ptr(), 0, buf.data_ptr())      # n_rows == 0: nothing written
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    dev.features_device(cam, rt.make_params(8, 6, 0, 50, bg), d_rows.data_ptr(), 6, buf.data_ptr())      # spp == 0: zeros
    torch.cuda.synchronize()
    assert bool((buf == 0.0).all())


# ---- 7. buffers -------------------------------------------------------------------------------------------------------
def test_device_variant_on_torch_buffers(rt, O):
    import torch
    W, H, spp = 56, 40, 3
    s = rt.HostScene("final_scene", seed=2022)
    cam, bg = s.default_view(W / H)
    p = rt.make_params(W, H, spp, 50, bg, seed=8)
    rows = rt.shuffled_rows(H, 3)
    dev = rt.DeviceScene(s.desc)
    host = dev.features(cam, p, rows)
    stream = torch.cuda.Stream()
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    d_out = torch.full((H * W * 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev.features_device(cam, p, d_rows.data_ptr(), H, d_out.data_ptr(), stream.cuda_stream)         # stats=None: enqueued, not waited for
    stream.synchronize()
    out = d_out.cpu().numpy()
    assert_same_bits(out[: H * W * 8].view(F.FEATURE_DTYPE), host.reshape(-1))
    assert np.isnan(out[H * W * 8:]).all()                                                          # nothing past the last record
    st = F.rt_stats()
    d_out.fill_(float("nan"))
    torch.cuda.synchronize()
    dev.features_device(cam, p, d_rows.data_ptr(), H, d_out.data_ptr(), stream.cuda_stream, stats=st)
    assert_same_bits(d_out.cpu().numpy()[: H * W * 8].view(F.FEATURE_DTYPE), host.reshape(-1))      # (the call has synchronised)
    assert st.paths == st.rays == W * H * spp and st.node_visits > st.rays and st.rng_draws >= 5 * st.rays and st.ms > 0
    L = rt.lib()
    q = F.rt_params.from_buffer_copy(p)
    q.n_rows, q.row_ids = H, d_rows.data_ptr()
    assert L.rt_features_device(dev._h, C.byref(cam), C.byref(q), d_out.data_ptr() + 8, stream.cuda_stream, None) == F.RT_ERR_INVALID
    assert "16-byte aligned" in L.rt_last_error().decode()
    bad = rows.copy()
    bad[5] = H                                                                                      # a device-resident row id out of range
    d_bad = torch.from_numpy(bad.view(np.int32)).cuda()
    q.row_ids = d_bad.data_ptr()
    assert L.rt_features_device(dev._h, C.byref(cam), C.byref(q), d_out.data_ptr(), stream.cuda_stream, None) == F.RT_ERR_INVALID
    assert "row id out of range" in L.rt_last_error().decode()
    assert_same_bits(dev.features(cam, p, rows), host)                                              # the scene is still fine


# ---- 8. beside an asynchronous render ---------------------------------------------------------------------------------
def test_features_beside_an_asynchronous_render_and_destroy(rt):
    import torch
    W, H, spp = 64, 48, 4
    s = rt.HostScene("final_scene", seed=2022)
    cam, bg = s.default_view(W / H)
    rows = rt.shuffled_rows(H, 3)
    p = rt.make_params(W, H, spp, 50, bg, seed=2022, spp_chunk=1)
    dev = rt.DeviceScene(s.desc)
    ref_render = dev.render(cam, p, rows)
    ref_feat = dev.features(cam, p, rows)
    a_stream, b_stream = torch.cuda.Stream(), torch.cuda.Stream()
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    out = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda")
    feats = [torch.full((H * W * 8,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    dev.render_device(cam, p, d_rows.data_ptr(), H, out.data_ptr(), a_stream.cuda_stream, None, asynchronous=True)
    for f_ in feats:
        dev.features_device(cam, p, d_rows.data_ptr(), H, f_.data_ptr(), b_stream.cuda_stream)
    b_stream.synchronize()
    dev.wait(a_stream.cuda_stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), ref_render.view(np.uint64))
    for f_ in feats:
        assert_same_bits(f_.cpu().numpy().view(F.FEATURE_DTYPE), ref_feat.reshape(-1))
    assert np.array_equal(dev.render(cam, p, rows).view(np.uint64), ref_render.view(np.uint64))     # the render's workspace is untouched
    # destroying the scene with a feature call just enqueued waits for it
    last = torch.full((H * W * 8,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev.features_device(cam, p, d_rows.data_ptr(), H, last.data_ptr(), b_stream.cuda_stream)
    dev.close()
    assert_same_bits(last.cpu().numpy().view(F.FEATURE_DTYPE), ref_feat.reshape(-1))


def test_either_engine_selected(rt):
    """A feature call uses neither engine: the same records with the megakernel selected for renders."""
    s = rt.HostScene("cornell_box", seed=2022)
    cam, bg = s.default_view(1.0)
    p = rt.make_params(32, 32, 2, 50, bg, seed=4)
    rows = rt.shuffled_rows(32, 4)
    dev = rt.DeviceScene(s.desc)
    want = dev.features(cam, p, rows)
    dev.set_engine("mega")
    assert_same_bits(dev.features(cam, p, rows), want)


# ---- 9. headline size -------------------------------------------------------------------------------------------------
def sampled_pixels(n_rows, width, n, seed):
    g = np.random.default_rng(seed)
    return list(zip(g.integers(0, n_rows, n).tolist(), g.integers(0, width, n).tolist()))


def test_headline_frame(rt, O):
    W = H = 800
    spp = 4
    s = rt.HostScene("final_scene", seed=2022)
    cam, bg = s.default_view(1.0)
    p = rt.make_params(W, H, spp, 50, bg, seed=2022)
    rows = rt.shuffled_rows(H, 2022)
    dev = rt.DeviceScene(s.desc)
    whole = dev.features(cam, p, rows)
    halves = np.concatenate([dev.features(cam, p, rows[: H // 2]), dev.features(cam, p, rows[H // 2:])])
    assert_same_bits(whole, halves, "two half strips")
    pixels = sampled_pixels(H, W, 2000, seed=20221)
    ref, _, seen = oracle_features(O, s.desc, cam, p, rows, pixels=pixels)
    got = np.array([whole[i, px] for i, px in pixels], dtype=F.FEATURE_DTYPE)
    assert_same_bits(got, ref)
    assert whole["hits"].min() >= 0 and whole["hits"].max() <= spp and np.array_equal(whole["hits"], np.floor(whole["hits"]))
    # Every sample's normal has unit length to rounding (or is 0 on a miss), so the sum's length is at most hits to rounding.
    # The rounding: a sphere's normal is (o + t d - c) / r, and Sphere::hit accepts a root whenever the COMPUTED discriminant
    # hb^2 - a c is >= 0; its two terms are of size (|oc| |d|)^2 with relative error eps each, so a ray may be accepted that
    # really passes the sphere at distance r + h, h ~ eps |oc|^2 / r, and the normal is then longer than 1 by h / r ~
    # eps (|oc| / r)^2. In this scene |oc| < 2000 (camera to the far end of the ground boxes) and the smallest radius is 10:
    # eps (200)^2 = 9e-12; with a factor 64 for the dozen roundings on the way (t, p, the division, the transforms, the sum)
    # the bound is 6e-10: 1e-9 relative.
    length, hits = np.linalg.norm(whole["normal"], axis=-1), whole["hits"]
    print("largest |sum of normals| - hits: %.3e (relative %.3e)" % ((length - hits).max(), ((length - hits) / np.maximum(hits, 1)).max()))
    assert np.all(length <= hits * (1 + 1e-9))
    assert np.all(whole["depth"][whole["hits"] == 0] == 0) and np.all(whole["depth"][whole["hits"] > 0] > 0)


# ---- 10. the deep-stack instances -------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,param,assets", [("wwscene", 3, True), ("random_scene", 158, False)])
def test_big_scenes_on_the_deep_stack_instances(rt, O, scene, param, assets):
    """The C5 mesh (0.84 M triangles under three movers, 30-entry stacks) and the 1e5-sphere scene (a node table far beyond
    LDS): a whole small frame on the device, a pixel sample against the oracle."""
    s = rt.HostScene(scene, seed=2022, param=param, assets_dir=ASSETS if assets else None)
    d = s.desc
    assert d.n_nodes > 100_000
    W, H, spp = 160, 120, 2
    cam, bg = s.default_view(W / H)
    p = rt.make_params(W, H, spp, 50, bg, seed=param)
    rows = rt.shuffled_rows(H, param)
    dev = rt.DeviceScene(d)
    assert dev.info()["stack_need"] > 16                                    # not the LDS-prefix instance
    got, st = dev.features(cam, p, rows, want_stats=True)
    pixels = sampled_pixels(H, W, 1500, seed=param)
    ref, _, _ = oracle_features(O, d, cam, p, rows, pixels=pixels)
    assert_same_bits(np.array([got[i, px] for i, px in pixels], dtype=F.FEATURE_DTYPE), ref)
    assert st.paths == st.rays == W * H * spp and st.node_visits > st.rays
    assert_same_bits(dev.features(cam, p, rows), got, "plain instance")
    assert got["hits"].sum() > 1000
