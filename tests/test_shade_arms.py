"""Every arm of the shade pass (wf_shade, pt_wavefront_shade.hip; the megakernel's twin, pt_kernel.hip) on a scene built to enter it
(tests/shade_scenes.py), compared with the CPU oracle bit for bit — pixel sums with their NaN patterns, counters, u8 pixels. That
the oracle's paths enter the arm a case is named for is asserted without a GPU, from its shade census
(tests/test_shade_scenes.py); equal counters then say the device's paths took the same turns.

Per case: rt_render with and without counters on one DeviceScene, and the megakernel engine. Over a spread of the cases — every
material kind, the 9-entry light list, the tape cases — the ways the pass is instantiated and driven: spp_chunk 0, 1 and 3 at 7
samples (an uneven last chunk), the partial-sum ring forced to 1 and to 2 planes, two frames in one call, and rt_radiance for
the pinhole rays of the same view with and without the ring: wf_shade<STATS, RING, RAYS> in all its eight instances."""
import numpy as np
import pytest

import shade_scenes as S
import trace_scenes as T
from raytracer_2022_amd import _ffi as F
from raytracer_2022_amd import film
from compare import same_bits
from gpu_first import torch_first  # noqa: F401
from radiance_ref import oracle_radiance, radiance_counters

pytestmark = pytest.mark.gpu

# Every comparison here is same_bits without payloads — bit for bit, a NaN wherever the oracle has one. A NaN's payload must not
# be compared: 0 / 0 and inf * 0 need not agree on a sign.

IDS = [c.name for c in S.CASES]
# every material kind (and the textures that need u, v on each), the light list behind the LDS table, every tape case
SPREAD = ["lambertian-checker-image-noise", "light-image", "isotropic-nested8", "metal-fuzz-1", "glass-outside", "lights-9",
          "tape-black-background", "tape-sky-background", "tape-depth-2", "tape-zero-light", "tape-inf-light"]
SPP7 = 7


def with_params(p, **kw):
    q = F.rt_params.from_buffer_copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


@pytest.fixture(scope="module")
def scenes():
    """case name → its scene (desc, cam, params, rows [, extra]) and one DeviceScene of it, built once."""
    import raytracer_2022_amd as rt
    cache = {}

    def get(name):
        if name not in cache:
            scene = S.BY_NAME[name].build()
            cache[name] = (scene, rt.DeviceScene(scene[0]))
        return cache[name]
    yield get
    for _, dev in cache.values():
        dev.close()


@pytest.fixture(scope="module")
def oracle_render(O):
    """The oracle's render of (case, params, rows), made once and never written to → (pixel sums, counters)."""
    cache = {}

    def get(name, scene, p, rows):
        key = (name, p.spp, p.spp_chunk, p.n_frames, p.max_depth, bytes(np.asarray(rows, dtype=np.uint32)))
        if key not in cache:
            ref, st = O.render_cpu(scene[0], scene[1], p, rows, n_threads=8, want_stats=True)
            ref.setflags(write=False)
            cache[key] = (ref, st.as_dict())
        return cache[key]
    return get


def check_render(rt, O, dev, ref, counters_ref, cam, p, rows, what):
    out, st = dev.render(cam, p, rows, want_stats=True)
    assert st.as_dict() == counters_ref, (what, "the device's paths took other turns than the oracle's")
    assert same_bits(out, ref), (what, "counting instance")
    assert np.array_equal(rt.write_color(out, max(p.spp, 1)), O.write_color(ref, max(p.spp, 1))), what
    assert same_bits(dev.render(cam, p, rows), ref), (what, "timed instance")
    return st


@pytest.mark.parametrize("name", IDS)
def test_case_matches_the_oracle(rt, O, scenes, oracle_render, name):
    scene, dev = scenes(name)
    d, cam, p, rows = scene[:4]
    ref, counters_ref = oracle_render(name, scene, p, rows)
    dev.set_engine("wavefront")
    check_render(rt, O, dev, ref, counters_ref, cam, p, rows, name)


@pytest.mark.parametrize("name", IDS)
def test_megakernel_matches_the_oracle(rt, O, scenes, oracle_render, name):
    scene, dev = scenes(name)
    d, cam, p, rows = scene[:4]
    assert not T.mega_refuses(d)                          # (every medium here has a sphere for its boundary)
    ref, counters_ref = oracle_render(name, scene, p, rows)
    dev.set_engine("mega")
    try:
        check_render(rt, O, dev, ref, counters_ref, cam, p, rows, name)
    finally:
        dev.set_engine("wavefront")


@pytest.mark.parametrize("name", SPREAD)
def test_chunks_ring_and_frames(rt, O, scenes, oracle_render, name):
    """7 samples in chunks of 7, 1 and 3 (the last chunk holds one sample); one-sample items through a ring of 1 and of 2 planes;
    two frames in one call. With counters (wf_shade<true, RING>) and without (wf_shade<false, RING>)."""
    scene, dev = scenes(name)
    d, cam, p, rows = scene[:4]
    dev.set_engine("wavefront")
    pixels = S.W * S.H
    for chunk in (0, 1, 3):
        q = with_params(p, spp=SPP7, spp_chunk=chunk)
        ref, counters_ref = oracle_render(name, scene, q, rows)
        dev.set_partial_ring(-1)
        st = check_render(rt, O, dev, ref, counters_ref, cam, q, rows, (name, "chunk", chunk))
        assert st.spp_chunk == (chunk or SPP7) and st.partial_bytes == pixels * {0: 0, 1: 7, 3: 3}[chunk] * 24      # (one chunk sums in place)
        if chunk == 1:
            for planes in (1, 2):
                dev.set_partial_ring(planes)
                st = check_render(rt, O, dev, ref, counters_ref, cam, q, rows, (name, "ring", planes))
                assert st.partial_bytes == pixels * planes * 24, "the ring was not used"
    dev.set_partial_ring(0)
    q = with_params(p, n_frames=2, spp_chunk=1)
    strip = film.strip_rows(S.H, 2, 5)
    assert set(strip // S.H) == {0, 1}
    ref, counters_ref = oracle_render(name, scene, q, strip)
    check_render(rt, O, dev, ref, counters_ref, cam, q, strip, (name, "two frames"))
    one = dev.render(cam, with_params(p, spp_chunk=1), strip[strip < S.H])
    assert same_bits(one, ref[strip < S.H]), "frame 0 of the strip is the frame rendered alone"


def radiance_same(a, ref):
    return same_bits(np.asarray(a), np.asarray(ref))


@pytest.mark.parametrize("name", SPREAD + ["lambertian-image-rect"])
def test_radiance_of_the_view(rt, O, scenes, name):
    """rt_radiance (wf_shade<STATS, RING, true>) for the pinhole rays of the case's view — and, for the image on a rect, rays
    that hit it exactly on its a1 / b1 edges (u == 1: the index clamp of the image lookup). 3 samples: all planes, then a ring."""
    scene, dev = scenes(name)
    d, cam, p, rows = scene[:4]
    dev.set_engine("wavefront")
    g = np.random.default_rng(len(name))
    origins, dirs = S.pinhole_rays(cam, S.W, S.H)
    rays = rt.radiance_rays(origins, dirs, time=g.uniform(cam.time0, cam.time1, len(origins)),
                            rng_state=g.integers(0, 2**63, len(origins), dtype=np.uint64))
    if len(scene) > 4 and "origins" in scene[4]:
        edge = scene[4]
        rays = np.concatenate([rt.radiance_rays(np.array(edge["origins"]), edge["direction"], rng_state=g.integers(0, 2**63, len(edge["origins"]), dtype=np.uint64)), rays])
    bg, spp, depth = tuple(p.background[:]), 3, p.max_depth
    ref, st_ref = oracle_radiance(O, d, rays, spp, bg, p.t_min, depth)
    n = len(rays)
    for planes, want_bytes in ((-1, n * spp * 24), (2, n * 2 * 24), (1, n * 24)):
        dev.set_partial_ring(planes)
        try:
            got, st = dev.radiance(rays, spp=spp, background=bg, t_min=p.t_min, max_depth=depth, want_stats=True)
            plain = dev.radiance(rays, spp=spp, background=bg, t_min=p.t_min, max_depth=depth)
        finally:
            dev.set_partial_ring(0)
        assert radiance_same(got, ref), (name, planes, "counting instance")
        assert radiance_counters(st) == radiance_counters(st_ref) and st.paths == n * spp, (name, planes)
        assert st.partial_bytes == want_bytes, (name, planes, "the ring was not used" if planes > 0 else "")
        assert radiance_same(plain, ref), (name, planes, "timed instance")
