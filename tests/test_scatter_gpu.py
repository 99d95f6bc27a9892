"""rt_scatter / rt_scatter_device on the GPU against tests/scatter_ref.py, record by record and field by field (doubles by their
bits, NaN where the reference has NaN; words exactly): first hits and made-up records, batch sizes, hostile entries, `prev` and
the two permitted aliasings, the identity radiance_by_steps == rt_radiance == rto_radiance, and the device form."""
import json
import os

import numpy as np
import pytest

from raytracer_2022_amd import _ffi as F

import scatter_ref as S
from compare import assert_same_bits
from gpu_first import torch_first  # noqa: F401
from query_ref import camera_rays, unit_vectors
from query_scenes import every_kind_lit_scene, every_material_scene
from radiance_ref import radiance_camera_rays
from specular_ref import state_after

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INDEX = json.load(open(os.path.join(HERE, "golden", "golden_index.json")))
BUILDERS = sorted({c["scene"] for c in INDEX.values()})
LIVE = (F.RT_SCATTER_SPECULAR, F.RT_SCATTER_DIFFUSE)


def assert_records(got, ref, what=""):
    """Two arrays of one record dtype: every double by its bits (NaNs in the same places), every word exactly."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    for name in got.dtype.names:
        if got.dtype[name].base == np.float64:
            assert_same_bits(got[name], ref[name], (what, name))
        else:
            bad = np.flatnonzero(got[name] != ref[name])
            assert len(bad) == 0, (what, name, bad[:5].tolist(), got[name][bad[:5]].tolist(), ref[name][bad[:5]].tolist())


def reference(O, desc, rays, hits, background=(0.0, 0.0, 0.0), t_min=0.001, prev=None):
    """scatter_ref.step entry by entry → (records, next rays, light_pdf_tests)."""
    recs, nxt = np.zeros(len(rays), dtype=F.SCATTER_REC_DTYPE), np.zeros(len(rays), dtype=F.QUERY_RAY_DTYPE)
    per_record, tests = S.light_tests_per_record(desc), 0
    for i, (r, h) in enumerate(zip(rays, hits)):
        if prev is not None and int(prev[i]["status"]) not in LIVE:
            recs[i]["status"], nxt[i]["rng_state"] = F.RT_SCATTER_ENDED, r["rng_state"]
            continue
        ray = list(r["origin"]) + list(r["direction"]) + [float(r["time"])]
        recs[i], nxt[i], _ = S.step(O, desc, ray, S.hit_record(O, h), state_after(int(r["rng_state"]), int(h["rng_draws"])), background, t_min)
        if int(recs[i]["status"]) == F.RT_SCATTER_DIFFUSE and desc.n_lights:
            tests += per_record
    return recs, nxt, tests


def check_step(O, dev, desc, rays, hits, background=(0.0, 0.0, 0.0), t_min=0.001, prev=None, what=""):
    recs, nxt, st = dev.scatter(rays, hits, background, t_min, prev, want_stats=True)
    ref_recs, ref_nxt, tests = reference(O, desc, rays, hits, background, t_min, prev)
    assert_records(recs, ref_recs, (what, "records"))
    assert_records(nxt, ref_nxt, (what, "next rays"))
    assert st.rng_draws == int(ref_recs["rng_draws"].sum()) and st.light_pdf_tests == tests, what
    assert st.ms > 0 and st.rays == 0 and st.paths == 0 and st.node_visits == 0 and not any(st.prim_tests) and st.passes == 0, what
    plain = dev.scatter(rays, hits, background, t_min, prev)                       # the plain kernel instance
    assert_records(plain[0], recs, (what, "plain"))
    assert_records(plain[1], nxt, (what, "plain"))
    return recs, nxt


def two_steps(rt, O, dev, desc, cam, n, seed, background, what):
    """First hits of n camera rays, and the step behind them chained with prev."""
    g = np.random.default_rng(seed)
    q = camera_rays(rt, cam, n, g)
    q["rng_state"] = g.integers(0, 2**63, n, dtype=np.uint64)
    q["t_max"] = np.finfo(np.float64).max
    hits = dev.intersect(q)
    recs, nxt = check_step(O, dev, desc, q, hits, background, what=(what, "first hits"))
    hits2 = dev.intersect(nxt)
    recs2, _ = check_step(O, dev, desc, nxt, hits2, background, prev=recs, what=(what, "second step"))
    live = np.isin(recs["status"], LIVE)
    assert np.all(recs2["status"][~live] == F.RT_SCATTER_ENDED) and np.all(recs2["status"][live] != F.RT_SCATTER_ENDED)
    return recs, recs2


@pytest.mark.parametrize("name", BUILDERS)
def test_first_hits_of_every_scene_builder(rt, O, name):
    s = rt.HostScene(name, seed=2022)
    cam, bg = s.default_view(1.5)
    recs, recs2 = two_steps(rt, O, rt.DeviceScene(s.desc), s.desc, cam, 384, len(name), tuple(bg), name)
    assert len(set(recs["status"].tolist()) | set(recs2["status"].tolist())) >= 3


@pytest.mark.parametrize("lights", [True, False])
def test_first_hits_of_every_kind(rt, O, lights):
    b, d, cam = every_kind_lit_scene(rt, lights=lights)
    recs, recs2 = two_steps(rt, O, rt.DeviceScene(d), d, cam, 512, 3 + lights, (0.3, 0.2, 0.7), "every kind, lights %s" % lights)
    assert {F.RT_SCATTER_MISS, F.RT_SCATTER_SPECULAR, F.RT_SCATTER_DIFFUSE} <= set(recs["status"].tolist())


def test_first_hits_of_every_material(rt, O):
    """Every material kind x every texture kind, no light list: records rt_intersect itself made, and the step behind them."""
    b, d, named = every_material_scene(rt)
    assert d.n_lights == 0
    cam = rt.camera_new((0, 1.8, 9.0), (0, 1.5, 0), (0, 1, 0), 50.0, 1.5, 0.0, 9.0, 0.0, 1.0)
    recs, recs2 = two_steps(rt, O, rt.DeviceScene(d), d, cam, 512, 7, (0.6, 0.7, 0.9), "every material")
    assert {F.RT_SCATTER_MISS, F.RT_SCATTER_EMITTED, F.RT_SCATTER_SPECULAR, F.RT_SCATTER_DIFFUSE} <= set(recs["status"].tolist())


def made_up(desc, n, g, mats=None):
    """n entries no traversal made: random rays and records on every material of the scene, both faces."""
    rays = np.zeros(n, dtype=F.QUERY_RAY_DTYPE)
    rays["origin"], rays["direction"], rays["time"] = g.normal(size=(n, 3)) * 3, g.normal(size=(n, 3)), g.random(n)
    rays["t_min"], rays["t_max"], rays["rng_state"] = 0.001, np.inf, g.integers(0, 2**64, n, dtype=np.uint64)
    hits = np.zeros(n, dtype=F.HIT_DTYPE)
    hits["t"], hits["u"], hits["v"] = g.exponential(3.0, n), g.random(n), g.random(n)
    hits["p"], hits["normal"] = g.normal(size=(n, 3)) * 2 + (0, 2, 0), unit_vectors(g, n)
    hits["hit"], hits["front_face"] = 1, g.integers(0, 2, n)
    hits["mat"] = np.arange(n) % desc.n_materials if mats is None else g.choice(mats, n)
    hits["prim"], hits["rng_draws"] = g.integers(0, 2**32, n), g.integers(0, 40, n)
    return rays, hits


@pytest.fixture(scope="module")
def lit(rt):
    b, d, cam = every_kind_lit_scene(rt)
    return b, d, cam, rt.DeviceScene(d)


@pytest.fixture(scope="module")
def made_up_1000(rt, O, lit):
    """1 000 made-up entries on the lit scene with the device's records and the reference's, computed once."""
    b, d, cam, dev = lit
    rays, hits = made_up(d, 1000, np.random.default_rng(21))
    recs, nxt = check_step(O, dev, d, rays, hits, (0.2, 0.4, 0.6), what="made up, lit")
    return rays, hits, recs, nxt


def test_made_up_records(rt, O, made_up_1000):
    rays, hits, recs, nxt = made_up_1000
    assert set(recs["status"].tolist()) == {F.RT_SCATTER_EMITTED, F.RT_SCATTER_SPECULAR, F.RT_SCATTER_DIFFUSE}
    b, d, named = every_material_scene(rt)                                      # every material x every texture, no light list
    dev = rt.DeviceScene(d)
    r2, h2 = made_up(d, 600, np.random.default_rng(22))
    check_step(O, dev, d, r2, h2, (0.6, 0.7, 0.9), what="made up, every material")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_sizes(rt, lit, made_up_1000, n):
    """An entry's output depends neither on its place nor on the batch."""
    rays, hits, recs, nxt = made_up_1000
    dev = lit[3]
    pick = np.random.default_rng(n).permutation(1000)[:n]
    got = dev.scatter(rays[pick], hits[pick], (0.2, 0.4, 0.6))
    assert_records(got[0], recs[pick], n)
    assert_records(got[1], nxt[pick], n)


def test_hostile_entries(rt, O, lit):
    b, d, cam, dev = lit
    g = np.random.default_rng(31)
    lamb = [i for i in range(d.n_materials) if d.materials[i].kind == F.RT_MAT_LAMBERTIAN][:2]
    others = [next(i for i in range(d.n_materials) if d.materials[i].kind == k)
              for k in (F.RT_MAT_METAL, F.RT_MAT_DIELECTRIC, F.RT_MAT_ISOTROPIC, F.RT_MAT_DIFFUSE_LIGHT)]
    mats = lamb + others
    n = 8 * len(mats) * 4
    rays, hits = made_up(d, n, g, mats)
    hits["mat"] = np.repeat(mats, n // len(mats))
    k = np.arange(n) % 8
    hits["normal"][k == 0] = (np.nan, 0.0, 1.0)
    hits["normal"][k == 1] = (0.0, 0.0, 0.0)
    hits["normal"][k == 2] = (np.inf, 1.0, 0.0)
    rays["direction"][k == 3] = (0.0, 0.0, 0.0)
    hits["rng_draws"][k == 4] = 0xFFFFFFFF
    hits["hit"][k == 5], hits["front_face"][k == 5] = 2, 7                         # any non-zero word is true
    hits["p"][k == 6] = (np.nan, np.inf, -np.inf)
    rays["direction"][k == 7] = (np.nan, 1.0, -np.inf)
    recs, nxt = check_step(O, dev, d, rays, hits, (0.1, 0.2, 0.3), what="hostile")
    assert np.all(recs["status"][(k == 5) & (hits["mat"] != others[3])] != F.RT_SCATTER_MISS)
    # hit == 0 with garbage elsewhere: a miss, whatever the record says — a material no pool holds included
    junk = hits.copy()
    junk["hit"] = 0
    junk["mat"][::2] = 0xFFFFFFFF
    junk.view(np.uint8).reshape(n, 96)[:, :72] = g.integers(0, 256, (n, 72), dtype=np.uint8)
    recs, nxt = check_step(O, dev, d, rays, junk, (0.1, 0.2, 0.3), what="misses")
    assert np.all(recs["status"] == F.RT_SCATTER_MISS) and np.all(recs["radiance"] == (0.1, 0.2, 0.3))
    assert not nxt.view(np.uint8).reshape(n, 80)[:, :72].any()
    assert [int(x) for x in nxt["rng_state"]] == [state_after(int(s), int(w)) for s, w in zip(rays["rng_state"], junk["rng_draws"])]
    # a material index at or beyond the pool: INVALID with zeros
    bad = hits.copy()
    bad["mat"] = np.where(np.arange(n) % 2, d.n_materials, 0xFFFFFFFF)
    recs, nxt = check_step(O, dev, d, rays, bad, (0.1, 0.2, 0.3), what="invalid")
    assert np.all(recs["status"] == F.RT_SCATTER_INVALID)
    assert not recs.view(np.uint8).reshape(n, 64)[:, :56].any() and np.all(recs["rng_draws"] == 0)
    assert not nxt.view(np.uint8).reshape(n, 80)[:, :72].any()


def test_prev_every_status_and_the_aliasings(rt, O, lit, made_up_1000):
    import torch
    b, d, cam, dev = lit
    rays, hits, recs, nxt = (a[:300] for a in made_up_1000)
    g = np.random.default_rng(41)
    prev = np.zeros(300, dtype=F.SCATTER_REC_DTYPE)
    prev["status"] = np.arange(300) % 8                                            # the six statuses and two words that are none
    prev["status"][prev["status"] == 7] = 0xFFFFFFFF
    prev["weight"], prev["pdf"], prev["radiance"], prev["rng_draws"] = g.random((300, 3)), g.random(300), g.random((300, 3)), 5
    got, got_next = check_step(O, dev, d, rays, hits, (0.2, 0.4, 0.6), prev=prev, what="prev")
    live = np.isin(prev["status"], LIVE)
    assert np.all(got["status"][~live] == F.RT_SCATTER_ENDED) and live.sum() == 2 * (300 // 8) + 2
    assert_records(got[live], recs[live], "live under prev")                       # a live entry is what it is without prev
    assert not got[~live].view(np.uint8).reshape(-1, 64)[:, :56].any() and np.all(got["rng_draws"][~live] == 0)
    assert np.array_equal(got_next["rng_state"][~live], rays["rng_state"][~live])
    assert not got_next[~live].view(np.uint8).reshape(-1, 80)[:, :72].any()
    # device form: the records written over prev, the next rays over the rays
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.from_numpy(hits.view(np.uint8).copy()).cuda()
    d_prev = torch.from_numpy(prev.view(np.uint8).copy()).cuda()
    p = rt.scatter_params((0.2, 0.4, 0.6))
    st = F.rt_stats()
    dev.scatter_device(d_rays.data_ptr(), d_hits.data_ptr(), 300, d_prev.data_ptr(), d_rays.data_ptr(), p, d_prev_ptr=d_prev.data_ptr(), stats=st)
    assert_records(d_prev.cpu().numpy().view(F.SCATTER_REC_DTYPE), got, "records over prev")
    assert_records(d_rays.cpu().numpy().view(F.QUERY_RAY_DTYPE), got_next, "next rays over rays")
    assert st.ms > 0 and st.rng_draws == 0                                         # (no RT_FLAG_COUNTERS: nothing is counted)


IDENTITY = ["cornell_box", "cornell_smoke", "final_scene", "random_scene", "simple_light", "no_lights"]


@pytest.mark.parametrize("name", IDENTITY)
def test_steps_unwound_are_rt_radiance(rt, O, name):
    """radiance_by_steps == dev.radiance == rto_radiance bit for bit, and the loop's counts are rt_radiance's."""
    if name == "no_lights":
        b, d, cam = every_kind_lit_scene(rt, lights=False)
        bg = (0.3, 0.2, 0.7)
    else:
        s = rt.HostScene(name, seed=2022)
        d = s.desc
        cam, bg = s.default_view(1.5)
    dev = rt.DeviceScene(d)
    rays = radiance_camera_rays(rt, cam, 256, np.random.default_rng(len(name)))
    seen = []
    for spp in (1, 3):
        for depth in (1, 2, 5, 50):
            calls = []
            got, counts = rt.radiance_by_steps(dev, rays, spp=spp, max_depth=depth, background=tuple(bg), want_stats=True,
                                               on_step=lambda k, q, h, r: calls.append((k, len(q), len(h), len(r))))
            want, st = dev.radiance(rays, spp=spp, background=tuple(bg), max_depth=depth, want_stats=True)
            assert_same_bits(got, want, (name, spp, depth, "rt_radiance"))
            assert_same_bits(got, O.radiance(d, rays, spp=spp, background=tuple(bg), depth=depth, n_threads=8), (name, spp, depth, "rto_radiance"))
            assert counts == {"rng_draws": st.rng_draws, "light_pdf_tests": st.light_pdf_tests, "rays": st.rays}, (name, spp, depth)
            assert len(calls) <= spp * depth and all(c[1:] == (256, 256, 256) for c in calls) and max(c[0] for c in calls) < depth
            seen.append(len(calls))
    assert np.any(got != 0) and seen[0] == 1 and seen[1] == 2 and seen[3] >= seen[2] >= 3      # (the loop stops when nothing is live)


def test_device_form_on_torch_buffers(rt, O, lit, made_up_1000):
    import torch
    b, d, cam, dev = lit
    rays, hits, recs, nxt = made_up_1000
    n = len(rays)
    stream = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.from_numpy(hits.view(np.uint8).copy()).cuda()
    d_recs = torch.full((n * 64,), 0xAB, dtype=torch.uint8, device="cuda")
    d_next = torch.full((n * 80,), 0xAB, dtype=torch.uint8, device="cuda")
    p = rt.scatter_params((0.2, 0.4, 0.6))
    torch.cuda.synchronize()
    dev.scatter_device(d_rays.data_ptr(), d_hits.data_ptr(), n, d_recs.data_ptr(), d_next.data_ptr(), p, stream_ptr=stream.cuda_stream)   # stats=None: no sync
    with torch.cuda.stream(stream):
        copy = d_recs.clone()                                                      # a dependent copy on the caller's stream
    stream.synchronize()
    assert_records(copy.cpu().numpy().view(F.SCATTER_REC_DTYPE), recs, "torch buffers")
    assert_records(d_next.cpu().numpy().view(F.QUERY_RAY_DTYPE), nxt, "torch buffers")
    # n == 0 launches nothing
    d_recs.fill_(0xAB)
    dev.scatter_device(d_rays.data_ptr(), d_hits.data_ptr(), 0, d_recs.data_ptr(), d_next.data_ptr(), p, stream_ptr=stream.cuda_stream)
    stream.synchronize()
    assert bool((d_recs == 0xAB).all())
    # counters on the device form
    st = F.rt_stats()
    pc = rt.scatter_params((0.2, 0.4, 0.6), flags=F.RT_FLAG_COUNTERS)
    dev.scatter_device(d_rays.data_ptr(), d_hits.data_ptr(), n, d_recs.data_ptr(), d_next.data_ptr(), pc, stream_ptr=stream.cuda_stream, stats=st)
    assert st.rng_draws == int(recs["rng_draws"].sum()) and st.ms > 0
    assert st.light_pdf_tests == S.light_tests_per_record(d) * int((recs["status"] == F.RT_SCATTER_DIFFUSE).sum())
    # misaligned and null buffers are refused with the outputs untouched
    d_recs.fill_(0xAB)
    d_next.fill_(0xAB)
    good = dict(d_rays_ptr=d_rays.data_ptr(), d_hits_ptr=d_hits.data_ptr(), n=n - 1, d_recs_ptr=d_recs.data_ptr(), d_next_rays_ptr=d_next.data_ptr(), params=p)
    for name in ("d_rays_ptr", "d_hits_ptr", "d_recs_ptr", "d_next_rays_ptr"):
        for value, msg in ((good[name] + 8, "16-byte aligned"), (0, "null ray, hit, record or next-ray buffer")):
            with pytest.raises(rt.RtError, match=msg) as e:
                dev.scatter_device(**{**good, name: value})
            assert e.value.code == F.RT_ERR_INVALID and "rt_scatter_device: " in str(e.value)
    with pytest.raises(rt.RtError, match="16-byte aligned"):
        dev.scatter_device(**good, d_prev_ptr=d_recs.data_ptr() + 4)
    torch.cuda.synchronize()
    assert bool((d_recs == 0xAB).all()) and bool((d_next == 0xAB).all())


def test_beside_an_asynchronous_render(rt, O):
    import torch
    s = rt.HostScene("final_scene", seed=2022)
    W, H, spp = 64, 48, 4
    cam, bg = s.default_view(W / H)
    rows = rt.shuffled_rows(H, 3)
    p = rt.make_params(W, H, spp, 50, bg, seed=2022, spp_chunk=1)
    dev = rt.DeviceScene(s.desc)
    ref_render = dev.render(cam, p, rows)
    g = np.random.default_rng(9)
    q = camera_rays(rt, cam, 30_000, g)
    q["rng_state"] = g.integers(0, 2**63, len(q), dtype=np.uint64)
    hits = dev.intersect(q)
    serial = dev.scatter(q, hits, tuple(bg))
    a_stream, b_stream = torch.cuda.Stream(), torch.cuda.Stream()
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    out = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda")
    d_rays, d_hits = torch.from_numpy(q.view(np.uint8)).cuda(), torch.from_numpy(hits.view(np.uint8)).cuda()
    d_recs = [torch.zeros(len(q) * 64, dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_next = [torch.zeros(len(q) * 80, dtype=torch.uint8, device="cuda") for _ in range(3)]
    sp = rt.scatter_params(tuple(bg))
    torch.cuda.synchronize()
    dev.render_device(cam, p, d_rows.data_ptr(), H, out.data_ptr(), a_stream.cuda_stream, None, asynchronous=True)
    for r_, n_ in zip(d_recs, d_next):
        dev.scatter_device(d_rays.data_ptr(), d_hits.data_ptr(), len(q), r_.data_ptr(), n_.data_ptr(), sp, stream_ptr=b_stream.cuda_stream)
    b_stream.synchronize()
    dev.wait(a_stream.cuda_stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), ref_render.view(np.uint64))
    for r_, n_ in zip(d_recs, d_next):
        assert_records(r_.cpu().numpy().view(F.SCATTER_REC_DTYPE), serial[0], "beside a render")
        assert_records(n_.cpu().numpy().view(F.QUERY_RAY_DTYPE), serial[1], "beside a render")
