"""Every entry point of the device on the generated scene graphs of tests/scene_gen.py, one case per committed scene: the
oracle bit for bit where the project holds the device to it, and tests/brute_hits.py — which never reads a node box — for the
closest hit itself. tests/test_scene_gen.py holds the oracle to the same references on the same scenes, CPU only.

Per scene, in this order: the stack need and the wf_trace instance rt_scene_create chose, asserted BEFORE any launch (a wrong
need on a shape nobody built is a stack overrun in a kernel, not a wrong pixel); rt_intersect (plain and counter instance);
RT_FLAG_ANY_HIT where the scene has no medium; rt_ray_order + rt_intersect_ordered; rt_radiance; rt_render under both engines
and chunkings; rt_features under the four flag combinations; rt_scatter; and the closest hits again on a tree rebuilt by the
device builder. SCENE_GEN_LOG=<path> appends the measured shares per scene to that file (profiles/scene_gen.log is such a run)."""
import os

import numpy as np
import pytest

import brute_hits as B
import brute_scenes as S
import features_ref as FR
import scatter_ref as SC
import scene_gen as G
import specular_ref as SP
import surface_ref as SU
import trace_scenes as T
from compare import assert_same_bits, same_bits
from gpu_first import torch_first  # noqa: F401
from query_ref import assert_prims_consistent, assert_records_equal, oracle_hits, query_counters
from radiance_ref import oracle_radiance, radiance_camera_rays, radiance_counters, render_counters
from raytracer_2022_amd import _ffi as F

pytestmark = pytest.mark.gpu

BACKGROUND = (0.15, 0.25, 0.4)
W, H, SPP, DEPTH = 16, 12, 2, 8
CLASS2_SHARE = 0.5                                           # tests/test_scene_gen.py


def assert_records(got, ref, what):
    """Two arrays of one record dtype: every double by its bits, every word exactly."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    for name in got.dtype.names:
        if got.dtype[name].base == np.float64:
            assert_same_bits(got[name], ref[name], (what, name))
        else:
            assert np.array_equal(got[name], ref[name]), (what, name)


def brute_check(dev, profile, sc, fams, name, who):
    """rt_intersect of every family against the brute answer → ({key: records of the plain instance}, worst |dt| / tolerance,
    worst ambiguous share)."""
    hits, worst, share, compared = {}, 0.0, 0.0, 0
    for key, (rays, ans) in fams.items():
        c1, c2, c3, amb = B.classify(sc, ans)
        assert amb.sum() <= S.AMBIGUOUS_SHARE * len(rays), (name, key)                          # (before any result)
        assert not c1.any() and c2.sum() <= (CLASS2_SHARE * len(rays) if G.PROFILES[profile]["zoom_under_node"] else 0)
        q = np.ascontiguousarray(rays, dtype=F.QUERY_RAY_DTYPE)
        got = dev.intersect(q)
        ta, _ = B.compare(sc, rays, got["hit"], got["t"], got["rng_draws"], got["prim"], ans=ans)
        print(ta.line(name, "%s/%s" % key, who))
        assert not ta.failures, (name, key, ta.failures[:5])
        assert ta.worst <= 1.0
        hits[key], worst, share, compared = got, max(worst, ta.worst), max(share, amb.sum() / len(rays)), compared + ta.compared
    assert compared >= 0.5 * 2 * S.N_RAYS
    return hits, worst, share


@pytest.mark.parametrize("case", G.CASES, ids=[G.case_id(c) for c in G.CASES])
def test_every_entry_point_on_a_generated_scene(rt, O, case):
    profile, seed = case
    name = G.case_id(case)
    _, d, cams, facts, sc, fams = G.solved(profile, seed)
    dev = rt.DeviceScene(d)
    # 1. what check_scene derived from the graph, before any launch on the scene
    need = T.stack_need(d)
    assert dev.info()["stack_need"] == need
    want = T.expected_variant(d, need)
    assert dev.trace_variant() == {k: v for k, v in want.items() if k != "table"}, want
    # 2. rt_intersect: the oracle's records and counters, then the brute answer
    hits, worst, share = brute_check(dev, profile, sc, fams, name, "hip")
    for key, (rays, ans) in fams.items():
        q = np.ascontiguousarray(rays, dtype=F.QUERY_RAY_DTYPE)
        counted, st = dev.intersect(q, want_stats=True)
        assert np.array_equal(hits[key].view(np.uint8), counted.view(np.uint8)) and st.rays == len(q)
        ref, st_ref = oracle_hits(O, d, q)
        assert_records_equal(counted, ref, (name, key))
        assert_prims_consistent(d, counted)
        assert query_counters(st) == query_counters(st_ref, ref), (name, key)
        # 3. any hit: the same verdict, and some candidate's own record
        if not sc.media:
            anyh = dev.intersect(q, any_hit=True)
            assert np.array_equal(anyh["hit"], counted["hit"]), (name, key)
            c1, c2, c3, amb = B.classify(sc, ans)
            h = np.flatnonzero((anyh["hit"] == 1) & ~(c1 | c2 | c3 | amb))
            ok = B.matches_a_candidate(sc, rays["origin"][h], rays["direction"][h], rays["time"][h], rays["t_min"][h], rays["t_max"][h],
                                       anyh["t"][h], anyh["prim"][h])
            assert ok.all(), (name, key, h[~ok][:5].tolist())
        # 4. a coherence order of the device's own, and the query through it
        order = rt.ray_order(q)
        assert np.array_equal(np.sort(order), np.arange(len(q)))
        assert np.array_equal(dev.intersect(q, order=order).view(np.uint8), hits[key].view(np.uint8)), (name, key)
    # 5. rt_radiance
    g = np.random.default_rng(seed)
    rr = np.concatenate([radiance_camera_rays(rt, cam, 128, g) for cam in cams])
    out, st = dev.radiance(rr, spp=SPP, background=BACKGROUND, max_depth=DEPTH, want_stats=True)
    ref, st_ref = oracle_radiance(O, d, rr, SPP, BACKGROUND, depth=DEPTH)
    assert same_bits(out, ref), name
    assert radiance_counters(st) == radiance_counters(st_ref), name
    # 6. rt_render
    rows = rt.shuffled_rows(H, seed)
    p0 = rt.make_params(W, H, SPP, DEPTH, BACKGROUND, seed=seed)
    ref, st_ref = O.render_cpu(d, cams[0], p0, rows, n_threads=4, want_stats=True)
    for engine in ("wavefront", "mega"):
        if engine == "mega" and T.mega_refuses(d):
            with pytest.raises(F.RtError) as e:
                dev.set_engine("mega")
            assert e.value.code == F.RT_ERR_UNSUPPORTED
            continue
        dev.set_engine(engine)
        for chunk in (0, 1):
            p = rt.make_params(W, H, SPP, DEPTH, BACKGROUND, seed=seed, spp_chunk=chunk)
            out, st = dev.render(cams[0], p, rows, want_stats=True)
            assert same_bits(out, ref), (name, engine, chunk)
            assert render_counters(st) == render_counters(st_ref), (name, engine, chunk)
    dev.set_engine("wavefront")
    # 7. rt_features: plain, RT_FLAG_SURFACES, RT_FLAG_SPECULAR, both
    FR.check_view(rt, O, d, cams[0], p0, rows, dev)
    ref, st_copy, seen, words = SU.oracle_surface_features(O, d, cams[0], p0, rows)
    got, st = dev.features(cams[0], p0, rows, want_stats=True, surfaces=True)
    assert_same_bits(got.reshape(-1), ref, (name, "surfaces"))
    SU.check_surface_counters(st, st_copy, words, W * H * SPP, d)
    assert_same_bits(dev.features(cams[0], p0, rows, surfaces=True).reshape(-1), ref, (name, "surfaces, plain instance"))
    for surfaces in (False, True):
        ref, st_ref, info = SP.oracle_specular_features(O, d, cams[1], p0, rows, surfaces)
        got, st = dev.features(cams[1], p0, rows, want_stats=True, surfaces=surfaces, specular=True)
        assert_same_bits(got.reshape(-1), ref, (name, "specular", surfaces))
        SP.check_specular_counters(st, st_ref, info, W * H * SPP, d, surfaces)
        assert_same_bits(dev.features(cams[1], p0, rows, surfaces=surfaces, specular=True).reshape(-1), ref, (name, "specular, plain instance", surfaces))
    # 8. rt_scatter: one step on the first hits of both cameras' own rays
    for key in (("outer", "camera"), ("inner", "camera")):
        q = np.ascontiguousarray(fams[key][0][:250], dtype=F.QUERY_RAY_DTYPE)
        h = hits[key][:250]
        recs, nxt, st = dev.scatter(q, h, BACKGROUND, want_stats=True)
        ref_recs, ref_nxt = np.zeros(len(q), dtype=F.SCATTER_REC_DTYPE), np.zeros(len(q), dtype=F.QUERY_RAY_DTYPE)
        tests = 0
        for i, (r, hh) in enumerate(zip(q, h)):
            ray = list(r["origin"]) + list(r["direction"]) + [float(r["time"])]
            state = SP.state_after(int(r["rng_state"]), int(hh["rng_draws"]))
            ref_recs[i], ref_nxt[i], _ = SC.step(O, d, ray, SC.hit_record(O, hh), state, BACKGROUND)
            if int(ref_recs[i]["status"]) == F.RT_SCATTER_DIFFUSE and d.n_lights:
                tests += SC.light_tests_per_record(d)
        assert_records(recs, ref_recs, (name, key, "records"))
        assert_records(nxt, ref_nxt, (name, key, "next rays"))
        assert st.rng_draws == int(ref_recs["rng_draws"].sum()) and st.light_pdf_tests == tests, (name, key)
    # 9. the closest hit does not depend on the tree: the root rebuilt by the device builder
    if F.ref_kind(d.root) == F.RT_KIND_NODE:
        d2 = rt.rebuild_bvh(d)
        dev2 = rt.DeviceScene(d2)
        assert dev2.info()["stack_need"] == T.stack_need(d2)
        _, worst2, _ = brute_check(dev2, profile, sc, fams, name, "rebuilt")
        worst = max(worst, worst2)
    log = os.environ.get("SCENE_GEN_LOG")
    if log:
        with open(log, "a") as f:
            f.write("%-10s paths %2d need %2d %-7s worst ambiguous share %.4f  worst |dt| / tolerance %.3e\n" % (
                name, facts["paths"], need, want["table"], share, worst))
