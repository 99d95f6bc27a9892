"""The scenes of tests/trace_scenes.py, checked on the oracle alone (no GPU): every case has the feature word it was asked for,
its rays reach every object kind the word promises and no other, paths go on past the camera ray, and the node count and
stack need sit where the instance the case is meant to select needs them. So the device tests of
tests/test_trace_instances.py cannot pass on an arm that no ray enters."""
import pytest

import trace_scenes as T
from raytracer_2022_amd import _ffi as F


@pytest.mark.parametrize("case", T.matrix_cases(), ids=T.case_id)
def test_matrix_scene_reaches_what_its_feature_word_promises(O, case):
    feat, shape, sphere_only = case
    d, cam, p, rows = T.make_scene(feat, shape, 1, sphere_only)
    assert T.feature_word(d) == feat
    assert (d.n_rects == 0) == sphere_only
    ref, st = O.render_cpu(d, cam, p, rows, n_threads=4, want_stats=True)
    promised = T.promised_kinds(feat, sphere_only)
    for k in range(1, F.RT_KIND_COUNT):
        assert (st.prim_tests[k] > 0) == (k in promised), (F.KIND_NAMES[k], st.prim_tests[k])
    assert st.rays > T.W * T.H * T.SPP and st.node_visits > 0
    need = T.stack_need(d)
    if shape == "partial":
        assert d.n_nodes > T.NODE_CACHE and need <= T.STACK_TINY
    elif shape in ("whole", "small"):
        assert d.n_nodes <= T.NODE_CACHE and need <= T.STACK_TINY
    elif shape == "mid":
        assert T.STACK_SMALL < need <= T.STACK_MID
    else:
        assert T.STACK_MID < need <= T.STACK_LARGE
    if shape in ("mid", "large"):
        # every link of the chain is visited by every ray: its box holds the camera and the whole scene
        base = T.make_scene(feat, "whole", 1, sphere_only)[0]
        links = d.n_nodes - base.n_nodes
        assert links == need - T.stack_need(base) and links >= 15
        assert st.node_visits >= links * st.rays
    if feat & 4 and feat & 2:                             # the medium's boundary lies under movers, and is one primitive
        assert F.ref_kind(d.media[0].boundary) == F.RT_KIND_TRANSLATE and not T.mega_refuses(d)


def test_expected_variant_of_the_matrix():
    """The restated choice, per case: the table each shape is built for — and the two meshes without boxes or media (FEAT 1, 3)
    that choose_trace sends to the plain single-precision kernels instead of the partial table."""
    for feat, shape, sphere_only in T.matrix_cases():
        d = T.make_scene(feat, shape, 1, sphere_only)[0]
        v = T.expected_variant(d, T.stack_need(d), T.TUNING | (T.NO_TABLE if shape == "small" else 0))
        want = {"whole": "prims" if sphere_only else "whole", "partial": "plain" if feat in (1, 3) else "partial"}.get(shape, "plain")
        assert v["table"] == want, (feat, shape, v)
        assert v["stack_entries"] == {"whole": 16, "partial": 22 if feat in (1, 3) else 16, "small": 22, "mid": 30, "large": 64}[shape]
        assert v["f32_slabs"] == (sphere_only or (want == "plain" and feat in (1, 3)))


@pytest.mark.parametrize("mid", [False, True], ids=["list-root", "mid-chain"])
def test_overflow_scene_reaches_the_records_behind_the_tables(O, mid):
    d, cam, p, rows, mats = T.overflow_scene(mid=mid)
    assert T.feature_word(d) == 7 and not T.mega_refuses(d)
    assert d.n_xforms >= 12 and d.n_media == 5 and d.n_lights == 12
    assert len(set(mats["movers"])) == 12 and len(set(mats["media"])) == 5
    need = T.stack_need(d)
    assert (T.STACK_SMALL < need <= T.STACK_MID) if mid else need <= T.STACK_TINY
    # every mover and every medium is what some camera ray of the view hits first
    Wv, Hv, spp = T.OVERFLOW_VIEW
    origins, dirs = T.pinhole_rays(cam, Wv, Hv)
    first = set()
    for i in range(len(origins)):
        rec = O.hit(d, d.root, origins[i], dirs[i], tm=0.5, rng_state=i + 1)
        if rec.hit:
            first.add(rec.mat)
    assert set(mats["movers"]) <= first and set(mats["media"]) <= first
    # the mover and medium records of those objects: more than the 8 and the 2 the kernels keep in LDS
    seen_xf = {i for i in range(d.n_xforms) if _leaf_mat(d, d.xforms[i].child) in set(mats["movers"])}
    assert len([i for i in seen_xf if i >= 8]) >= 4 and d.n_media - 2 >= 3
    # a uniform index over 12 lights: the chance that none of n draws is >= 8 is (2 / 3)^n
    ref, st = O.render_cpu(d, cam, p, rows, n_threads=4, want_stats=True)
    assert st.rays - Wv * Hv * spp >= 1000 and st.light_pdf_tests >= 12 * 1000
    assert all(st.prim_tests[k] > 0 for k in range(1, F.RT_KIND_COUNT) if k != F.RT_KIND_MOVING_SPHERE)


def _leaf_mat(d, ref):
    """The material of the primitive under a chain of movers (None for anything else)."""
    while F.RT_KIND_TRANSLATE <= F.ref_kind(ref) <= F.RT_KIND_ZOOM:
        ref = d.xforms[F.ref_index(ref)].child
    pool = {F.RT_KIND_SPHERE: d.spheres, F.RT_KIND_BOX: d.boxes}.get(F.ref_kind(ref))
    return pool[F.ref_index(ref)].mat if pool is not None else None


def test_threshold_scenes_sit_one_apart():
    for n in (1739, 1740, 1741):
        d = T.node_count_scene(n)[0]
        assert d.n_nodes == n and d.n_rects == 2 and T.feature_word(d) == 0 and T.stack_need(d) <= T.STACK_TINY
        assert T.expected_variant(d, T.stack_need(d))["table"] == ("whole" if n <= 1740 else "partial")
    for kw, table in ((dict(n_spheres=256), "prims"), (dict(n_spheres=257), "whole"), (dict(n_spheres=4, n_moving=512), "prims"),
                      (dict(n_spheres=4, n_moving=513), "whole"), (dict(n_nodes=600), "prims"), (dict(n_nodes=601), "whole")):
        d = T.sphere_count_scene(**kw)[0]
        assert d.n_rects == 0 and T.feature_word(d) == 0 and T.stack_need(d) <= T.STACK_TINY
        if "n_nodes" in kw:
            assert d.n_nodes == kw["n_nodes"] and d.n_spheres <= T.PRIM_SPHERES and d.n_moving_spheres <= T.PRIM_MOVING
        else:
            assert d.n_spheres == kw["n_spheres"] and d.n_moving_spheres == kw.get("n_moving", 0) and d.n_nodes <= T.PRIM_NODES
        assert T.expected_variant(d, T.stack_need(d))["table"] == table, kw
    for need, stack in ((16, 16), (17, 22), (22, 22), (23, 30), (30, 30), (31, 64), (64, 64)):
        d = T.stack_need_scene(need)[0]
        assert T.stack_need(d) == need and T.expected_variant(d, need)["stack_entries"] == stack
