"""rt_intersect against the BVH-free reference of tests/brute_hits.py directly: prim is the winner's leaf ref (flip bit
included), t within the derived tolerance, media / ambiguity / the three named classes by the rules of tests/test_brute_hits.py.
The other GPU tests hold the device to the oracle bit for bit; this one holds it to geometry that never read a node box.

One case per shell of the query kernel (pt_traverse.hpp, trav_dispatch), at the smallest sizes of tests/trace_scenes.py that
select it, each through the plain and the counter instance, plus one scene each with movers, boxes and a small mesh:
  tiny-whole    stack need <= 16, n_nodes <= 1740: the whole node table in LDS
  tiny-partial  stack need <= 16, n_nodes > 1740: the table's first 1740 records in LDS
  small         stack need 17..22: no table
  mid, large    30 and 64 stack entries
rt_intersect never enters wf_trace: its single-precision slab test and nearer-child-first order (tuning bit 15) exist only in
renders, which return no t or prim. test_winner_through_wf_trace reaches them another way: every leaf is given a light of a
colour of its own, and rt_radiance at depth 1 returns the colour of the leaf each ray's traversal found."""
import numpy as np
import pytest

import brute_hits as B
import brute_scenes as S
import trace_scenes as T
from gpu_first import torch_first  # noqa: F401
from raytracer_2022_amd import _ffi as F

pytestmark = pytest.mark.gpu

REF_ORDER = 1 << 15                                      # rt2022_debug.h: tuning bit 15, the reference's child order
NODE_CACHE = T.NODE_CACHE


def query_shell(d, need):
    """trav_dispatch (pt_traverse.hpp), restated."""
    if need <= T.STACK_TINY:
        return "tiny-whole" if d.n_nodes <= NODE_CACHE else "tiny-partial"
    return "small" if need <= T.STACK_SMALL else "mid" if need <= T.STACK_MID else "large"


def scene_of(name):
    if name == "stack-20":
        return T.stack_need_scene(20)[:2]
    return S.make(name)


CASES = [("trace-feat7-whole", "tiny-whole"), ("trace-feat7-partial", "tiny-partial"), ("stack-20", "small"),
         ("trace-feat7-mid", "mid"), ("trace-feat7-large", "large"), ("trace-overflow", "tiny-whole"),
         ("every_kind", "tiny-whole"), ("cornell_smoke", "tiny-whole"), ("final_scene", None), ("wwscene", None)]


@pytest.fixture(scope="module")
def solved():
    """name → (desc, Scene, {family: (rays, Answer)}): the reference is computed once per scene and shared, unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            d, cam = scene_of(name)
            sc = B.Scene(d)
            fams = {}
            for family, rays in S.families(B, sc, cam, 300 + len(name)).items():
                ans = B.solve(sc, rays["origin"], rays["direction"], rays["time"], rays["t_min"], rays["t_max"])
                assert B.classify(sc, ans)[3].sum() <= S.AMBIGUOUS_SHARE * len(rays), (name, family)      # (before any result)
                fams[family] = (rays, ans)
            assert sum(len(r) for r, _ in fams.values()) * max(1, len(sc.paths)) < 2e7
            cache[name] = (d, sc, fams)
        return cache[name]
    return get


@pytest.mark.parametrize("name,shell", CASES, ids=[c[0] for c in CASES])
def test_intersect_against_brute_force(rt, solved, name, shell):
    d, sc, fams = solved(name)
    dev = rt.DeviceScene(d)
    if shell is not None:
        assert query_shell(d, dev.info()["stack_need"]) == shell
    compared = 0
    for family, (rays, ans) in fams.items():
        q = np.ascontiguousarray(rays, dtype=F.QUERY_RAY_DTYPE)
        got = dev.intersect(q)                                                           # the plain instance
        counted, st = dev.intersect(q, want_stats=True)                                  # the counter instance
        assert np.array_equal(got.view(np.uint8), counted.view(np.uint8)) and st.rays == len(q)
        ta, _ = B.compare(sc, rays, got["hit"], got["t"], got["rng_draws"], got["prim"], ans=ans)
        print(ta.line(name, family, "hip"))
        assert not ta.failures, (name, family, ta.failures[:5])
        assert ta.worst <= 1.0
        compared += ta.compared
        if not B.flat_node_paths(sc).any():
            assert ta.class1 == 0
        if not any(p.zoomed for p in sc.paths):
            assert ta.class2 == 0
    assert compared >= 0.5 * S.N_RAYS


@pytest.mark.parametrize("name", ["trace-feat3-whole", "trace-spheres-large", "random_scene", "wwscene"])
def test_any_hit_answers_hit_iff_the_reference_has_a_candidate(rt, solved, name):
    d, sc, fams = solved(name)
    assert not sc.media
    dev = rt.DeviceScene(d)
    for family, (rays, ans) in fams.items():
        q = np.ascontiguousarray(rays, dtype=F.QUERY_RAY_DTYPE)
        got = dev.intersect(q, any_hit=True)
        class1, class2, class3, amb = B.classify(sc, ans)
        check = ~(class1 | class2 | class3 | amb)
        bad = np.flatnonzero(check & (got["hit"].astype(bool) != ans.hit))
        print("%-22s %-7s any-hit rays %5d compared %5d hits %5d" % (name, family, len(q), check.sum(), (got["hit"][check] == 1).sum()))
        assert len(bad) == 0, (name, family, [(int(i), bool(ans.hit[i]), float(ans.t[i]), ans.margin[i]) for i in bad[:5]])
        h = np.flatnonzero(check & ans.hit)
        assert np.all(got["t"][h] >= np.asarray(ans.t[h], dtype=np.float64) - B.tolerance(ans, rays["direction"])[h])


# ---- the winner through wf_trace: every leaf a light of its own colour ------------------------------------------------------------
LEAF_POOLS = {B.K_SPHERE: "spheres", B.K_MOVING_SPHERE: "moving_spheres", B.K_RECT: "rects", B.K_BOX: "boxes", B.K_TRIANGLE: "triangles",
              B.K_RING: "rings"}
BACKGROUND = (0.25, 0.5, 0.75)


def colour_of(kind, index):
    return (float(kind), float(1 + index // 1024), float(1 + index % 1024))


def lit_copy(rt, d):
    """The desc's geometry (same pools, same BVH, same boxes) with every solid leaf's material replaced by a DiffuseLight of
    the colour colour_of(kind, index): ray_color at depth 1 returns that colour for a front-face hit, black for a back face
    and the background for a miss. Media keep their Isotropic material (black at depth 1)."""
    import ctypes as C
    out = F.rt_scene_desc.from_buffer_copy(d)
    keep = [d]
    mats = [d.materials[i] for i in range(d.n_materials)]
    texs = [d.textures[i] for i in range(d.n_textures)]
    for kind, pool in LEAF_POOLS.items():
        n = getattr(d, "n_" + pool)
        if not n:
            continue
        ctype = type(getattr(d, pool)[0])
        arr = (ctype * n)()
        C.memmove(arr, getattr(d, pool), n * C.sizeof(ctype))
        for i in range(n):
            texs.append(F.rt_texture(kind=F.RT_TEX_SOLID, color=F.d3(*colour_of(kind, i))))
            mats.append(F.rt_material(kind=F.RT_MAT_DIFFUSE_LIGHT, tex=len(texs) - 1))
            arr[i].mat = len(mats) - 1
        setattr(out, pool, C.cast(arr, C.POINTER(ctype)))
        keep.append(arr)
    m_arr, t_arr = (F.rt_material * len(mats))(*mats), (F.rt_texture * len(texs))(*texs)
    out.n_materials, out.materials = len(mats), C.cast(m_arr, C.POINTER(F.rt_material))
    out.n_textures, out.textures = len(texs), C.cast(t_arr, C.POINTER(F.rt_texture))
    out.n_lights = 0
    out._keep = keep + [m_arr, t_arr]
    return out


def near_view(rt, eye, at):
    return rt.camera_new(eye, at, (0, 1, 0), 60.0, T.W / T.H, 0.0, 3.0, 0.0, 1.0)


def wf_scene(rt, name):
    """(scene, tuning, the facts of the wf_trace instance the case stands for)."""
    if name == "whole-f32":
        return S.make("trace-spheres-801"), T.TUNING, ("whole", True)               # (the view from inside the cloud)
    if name == "whole-f64":
        return T.make_scene(6, "whole", 2)[:2], T.TUNING, ("whole", False)
    if name == "partial":                                       # (seen from the front of the cloud of small spheres, which the
        # bounce, random and axis families still hit from close by: the 3 % bound with t_max = +inf)
        return (T.make_scene(4, "partial", 2)[0], near_view(rt, (0.0, 2.5, -4.5), (0.0, 1.0, 0.0))), T.TUNING, ("partial", False)
    if name == "no-table":
        return T.make_scene(6, "small", 2)[:2], T.TUNING | T.NO_TABLE, ("plain", False)
    assert name == "stack-64"                                   # (seen from half the distance: the row of spheres of radius 0.18)
    return (T.make_scene(0, "large", 2, True)[0], near_view(rt, (0.0, 2.5, 4.0), (0.0, 1.5, -2.0))), T.TUNING, ("plain", True)


@pytest.mark.parametrize("name", ["whole-f32", "whole-f64", "partial", "no-table", "stack-64"])
def test_winner_through_wf_trace(rt, name):
    """The timed wf_trace instance of the case — asserted from the restated choice — with the nearer child first and with the
    reference's order (tuning bit 15). For every ray with the render's window (t_min 0.001, t_max +inf) that is not ambiguous,
    tied or of a named class, the radiance is exactly what the reference's winner says:
      - no candidate: the background, or black if the ray crosses a medium's chord (it may scatter there);
      - a winner reached through no mover: its colour if the reference finds its front face (the ray against the outward
        normal, turned over by FlipFace), black if its back face; black too if a medium's chord is crossed before it;
      - a winner under movers (their set_face_normal calls recompute the face): its colour or black."""
    (d0, cam), tuning, (table, f32) = wf_scene(rt, name)
    d = lit_copy(rt, d0)
    sc = B.Scene(d)
    dev = rt.DeviceScene(d)
    dev.set_tuning(tuning)
    want = T.expected_variant(d, dev.info()["stack_need"], tuning)
    assert (want["table"], want["f32_slabs"]) == (table, f32), want
    assert dev.trace_variant() == {k: v for k, v in want.items() if k != "table"}
    fams = S.families(B, sc, cam, 500 + len(name))
    rays = np.concatenate(list(fams.values()))
    family = np.concatenate([np.full(len(r), i) for i, r in enumerate(fams.values())])
    rays["t_min"], rays["t_max"] = 0.001, np.inf
    ans = B.solve(sc, rays["origin"], rays["direction"], rays["time"], 0.001, np.inf)
    class1, class2, class3, amb = B.classify(sc, ans)
    for i, fam in enumerate(fams):
        assert amb[family == i].sum() <= S.AMBIGUOUS_SHARE * (family == i).sum(), (name, fam, int(amb[family == i].sum()))
    check = ~(class1 | class2 | class3 | amb | ans.tie)
    assert check.sum() >= 0.9 * len(rays)
    colour = np.array([colour_of(B.ref_kind(l), B.ref_index(l)) if h else BACKGROUND for l, h in zip(ans.leaf, ans.hit)])
    rr = rt.radiance_rays(rays["origin"], rays["direction"], time=rays["time"], rng_state=rays["rng_state"])
    in_medium = np.zeros(len(rays), bool)
    for m in sc.media:
        t_in, _, crossed = B.chord(sc, m, rays["origin"], rays["direction"], rays["time"], 0.001, np.inf)
        in_medium |= crossed & (t_in < ans.t)
    faced = ans.hit & ~ans.moved & ~in_medium                                           # the reference knows the face
    must_colour = ~in_medium & (~ans.hit | (faced & ans.front))
    must_black = faced & ~ans.front
    for word, ordered in ((tuning, True), (tuning | REF_ORDER, False)):
        dev.set_tuning(word)
        assert dev.child_order()["timed"] == ordered
        out = dev.radiance(rr, spp=1, background=BACKGROUND, t_min=0.001, max_depth=1)
        black = (out == 0).all(1)
        same = (out == colour).all(1)
        ok = np.where(must_colour, same, np.where(must_black, black, same | black))
        bad = np.flatnonzero(check & ~ok)
        print("%-10s %-9s rays %5d compared %5d: colour required %5d, black required %5d, either %5d" % (
            name, "ordered" if ordered else "ref-order", len(rays), check.sum(), (check & must_colour).sum(), (check & must_black).sum(),
            (check & ~must_colour & ~must_black).sum()))
        assert len(bad) == 0, (name, ordered, [(int(i), out[i].tolist(), colour[i].tolist(), float(ans.t[i]), bool(ans.front[i])) for i in bad[:5]])
        assert (check & must_colour & ans.hit).sum() >= 100 and (check & must_black).sum() >= 20 and (check & must_colour & ~ans.hit).sum() >= 50
