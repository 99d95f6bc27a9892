"""The timed traversal kernels visit the nearer child of a BVH node first where the result cannot change (wf_trace, kOrder;
DESIGN.md §4.13). Every case here renders with a timed kernel in both modes — ordered, and the reference's order forced by
tuning bit 15 — and compares the pixel sums with the CPU oracle bit for bit: scenes with exact ties in t under nodes that
swap, seen from all eight octants; a medium between reorderable subtrees inside a Translate(RotateY(bvh)); one scene per
instance family. The counting kernel keeps the reference's order: its counters stay the oracle's."""
import ctypes as C

import numpy as np
import pytest

import trace_scenes as T
from raytracer_2022_amd import _ffi as F
from compare import same_bits
from gpu_first import torch_first  # noqa: F401

pytestmark = pytest.mark.gpu

REF_ORDER = 1 << 15                                      # rt2022_debug.h: tuning bit 15
W = H = 48
OCTANTS = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]


# ---- scenes over the reference's own BVH builder -------------------------------------------------------------------------
def add_bvh(rt, b, leaves, seed):
    """BvhNode::new_list (rtb_bvh_build) over leaves [(ref, lo, hi)], appended to the builder's node pool → the root's ref."""
    n = len(leaves)
    refs = (C.c_uint32 * n)(*[l[0] for l in leaves])
    flat = (C.c_double * (6 * n))(*[x for l in leaves for x in (*l[1], *l[2])])
    out = (F.rt_bvh_node * (2 * n + 2))()
    cnt = rt.lib().rtb_bvh_build(refs, flat, n, seed, out, 2 * n + 2)
    assert cnt > 0
    base = len(b.pools["nodes"])

    def moved(ref):
        return F.make_ref(F.RT_KIND_NODE, F.ref_index(ref) + base) if F.ref_kind(ref) == F.RT_KIND_NODE else ref
    for i in range(cnt):
        b.node(tuple(out[i].bmin), tuple(out[i].bmax), moved(out[i].left), moved(out[i].right))
    return F.make_ref(F.RT_KIND_NODE, base)                # (the builder's root is its record 0)


def sphere_box(c, r):
    return tuple(x - r for x in c), tuple(x + r for x in c)


def tie_scene(rt, kind, seed):
    """A dozen spheres round the origin and, among them, a pair that every ray hits at exactly the same t: two coincident
    spheres (a light and a Lambertian) or two coplanar overlapping rects (a metal and a Lambertian). → (desc, the pair's refs)."""
    b = rt.DescBuilder()
    g = np.random.default_rng(100 + seed)
    leaves = []
    for i in range(12):
        c = tuple(float(x) for x in g.uniform(-3.0, 3.0, 3))
        if max(abs(x) for x in c) < 1.4:
            c = (c[0] + 2.0, c[1], c[2] - 2.0)
        r = float(g.uniform(0.3, 0.6))
        m = b.lambertian(tuple(g.uniform(0.2, 0.9, 3))) if i % 3 else b.metal((0.8, 0.8, 0.7), 0.05)
        leaves.append((b.sphere(c, r, m), *sphere_box(c, r)))
    if kind == "spheres":
        lamp, lam = b.diffuse_light((4.0, 3.0, 2.0)), b.lambertian((0.2, 0.7, 0.3))
        pair = [b.sphere((0.0, 0.0, 0.0), 1.0, lamp), b.sphere((0.0, 0.0, 0.0), 1.0, lam)]
        # (the light list holds a lamp of its own: a path scattered on the Lambertian twin starts ON the coincident light, where
        # Sphere::pdf_value takes the root of 1 - r^2 / |c - o|^2 = 0 give or take a rounding — a NaN by chance, in the reference too)
        sun = b.sphere((0.5, 7.0, -0.5), 0.8, b.diffuse_light((6.0, 6.0, 5.0)))
        leaves.append((sun, *sphere_box((0.5, 7.0, -0.5), 0.8)))
        b.light(sun)
        boxes = [sphere_box((0.0, 0.0, 0.0), 1.0)] * 2
    else:
        metal, lam = b.metal((0.9, 0.6, 0.2), 0.0), b.lambertian((0.2, 0.3, 0.8))
        pair = [b.rect(F.RT_RECT_XZ, -1.2, 0.6, -1.0, 1.0, 0.0, metal), b.rect(F.RT_RECT_XZ, -0.6, 1.2, -0.8, 1.1, 0.0, lam)]
        boxes = [((-1.2, -0.0001, -1.0), (0.6, 0.0001, 1.0)), ((-0.6, -0.0001, -0.8), (1.2, 0.0001, 1.1))]        # aarect.rs:123-128
    order = g.permutation(2)
    for j in order:                                           # (either of the two may come first in the builder's input)
        leaves.insert(int(g.integers(0, len(leaves) + 1)), (pair[j], *boxes[j]))
    b.set_root(add_bvh(rt, b, leaves, seed))
    d = b.desc()
    d._builder = b
    return d, pair


def octant_camera(rt, octant):
    look_from = tuple(s * v for s, v in zip(octant, (5.0, 3.5, 6.0)))
    return rt.camera_new(look_from, (0.0, 0.0, 0.0), (0, 1, 0), 40.0, W / H, 0.0, 8.0, 0.0, 1.0), look_from


# ---- the upload pass, restated for these scenes (spheres, rects and nodes) ---------------------------------------------
def centre2(d, ref):
    kind, i = F.ref_kind(ref), F.ref_index(ref)
    if kind == F.RT_KIND_NODE:
        return [d.nodes[i].bmin[a] + d.nodes[i].bmax[a] for a in range(3)]
    if kind == F.RT_KIND_SPHERE:
        s = d.spheres[i]
        return [(s.center[a] - s.radius) + (s.center[a] + s.radius) for a in range(3)]
    assert kind == F.RT_KIND_RECT and d.rects[i].axis == F.RT_RECT_XZ
    r = d.rects[i]
    return [r.a0 + r.a1, (r.k - 0.0001) + (r.k + 0.0001), r.b0 + r.b1]


def node_order(d, i):
    """child_order (csrc/host/scene_check.cpp) for a node of a medium-free BVH of unflipped spheres and rects: (axis, sense) or None."""
    n = d.nodes[i]
    if n.left == n.right:
        return None
    diff = [r - l for l, r in zip(centre2(d, n.left), centre2(d, n.right))]
    axis = max(range(3), key=lambda a: (abs(diff[a]), -a))
    if diff[axis] == 0.0:
        return None
    return axis, 0 if diff[axis] > 0.0 else 1


def leaves_below(d, ref):
    if F.ref_kind(ref) != F.RT_KIND_NODE:
        return [ref]
    n = d.nodes[F.ref_index(ref)]
    return leaves_below(d, n.left) + ([] if n.right == n.left else leaves_below(d, n.right))


def parting_node(d, pair):
    """The node with one of the pair in each subtree — where the order of the visits decides which is met first — and the
    pair in the reference's depth-first order (rank order)."""
    ref = d.root
    while True:
        n = d.nodes[F.ref_index(ref)]
        l, r = leaves_below(d, n.left), leaves_below(d, n.right)
        if any(p in l for p in pair) and any(p in r for p in pair) and n.left != n.right:
            first = [p for p in pair if p in l][0]
            return F.ref_index(ref), [first] + [p for p in pair if p != first]
        ref = n.left if all(p in l for p in pair) else n.right


def swaps_for(order, direction):
    """wf_trace: a node of (axis, sense) is entered right child first by a ray going down the axis (sense 0) or up it (sense 1)."""
    if order is None:
        return False
    axis, sense = order
    return direction[axis] < 0.0 if sense == 0 else direction[axis] > 0.0


# ---- 1. ties ---------------------------------------------------------------------------------------------------------------
SEEDS = (1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def swap_log():
    """(kind, seed) → the pair's parting node swaps for some camera's viewing direction; filled by the cases, read by the last test."""
    return {}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind", ("spheres", "rects"))
def test_ties_from_all_octants(rt, O, swap_log, kind, seed):
    """The tied pair under the reference's own BVH, seen from all eight octants (every sign mask occurs), in both modes: the
    pixels are the oracle's — the winner of every tie is the one the reference visits last."""
    d, pair = tie_scene(rt, kind, seed)
    dev = rt.DeviceScene(d)
    node, ranked = parting_node(d, pair)
    order = node_order(d, node)
    p = rt.make_params(W, H, 4, 12, (0.5, 0.6, 0.8), seed=seed)
    rows = rt.shuffled_rows(H, seed)
    swapped = False
    for octant in OCTANTS:
        cam, look_from = octant_camera(rt, octant)
        swapped = swapped or swaps_for(order, tuple(-x for x in look_from))
        ref = O.render_cpu(d, cam, p, rows, n_threads=8)
        for word, ordered in ((T.TUNING, True), (T.TUNING | REF_ORDER, False)):
            dev.set_tuning(word)
            assert dev.child_order() == {"timed": ordered, "counting": False}
            out = dev.render(cam, p, rows)
            assert same_bits(out, ref, payloads=True), (kind, seed, octant, "ordered" if ordered else "reference order")
    swap_log[(kind, seed)] = swapped
    assert len(ranked) == 2


def test_some_seed_parts_the_pair_under_a_swapping_node(swap_log):
    """Per kind of tie, at least one seed's BVH has the pair parted by a node that is entered right child first from some octant
    (worked out above from the restated order bits): the tie rule was exercised, not bypassed."""
    for kind in ("spheres", "rects"):
        seen = [v for (k, _), v in swap_log.items() if k == kind]
        assert len(seen) == len(SEEDS), "run the whole module: this test reads what the tie cases found"
        assert any(seen), kind


# ---- 2. a medium between reorderable subtrees, inside Translate(RotateY(bvh)) ------------------------------------------------
def union(a, b):
    return tuple(min(x, y) for x, y in zip(a[0], b[0])), tuple(max(x, y) for x, y in zip(a[1], b[1]))


def medium_scene(rt, seed=3):
    b = rt.DescBuilder()
    g = np.random.default_rng(seed)

    def cluster(cx):
        items = []
        for _ in range(4):
            c = (cx + float(g.uniform(-0.8, 0.8)), float(g.uniform(0.0, 1.6)), float(g.uniform(-0.8, 0.8)))
            r = float(g.uniform(0.25, 0.45))
            items.append((b.sphere(c, r, b.lambertian(tuple(g.uniform(0.3, 0.9, 3)))), sphere_box(c, r)))
        (r0, b0), (r1, b1), (r2, b2), (r3, b3) = items
        l, r = union(b0, b1), union(b2, b3)
        box = union(l, r)
        return b.node(*box, b.node(*l, r0, r1), b.node(*r, r2, r3)), box
    left, lbox = cluster(-2.4)
    right, rbox = cluster(2.4)
    fog_box = sphere_box((0.0, 0.8, 0.0), 1.0)
    fog = b.medium(b.sphere((0.0, 0.8, 0.0), 1.0, b.dielectric(1.5)), 0.9, b.isotropic((0.9, 0.9, 0.95)))
    inner_box = union(fog_box, rbox)
    inner = b.node(*inner_box, fog, right)
    bvh = b.node(*union(lbox, inner_box), left, inner)
    moved = b.translate(b.rotate_y(bvh, 0.5, 0.8660254037844386), (0.3, 0.0, -0.5))
    floor_ = b.rect(F.RT_RECT_XZ, -12, 12, -12, 12, -0.5, b.lambertian((0.5, 0.5, 0.5)))
    lamp = b.rect(F.RT_RECT_XZ, -2, 2, -2, 2, 6.0, b.diffuse_light((7, 7, 6)), flip=True)
    b.light(F.make_ref(F.RT_KIND_RECT, F.ref_index(lamp)))
    b.set_root(b.list([floor_, lamp, moved]))
    d = b.desc()
    d._builder = b
    return d


def test_medium_between_reorderable_subtrees(rt, O):
    """Both clusters are reordered, the nodes above the medium are not: the medium is visited with the closest hit the reference
    has at that point, makes the same draws — pixels equal in both modes, from two sides; the counting render's rng_draws (and
    every other counter) are the oracle's."""
    d = medium_scene(rt)
    dev = rt.DeviceScene(d)
    p = rt.make_params(W, H, 8, 12, (0.1, 0.12, 0.2), seed=5)
    rows = rt.shuffled_rows(H, 5)
    for look_from in ((6.0, 3.0, 7.0), (-7.0, 2.5, -5.0)):
        cam = rt.camera_new(look_from, (0.0, 0.8, 0.0), (0, 1, 0), 40.0, W / H, 0.0, 9.0, 0.0, 1.0)
        ref, st_ref = O.render_cpu(d, cam, p, rows, n_threads=8, want_stats=True)
        assert st_ref.as_dict()["prim_tests"][F.RT_KIND_MEDIUM] > 0 and st_ref.as_dict()["rng_draws"] > 0
        for word, ordered in ((T.TUNING, True), (T.TUNING | REF_ORDER, False)):
            dev.set_tuning(word)
            assert dev.child_order()["timed"] == ordered
            assert same_bits(dev.render(cam, p, rows), ref, payloads=True), (look_from, ordered)
        dev.set_tuning(T.TUNING)
        out, st = dev.render(cam, p, rows, want_stats=True)
        assert same_bits(out, ref, payloads=True)
        assert st.as_dict()["rng_draws"] == st_ref.as_dict()["rng_draws"]
        assert st.as_dict() == st_ref.as_dict()


# ---- 3. one scene per instance family -------------------------------------------------------------------------------------------
def family_scene(name):
    """(scene, tuning, the table and f32 facts the family stands for)."""
    if name == "whole-f64":
        return T.make_scene(6, "whole", 2), T.TUNING, ("whole", False)
    if name == "whole-f32":
        return T.sphere_count_scene(n_nodes=801), T.TUNING, ("whole", True)
    if name == "all-in-lds":
        return T.make_scene(0, "whole", 2, True), T.TUNING, ("prims", True)
    if name == "partial":
        return T.make_scene(4, "partial", 2), T.TUNING, ("partial", False)
    if name == "plain22-nodes32":
        return T.make_scene(0, "small", 2, True), T.TUNING | T.NO_TABLE, ("plain", True)
    if name == "plain30-nodes32":
        return T.make_scene(0, "mid", 2, True), T.TUNING, ("plain", True)
    if name == "plain64-nodes32":
        return T.make_scene(0, "large", 2, True), T.TUNING, ("plain", True)
    if name == "plain22-f64":
        return T.make_scene(6, "small", 2), T.TUNING | T.NO_TABLE, ("plain", False)
    assert name == "mesh"
    return T.make_scene(1, "mid", 2), T.TUNING, ("plain", True)


FAMILIES = ("whole-f64", "whole-f32", "all-in-lds", "partial", "plain22-nodes32", "plain30-nodes32", "plain64-nodes32", "plain22-f64", "mesh")


@pytest.mark.parametrize("family", FAMILIES)
def test_instance_family(rt, O, family):
    """The family's timed instance — asserted from the restated choice — in both modes against the oracle; trace_variant says
    "ordered" for it and not for the counting instance, whose node_visits and prim_tests stay the oracle's."""
    (d, cam, p, rows), tuning, (table, f32) = family_scene(family)
    dev = rt.DeviceScene(d)
    dev.set_tuning(tuning)
    want = T.expected_variant(d, dev.info()["stack_need"], tuning)
    assert (want["table"], want["f32_slabs"]) == (table, f32), want
    assert dev.trace_variant() == {k: v for k, v in want.items() if k != "table"}
    stacks = {"plain22-nodes32": 22, "plain30-nodes32": 30, "plain64-nodes32": 64, "plain22-f64": 22, "mesh": 30}
    if family in stacks:
        assert want["stack_entries"] == stacks[family]
    ref, st_ref = O.render_cpu(d, cam, p, rows, n_threads=8, want_stats=True)
    for word, ordered in ((tuning, True), (tuning | REF_ORDER, False)):
        dev.set_tuning(word)
        assert dev.child_order() == {"timed": ordered, "counting": False}
        assert same_bits(dev.render(cam, p, rows), ref, payloads=True), (family, "ordered" if ordered else "reference order")
    dev.set_tuning(tuning)
    out, st = dev.render(cam, p, rows, want_stats=True)
    assert same_bits(out, ref, payloads=True)
    got, exp = st.as_dict(), st_ref.as_dict()
    assert got["node_visits"] == exp["node_visits"] and list(got["prim_tests"]) == list(exp["prim_tests"])
    assert got == exp
