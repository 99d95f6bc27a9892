"""Scenes built to select one traversal-kernel instance each (wf_trace: pt_wavefront_trace.hip, choose_trace), and the Python
restatements the tests compare the library's choice with. No GPU is needed to build or to check a scene: the oracle alone
says which object kinds its rays reach (tests/test_trace_scenes.py); tests/test_trace_instances.py then runs every case on the
device.

A case is (feat, shape): `feat` is the feature word rt_scene_create computes from the pool counts (bit 1 = triangles or rings,
bit 2 = movers or lists, bit 4 = boxes or media), `shape` what decides the table and the stack of the instance:

  whole    n_nodes <= 1740 and a stack need <= 16: the whole node table in LDS
  partial  a median-split BVH of over 900 leaves: n_nodes > 1740, the stack need still <= 16
  small    the `whole` scene, rendered with tuning bit 28 (no node table): the plain 22-entry kernels
  mid      the `whole` scene under a left-leaning chain of nodes: a stack need in 23..30
  large    ... a longer chain: a stack need in 31..64
"""
import sys

import numpy as np

import raytracer_2022_amd as rt
from raytracer_2022_amd import _ffi as F

SHAPES = ("whole", "partial", "small", "mid", "large")
W, H, SPP, MAX_DEPTH = 40, 30, 4, 12
TUNING = 18 | (1 << 8) | (2 << 12) | (8 << 16) | (2 << 20) | (1 << 24)       # DeviceScene.set_tuning's default word
NO_TABLE, PROBE, LITERAL_STEP = 1 << 28, 1 << 29, 1 << 30                    # rt2022_debug.h: tuning bits 28, 29, 30
# pt_device.h
STACK_TINY, STACK_SMALL, STACK_MID, STACK_LARGE = 16, 22, 30, 64
NODE_CACHE, PRIM_NODES, PRIM_SPHERES, PRIM_MOVING = 1740, 600, 256, 512
MID_NEED, LARGE_NEED = 27, 48                                                # stack needs the `mid` / `large` chains are cut to
EPS = 1e-4
WORLD = ((-250.0, -250.0, -250.0), (250.0, 250.0, 250.0))                    # the box of every chain link: it holds every object (the
                                                                             # ground spheres reach y = -200.5) and the camera

# kinds each feature bit promises / the base scene holds (indices of rt_stats.prim_tests)
BASE_KINDS = (F.RT_KIND_SPHERE, F.RT_KIND_MOVING_SPHERE, F.RT_KIND_RECT)
SPHERE_KINDS = (F.RT_KIND_SPHERE, F.RT_KIND_MOVING_SPHERE)
BIT_KINDS = {1: (F.RT_KIND_TRIANGLE, F.RT_KIND_RING),
             2: (F.RT_KIND_TRANSLATE, F.RT_KIND_ROTATE_Y, F.RT_KIND_ZOOM, F.RT_KIND_LIST),
             4: (F.RT_KIND_BOX, F.RT_KIND_MEDIUM)}


# ---- BVHs of chosen shape --------------------------------------------------------------------------------------------
def median_split_bvh(b, leaves):
    """A BVH over `leaves` [(ref, lo, hi)]: halved at the median along x, y, z in turn, a span-1 node (the same child twice,
    bvh/mod.rs:44-47) per leaf: 2 n - 1 nodes."""
    def build(items, axis=0):
        if len(items) == 1:
            r, lo, hi = items[0]
            return b.node(lo, hi, r, r), lo, hi
        items = sorted(items, key=lambda it: it[1][axis])
        h = len(items) // 2
        l, llo, lhi = build(items[:h], (axis + 1) % 3)
        r, rlo, rhi = build(items[h:], (axis + 1) % 3)
        lo = tuple(min(a, c_) for a, c_ in zip(llo, rlo)); hi = tuple(max(a, c_) for a, c_ in zip(lhi, rhi))
        return b.node(lo, hi, l, r), lo, hi
    return build(leaves)[0]


def paired_leaf_bvh(b, leaves):
    """The same split with two different primitives per lowest node where two are left: n - 1 nodes for an even n, n for an odd one."""
    def build(items, axis=0):
        lo = tuple(min(it[1][k] for it in items) for k in range(3)); hi = tuple(max(it[2][k] for it in items) for k in range(3))
        if len(items) <= 2:
            return b.node(lo, hi, items[0][0], items[-1][0])
        items = sorted(items, key=lambda it: it[1][axis])
        h = len(items) // 2
        h += h & 1                                       # (an even left half: at most one lowest node holds a single leaf)
        return b.node(lo, hi, build(items[:h], (axis + 1) % 3), build(items[h:], (axis + 1) % 3))
    return build(leaves)


def chain(b, ref, links, right_child):
    """`links` nodes leaning left over `ref`, every one with the box WORLD and right_child(i) for its right child: a ray inside
    WORLD visits them all, and each adds one entry to the traversal stack's need."""
    for i in range(links):
        ref = b.node(WORLD[0], WORLD[1], ref, right_child(i))
    return ref


# ---- restatements of the library's rules -----------------------------------------------------------------------------
def feature_word(d):
    """rt_scene_create: the feature word, from the pool counts."""
    return ((1 if d.n_triangles or d.n_rings else 0) | (2 if d.n_xforms or d.n_lists else 0) | (4 if d.n_boxes or d.n_media else 0))


def stack_need(d):
    """Validator::need (csrc/host/scene_check.cpp): the stack entries a traversal of the scene needs."""
    memo = {}

    def need(ref):
        kind, idx = F.ref_kind(ref), F.ref_index(ref)
        if kind == F.RT_KIND_NODE:
            if idx not in memo:
                n = d.nodes[idx]
                nl = need(n.left)
                memo[idx] = max(1 + nl, nl if n.right == n.left else need(n.right))
            return memo[idx]
        if F.RT_KIND_TRANSLATE <= kind <= F.RT_KIND_ZOOM:
            return 1 + need(d.xforms[idx].child)
        if kind == F.RT_KIND_LIST:
            l = d.lists[idx]
            return max([max(1, l.count)] + [l.count - 1 - i + need(d.list_items[l.first + i]) for i in range(l.count)])
        if kind == F.RT_KIND_MEDIUM:
            return 1 + need(d.media[idx].boundary)
        return 1
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 10000))
    try:
        return need(d.root)
    finally:
        sys.setrecursionlimit(old)


def mega_refuses(d):
    """Validator::check_pools: the megakernel engine takes a medium whose boundary is one primitive under movers, nothing else."""
    for i in range(d.n_media):
        ref = d.media[i].boundary
        while F.RT_KIND_TRANSLATE <= F.ref_kind(ref) <= F.RT_KIND_ZOOM:
            ref = d.xforms[F.ref_index(ref)].child
        if not F.RT_KIND_SPHERE <= F.ref_kind(ref) <= F.RT_KIND_RING:
            return True
    return False


def expected_variant(d, need, tuning=TUNING):
    """choose_trace and trace_variant (pt_wavefront_trace.hip) for a timed render under the tuning word: what
    DeviceScene.trace_variant() must report, and `table` — plain, whole, partial or prims — for the reader."""
    feat = feature_word(d)
    spheres = feat == 0 and d.n_rects == 0
    mesh_f32 = bool(feat & 1) and not feat & 4                    # f32_hbm: single-precision node records in the plain kernels
    table = "plain"
    if not tuning & NO_TABLE and need <= STACK_TINY:
        if spheres and d.n_nodes <= PRIM_NODES and d.n_spheres <= PRIM_SPHERES and d.n_moving_spheres <= PRIM_MOVING:
            table = "prims"
        elif d.n_nodes <= NODE_CACHE:
            table = "whole"
        elif not (spheres or mesh_f32):
            table = "partial"
    if table == "plain":
        stack = STACK_SMALL if need <= STACK_SMALL else STACK_MID if need <= STACK_MID else STACK_LARGE
        f32 = spheres or mesh_f32
    else:
        stack = STACK_TINY
        f32 = table == "prims" or (spheres and table == "whole")
    return {"table": table, "workgroup_threads": 256 if table == "plain" else 1024, "stack_entries": stack,
            "nodes_in_lds": 0 if table == "plain" else min(d.n_nodes, NODE_CACHE), "spheres_in_lds": table == "prims",
            "f32_slabs": bool(f32)}


def promised_kinds(feat, sphere_only=False):
    """The indices of rt_stats.prim_tests a case's rays must reach; every other one (but 0: nodes count as node_visits) stays 0."""
    kinds = set(SPHERE_KINDS if sphere_only else BASE_KINDS)
    for bit, ks in BIT_KINDS.items():
        if feat & bit:
            kinds.update(ks)
    return kinds


# ---- the scenes ------------------------------------------------------------------------------------------------------
def _box(c, r):
    return tuple(x - r - EPS for x in c), tuple(x + r + EPS for x in c)


def _leaves(b, feat, g, sphere_only):
    """The objects of a case [(ref, lo, hi)]: the base, and what each bit of `feat` promises — nothing else."""
    lam = [b.lambertian(tuple(g.uniform(0.3, 0.9, 3))) for _ in range(3)]
    metal, glass = b.metal((0.8, 0.7, 0.6), 0.1), b.dielectric(1.5)
    out = []

    def sphere(c, r, m):
        out.append((b.sphere(c, r, m), *_box(c, r)))

    jit = lambda: float(g.uniform(-0.05, 0.05))
    sphere((-3.2 + jit(), 0.3, 0.5), 0.8, lam[0])
    sphere((3.2 + jit(), 0.3, 0.5), 0.8, metal)
    sphere((0.0, 0.6 + jit(), -3.0), 1.1, glass)
    out.append((b.moving_sphere((-1.5, 2.5, -2.0), (-1.5, 3.0 + jit(), -2.0), 0.0, 1.0, 0.4, lam[1]), (-1.9 - EPS, 2.1 - EPS, -2.4 - EPS), (-1.1 + EPS, 3.5, -1.6 + EPS)))
    if sphere_only:
        sphere((0.0, -100.5, 0.0), 100.0, lam[2])                                             # the ground, as a sphere
    else:
        out.append((b.rect(F.RT_RECT_XZ, -12, 12, -12, 12, -0.5, lam[2]), (-12, -0.5 - EPS, -12), (12, -0.5 + EPS, 12)))
        lamp = b.rect(F.RT_RECT_XZ, -2, 2, -3, 1, 7.0, b.diffuse_light((9, 9, 8)), flip=True)
        out.append((lamp, (-2, 7.0 - EPS, -3), (2, 7.0 + EPS, 1)))
        b.light(F.make_ref(F.RT_KIND_RECT, F.ref_index(lamp)))                                # (the light list holds the plain rect, as scene.rs does)
    if feat & 1:
        for a, bb, c in (((-2.0, -0.4, 2.5), (-0.5, -0.4, 2.5), (-1.2, 1.0 + jit(), 2.0)), ((0.8, -0.3, 2.8), (2.2, -0.3, 2.4), (1.5, 0.9, 2.2 + jit()))):
            pts = np.array([a, bb, c])
            out.append((b.triangle(a, bb, c, lam[0] if a[0] < 0 else metal), tuple(pts.min(0) - EPS), tuple(pts.max(0) + EPS)))
        out.append((b.ring(1.3, 0.35, lam[1]), (-1.65 - EPS, -EPS, -1.65 - EPS), (1.65 + EPS, EPS, 1.65 + EPS)))   # in y = 0 round the origin
    if feat & 2:
        # a RotateY nested in a Translate: leaving the inner mover restarts from the Translate's frame, not from the world ray
        inner = b.rotate_y(b.sphere((0.4, 0.5, 0.0), 0.5, lam[0]), 0.5, 0.8660254037844386)
        out.append((b.translate(inner, (-4.5, 0.0 + jit(), -2.5)), (-5.4 - EPS, -0.05 - EPS, -3.4 - EPS), (-3.6 + EPS, 1.05 + EPS, -1.6 + EPS)))
        out.append((b.zoom(b.sphere((2.2, 1.2, -1.0), 0.3, metal), 2.0), *_box((4.4, 2.4, -2.0), 0.6)))
        out.append((b.rotate_y(b.sphere((1.5, 2.2, -1.0), 0.4, lam[2]), 0.6, 0.8), (-2.3, 1.8 - EPS, -2.3), (2.3, 2.6 + EPS, 2.3)))
        out.append((b.list([b.sphere((-2.0, 2.6, 0.5), 0.35, glass), b.sphere((2.0, 2.8 + jit(), 0.5), 0.35, lam[1])]), (-2.35 - EPS, 2.25 - EPS, 0.15 - EPS), (2.35 + EPS, 3.2 + EPS, 0.85 + EPS)))
    if feat & 4:
        p0, p1 = (-1.6, -0.5, -1.9), (-0.6, 0.9 + jit(), -1.1)
        out.append((b.box(p0, p1, lam[1]), tuple(x - EPS for x in p0), tuple(x + EPS for x in p1)))
        fog = b.isotropic((0.8, 0.8, 0.9))
        if feat & 2:                                      # the boundary under movers: one primitive, so the megakernel takes the scene too
            shell = b.translate(b.rotate_y(b.box((-0.5, 0.0, -0.5), (0.5, 1.2, 0.5), glass), 0.5, 0.8660254037844386), (1.6, -0.4, 2.0))
            out.append((b.medium(shell, 1.5, fog), (0.8, -0.4 - EPS, 1.2), (2.4, 0.8 + EPS, 2.8)))
        else:
            out.append((b.medium(b.sphere((1.6, 0.4, 2.0), 0.7, glass), 1.5, fog), *_box((1.6, 0.4, 2.0), 0.7)))
    return out


def make_scene(feat, shape, seed, sphere_only=False):
    """(desc, cam, params, rows) of the case. The desc keeps its builder alive; `shape` small is the `whole` scene (the caller
    sets tuning bit 28)."""
    assert 0 <= feat <= 7 and shape in SHAPES and not (sphere_only and feat)
    g = np.random.default_rng(1000 * seed + 8 * SHAPES.index(shape) + feat)
    b = rt.DescBuilder()
    leaves = _leaves(b, feat, g, sphere_only)
    if shape == "partial":
        mats = [b.lambertian((0.6, 0.6, 0.7)), b.metal((0.9, 0.8, 0.7), 0.0), b.dielectric(1.5)]
        for i in range(900):                              # a cloud of small spheres behind the objects
            c = tuple(g.uniform((-6.0, 0.0, -9.0), (6.0, 5.0, -5.0)))
            r = float(g.uniform(0.05, 0.12))
            leaves.append((b.sphere(c, r, mats[i % 3]), *_box(c, r)))
    root = median_split_bvh(b, leaves)
    if shape in ("mid", "large"):
        b.set_root(root)
        links = (MID_NEED if shape == "mid" else LARGE_NEED) - stack_need(b.desc())
        lam = b.lambertian((0.7, 0.4, 0.3))

        def right_child(i):                               # a row of small objects across the top of the view
            c = (-5.0 + 10.0 * i / max(links - 1, 1), 4.6 + 0.4 * (i % 2), -3.0)
            if feat & 4:
                return b.box(tuple(x - 0.15 for x in c), tuple(x + 0.15 for x in c), lam)
            return b.sphere(c, 0.18, lam)
        root = chain(b, root, links, right_child)
    b.set_root(root)
    d = b.desc()
    d._builder = b                                        # (the pools live in the builder)
    cam = rt.camera_new((0.0, 3.0, 11.0), (0.0, 1.2, -1.0), (0, 1, 0), 42.0, W / H, 0.0, 10.0, 0.0, 1.0)
    bg = (0.6, 0.7, 0.9) if sphere_only else (0.08, 0.1, 0.16)
    p = rt.make_params(W, H, SPP, MAX_DEPTH, bg, seed=seed)
    return d, cam, p, rt.shuffled_rows(H, seed)


def matrix_cases():
    """(feat, shape, sphere_only) of every case of the instance matrix."""
    return [(f, s, False) for f in range(8) for s in SHAPES] + [(0, "whole", True), (0, "large", True)]


def case_id(case):
    return "%s%d-%s" % ("spheres" if case[2] else "feat", case[0], case[1])


# ---- the scene whose movers, media and lights outgrow the kernels' small LDS tables ----------------------------------------
OVERFLOW_VIEW = (40, 30, 4)


def overflow_scene(seed=7, mid=False):
    """FEAT 7 under a HittableList root: 12 movers (two of them hold a RotateY of their own; with the Translates of a medium's
    boundary and of the ring, 16 mover records), 5 media, 12 lights. The kernels keep the first 8 mover records, 2 medium records
    and 8 light records in LDS (wf_trace: kLdsXforms, kLdsMedia; wf_shade: kLdsLights) and read the others from global memory.
    rt_scene_create uploads the three pools in the order of the desc — the order of creation here — so mover records 8..15 (the
    movers 7 to 11, in the top row of the view), media 2..4 and lights 8..11 are the ones behind the tables.
    mid: the same under a chain of nodes, cut to a stack need of MID_NEED — the 30-entry kernels, which keep no world ray in LDS.
    → (desc, cam, params, rows, mats): mats = {"movers": [...], "media": [...]} the material index that tells each one's hits."""
    b = rt.DescBuilder()
    g = np.random.default_rng(seed)
    cells = [(x, y) for y in (0.5, 2.4, 4.3) for x in (-5.0, -3.0, -1.0, 1.0, 3.0, 5.0)]
    leaves, mover_mats, medium_mats = [], [], []
    s30, c30 = 0.5, 0.8660254037844386

    def own_mat():
        return b.lambertian(tuple(g.uniform(0.2, 0.9, 3)))

    # 12 movers of the three kinds with parameters of their own; numbers 3 and 9 hold a RotateY of their own
    for i in range(12):
        x, y = cells[i]
        m = own_mat()
        mover_mats.append(m)
        kind = i % 3
        if kind == 0:                                     # Translate (of a RotateY for two of them)
            prim = b.box((-0.45, -0.45, -0.45), (0.45, 0.45 + 0.02 * i, 0.45), m) if i % 2 else b.sphere((0.1, 0.0, 0.0), 0.5, m)
            if i in (3, 9):
                prim = b.rotate_y(prim, s30, c30) if i == 3 else b.rotate_y(prim, 0.6, 0.8)
            ref = b.translate(prim, (x, y + 0.01 * i, 0.0))
            r = 0.9
        elif kind == 1:                                   # RotateY by an angle of its own: the object on the circle through (x, 0)
            th = 0.1 + 0.07 * i
            s, c = float(np.sin(th)), float(np.cos(th))
            # the child's point q with q.x = c x' - s z', q.z = s x' + c z' for the world point (x', z') = (x, 0)
            ref = b.rotate_y(b.sphere((c * x, y, s * x), 0.5 + 0.01 * i, m), s, c)
            r = 0.7
        else:                                             # Zoom by a rate of its own
            rate = 1.2 + 0.1 * i
            ref = b.zoom(b.sphere((x / rate, y / rate, 0.0), 0.55 / rate, m), rate)
            r = 0.6
        leaves.append((ref, (x - r, y - r, -r), (x + r, y + r, r)))
    # 5 media of distinct density and colour: sphere boundaries (the record carries the sphere inline), a box, a box under a mover
    glass = b.dielectric(1.5)
    for j in range(5):
        x, y = cells[12 + j]
        iso = b.isotropic(tuple(g.uniform(0.2, 0.9, 3)))
        medium_mats.append(iso)
        if j in (0, 2, 4):
            shell = b.sphere((x, y, 0.0), 0.6, glass)
        elif j == 1:
            shell = b.box((x - 0.5, y - 0.5, -0.5), (x + 0.5, y + 0.5, 0.5), glass)
        else:
            shell = b.translate(b.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), glass), (x, y, 0.0))
        leaves.append((b.medium(shell, 3.0 + 1.5 * j, iso), (x - 0.7, y - 0.7, -0.7), (x + 0.7, y + 0.7, 0.7)))
    # 12 small lights of distinct emission in front of the objects, facing them and the walls: spheres and rects, every one in the light list
    for k in range(12):
        x = -5.5 + k
        em = b.diffuse_light(tuple(g.uniform(4.0, 14.0, 3)))
        if k % 2:
            ref = b.sphere((x, 5.9, 1.5), 0.2 + 0.01 * k, em)
            leaves.append((ref, *_box((x, 5.9, 1.5), 0.2 + 0.01 * k)))
            b.light(ref)
        else:
            ref = b.rect(F.RT_RECT_XZ, x - 0.25, x + 0.25, 1.2, 1.8 + 0.02 * k, 6.2, em, flip=True)
            leaves.append((ref, (x - 0.25, 6.2 - EPS, 1.2), (x + 0.25, 6.2 + EPS, 1.8 + 0.02 * k)))
            b.light(F.make_ref(F.RT_KIND_RECT, F.ref_index(ref)))
    # a triangle and a ring (FEAT bit 1), a floor and a back wall to scatter from
    wall = b.lambertian((0.7, 0.7, 0.7))
    leaves.append((b.triangle((5.6, 3.6, 0.0), (6.4, 3.6, 0.0), (6.0, 4.9, 0.3), own_mat()), (5.6 - EPS, 3.6 - EPS, -EPS), (6.4 + EPS, 4.9 + EPS, 0.3 + EPS)))
    leaves.append((b.translate(b.ring(0.5, 0.2, own_mat()), (6.0, 0.2, 1.0)), (5.2, 0.2 - EPS, 0.2), (6.8, 0.2 + EPS, 1.8)))
    floor_ = b.rect(F.RT_RECT_XZ, -12, 12, -6, 12, -0.4, wall)
    back = b.rect(F.RT_RECT_XY, -12, 12, -1, 9, -2.5, wall)
    bvh = median_split_bvh(b, leaves)
    root = b.list([floor_, back, bvh])
    if mid:
        b.set_root(root)
        lam = b.lambertian((0.5, 0.6, 0.4))
        root = chain(b, root, MID_NEED - stack_need(b.desc()), lambda i: b.box((-6.0 + 0.3 * i, 6.6, 0.0), (-5.8 + 0.3 * i, 6.8, 0.2), lam))
    b.set_root(root)
    d = b.desc()
    d._builder = b
    Wv, Hv, spp = OVERFLOW_VIEW
    cam = rt.camera_new((0.0, 2.6, 14.0), (0.0, 2.6, 0.0), (0, 1, 0), 36.0, Wv / Hv, 0.0, 14.0, 0.0, 1.0)
    p = rt.make_params(Wv, Hv, spp, MAX_DEPTH, (0.02, 0.02, 0.03), seed=seed)
    return d, cam, p, rt.shuffled_rows(Hv, seed), {"movers": mover_mats, "media": medium_mats}


def pinhole_rays(cam, width, height):
    """The ray through the middle of every pixel (origin, direction arrays): Camera::get_ray without the lens."""
    px, py = np.meshgrid(np.arange(width), np.arange(height))
    s, t = (px.ravel() + 0.5) / (width - 1), (py.ravel() + 0.5) / (height - 1)
    o = np.array(cam.origin[:])
    d = np.array(cam.lower_left_corner[:]) + s[:, None] * np.array(cam.horizontal[:]) + t[:, None] * np.array(cam.vertical[:]) - o
    return np.broadcast_to(o, d.shape).copy(), d


# ---- pairs of scenes one node, one sphere or one stack entry apart -------------------------------------------------------
def _view(d, b, seed, background):
    d._builder = b
    cam = rt.camera_new((0.0, 1.0, 10.0), (0.0, 0.5, -6.0), (0, 1, 0), 42.0, W / H, 0.0, 10.0, 0.0, 1.0)
    return d, cam, rt.make_params(W, H, 3, MAX_DEPTH, background, seed=seed), rt.shuffled_rows(H, seed)


def _cloud(b, g, n, moving=0):
    """n small spheres (the last `moving` of them MovingSpheres) in the view's depth."""
    mats = [b.lambertian((0.6, 0.6, 0.7)), b.metal((0.9, 0.8, 0.7), 0.0), b.dielectric(1.5)]
    leaves = []
    for i in range(n):
        c = tuple(g.uniform((-5.0, -2.5, -9.0), (5.0, 3.5, -3.0)))
        r = float(g.uniform(0.12, 0.3))
        if i >= n - moving:
            c1 = (c[0], c[1] + 0.3, c[2])
            leaves.append((b.moving_sphere(c, c1, 0.0, 1.0, r, mats[i % 3]), tuple(x - r - EPS for x in c), tuple(x + r + EPS for x in c1)))
        else:
            leaves.append((b.sphere(c, r, mats[i % 3]), *_box(c, r)))
    return leaves


def node_count_scene(n_nodes, seed=3):
    """Spheres and two rects (FEAT 0, not sphere-only) in a BVH of exactly n_nodes nodes: span-1 leaves make 2 n - 1; an even
    count takes one more node over the root whose right child is a sphere."""
    b = rt.DescBuilder()
    g = np.random.default_rng(seed)
    n_leaves = (n_nodes + 1) // 2 if n_nodes & 1 else n_nodes // 2
    leaves = _cloud(b, g, n_leaves - 2)
    lam = b.lambertian((0.6, 0.6, 0.6))
    leaves.append((b.rect(F.RT_RECT_XZ, -12, 12, -14, 4, -3.0, lam), (-12, -3.0 - EPS, -14), (12, -3.0 + EPS, 4)))
    lamp = b.rect(F.RT_RECT_XZ, -2, 2, -8, -4, 7.0, b.diffuse_light((9, 9, 9)), flip=True)
    leaves.append((lamp, (-2, 7.0 - EPS, -8), (2, 7.0 + EPS, -4)))
    b.light(F.make_ref(F.RT_KIND_RECT, 1))
    root = median_split_bvh(b, leaves)
    if not n_nodes & 1:
        root = b.node(WORLD[0], WORLD[1], root, b.sphere((0.0, 3.0, -4.0), 0.4, lam))
    b.set_root(root)
    d = b.desc()
    assert d.n_nodes == n_nodes
    return _view(d, b, seed, (0.1, 0.12, 0.2))


def sphere_count_scene(n_spheres=0, n_moving=0, n_nodes=None, seed=4):
    """A sphere-only scene of so many Spheres and MovingSpheres; two primitives per lowest node keep the node count under the
    all-in-LDS instance's 600 where the pools are at their own limits. n_nodes: exactly so many nodes instead, span-1 leaves (an
    even count as in node_count_scene)."""
    b = rt.DescBuilder()
    g = np.random.default_rng(seed)
    if n_nodes is None:
        root = paired_leaf_bvh(b, _cloud(b, g, n_spheres + n_moving, moving=n_moving))
    else:
        n_leaves = (n_nodes + 1) // 2 if n_nodes & 1 else n_nodes // 2
        n_moving = n_leaves // 3
        root = median_split_bvh(b, _cloud(b, g, n_leaves, moving=n_moving))
        if not n_nodes & 1:
            root = b.node(WORLD[0], WORLD[1], root, b.sphere((0.0, 3.0, -4.0), 0.4, b.lambertian((0.5, 0.5, 0.5))))
    b.set_root(root)
    d = b.desc()
    assert n_nodes is None or d.n_nodes == n_nodes
    return _view(d, b, seed, (0.6, 0.7, 0.9))


def stack_need_scene(need, seed=5):
    """A sphere-only scene whose traversal needs about `need` stack entries: a chain of need - 1 links over one sphere. (The
    test reads the need back from the library.)"""
    b = rt.DescBuilder()
    lam, metal = b.lambertian((0.6, 0.6, 0.7)), b.metal((0.8, 0.8, 0.9), 0.05)
    links = need - 1
    root = chain(b, b.sphere((0.0, -50.0, -20.0), 48.0, lam), links,
                 lambda i: b.sphere((-5.0 + 10.0 * i / max(links - 1, 1), 0.5 + 0.9 * (i % 4), -6.0 - 0.05 * i), 0.4, metal if i % 2 else lam))
    b.set_root(root)
    return _view(b.desc(), b, seed, (0.6, 0.7, 0.9))
