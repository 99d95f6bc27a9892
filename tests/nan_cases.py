"""Scenes and rays on which a hit distance is NaN or infinite, one scene per traversal-kernel family (wf_trace:
pt_wavefront_trace.hip, choose_trace). No test in here, no GPU needed: tests/test_nan_cases.py holds the oracle alone to the
conditions that keep a case from being vacuous, tests/test_nan_cases_gpu.py runs every case on the device.

Every comparison of a hit function, and what a NaN does to it (a comparison with a NaN is false):

  comparison                                csrc/hip/pt_common.hpp   oracle/rt_oracle.cpp   reference                       a NaN
  sphere   discriminant < 0 -> miss         :204                     :184                   sphere.rs:46, :145              passes on
  sphere   root < t_min || t_max < root     :207, :209               :187, :189             sphere.rs:52-54, :151-153       ACCEPTS: a NaN root,
                                                                                                                            and any root >= t_min under a NaN t_max
  rect     tt < t_min || tt > t_max         :228                     :217                   aarect.rs:48, :131, :214        ACCEPTS, likewise
  rect     a < a0 || a > a1 || b < ...      :231                     :220                   aarect.rs:54, :137, :220        ACCEPTS a NaN point
  box      six rects, closest-so-far        :245-256                 :245-255               boxes.rs:80-82, mod.rs:90-100   as rect, face by face
  triangle tt != tt || tt < ... || tt > ... :263                     :268                   triangle.rs:57                  REFUSES a NaN tt; accepts
                                                                                                                            a tt in the window under a NaN t_max
  triangle the three edge tests >= 0        :265-267                 :259-261               triangle.rs:33-46               REFUSES a NaN point
  ring     tt != tt || tt < ... || tt > ... :275                     :284                   ring.rs:38                      REFUSES a NaN tt
  ring     d < dis_min || d > dis_max       :278                     :287                   ring.rs:45                      accepts a NaN point
  medium   rec1.t >= rec2.t -> miss         pt_wavefront_trace.hip   :301                   constantmedium.rs:54            passes on
  medium   hit_distance > distance -> miss  (the medium arm)         :307                   constantmedium.rs:62            ACCEPTS
  node     t0 > t_min, t1 < t_max           (the literal node step)  :146-147               aabb.rs:25-26                   keeps the old end: a NaN
                                                                                                                            slab distance is skipped, a NaN t_max stays
  node     t_max <= t_min -> miss           (the literal node step)  :148                   aabb.rs:27                      ENTERS: a NaN t_max culls nothing
  node     right child against recl.t       (the traversal stack)    :160                   bvh/mod.rs:86-101               the NaN is handed on
  list     closest_so_far = rec.t           (the list arm)           :360                   mod.rs:92-95                    the NaN is handed on

So once the closest hit is NaN every sphere and rect that is visited accepts, and the leaf visited LAST wins: the answer depends
on the order of the visits, which the timed kernels may change, and on the nodes a NaN window end culls.

A case is (family, variant): `family` names the wf_trace instance the scene selects, `variant` what is put into it:
  base   the leaves alone: ray families a (NaN, infinite and zero components), b (in-plane axis-parallel rays: 0 / 0 on a rect,
         on a box face) and f (ordinary rays, the control)
  far    + one sphere centred 1e200 away, reached through the root's left child: every ray's half_b^2 - a c is inf - inf there.
         Ray family c, ordinary rays
  huge   + two spheres of radius 1e160 (r^2 = inf: the accepted root is +inf), reached likewise. One such sphere alone wins or
         loses whatever the order; two of them tie at t = inf, where the last one visited wins. Ray family c
  wide   every node box +-1.7e308. Ray family d, an origin coordinate of +-1e308: against a box of ordinary size both slab
         distances of that axis round to the same number and the root is missed; against these the ray reaches every leaf
  still  every sphere a MovingSphere with time0 == time1 (rt_scene_create accepts that): a NaN centre from 0 / 0, or from
         0 * inf where the ray's time differs. Ray family e. Sphere and FEAT 0 families only
  turned + two YZ rects in the plane x' = 0 of a RotateY whose sine and cosine are the same double. Ray family g: o.x == o.z and
         d.x == d.z, every component ordinary and non-zero — the world ray is a plain one, visited in the device's own order;
         inside the mover d'.x = c d.x - s d.z = 0 and o'.x = 0: 0 / 0 on both rects. Mover families only
Family b needs a rect or a box face, which the two sphere-only families do not have: they run a, c, d, e and f.

Every leaf is a DiffuseLight of a colour of its own under a FlipFace bit and sits in a span-1 node of its own (one medium of
the FEAT 4, 6, 7 scenes apart): a NaN ray has front_face = false, the flip makes the winner emit, so the radiance at depth 1
names the winner; the flipped refs keep their nodes unordered (scene_check.cpp: centre2) and the inner nodes over them ordered.
rto_hit reports no primitive: the winner's own material stands for it.

Cases are pure functions of a seed: same seed, same bytes (case_bytes)."""
import ctypes as C

import numpy as np

import raytracer_2022_amd as rt
from raytracer_2022_amd import _ffi as F

import trace_scenes as T

R = 3.0                                                   # the leaves lie in [-R, R]^3
K0 = 0.5                                                  # the plane y = K0 holds three rects and the boxes' bottom faces
K_XY, K_YZ = -1.0, 1.0                                    # ... z = K_XY one XY rect, x = K_YZ one YZ rect
EPS = 1e-4
BIG = 1.7e308
FAR, HUGE = 1e200, 1e160
MAX_LEAVES, MAX_RAYS = 64, 512

# family → (feature word, sphere-only, tuning, chain, (table, f32 slabs, stack entries, ordered))
FAMILIES = {
    "prims":         (0, True, T.TUNING, None, ("prims", True, 16, True)),
    "spheres-plain": (0, True, T.TUNING | T.NO_TABLE, None, ("plain", True, 22, True)),
    "feat0-whole":   (0, False, T.TUNING, None, ("whole", False, 16, True)),
    "feat0-plain":   (0, False, T.TUNING | T.NO_TABLE, None, ("plain", False, 22, True)),
    "feat1-mesh":    (1, False, T.TUNING | T.NO_TABLE, None, ("plain", True, 22, True)),
    "feat2-movers":  (2, False, T.TUNING, None, ("whole", False, 16, True)),
    "feat4-volumes": (4, False, T.TUNING, None, ("whole", False, 16, True)),
    "feat6":         (6, False, T.TUNING, None, ("whole", False, 16, True)),
    "feat7-control": (7, False, T.TUNING, None, ("whole", False, 16, False)),
    "mid-chain":     (0, False, T.TUNING, T.MID_NEED, ("plain", False, 30, True)),
    "large-chain":   (0, False, T.TUNING, T.LARGE_NEED, ("plain", False, 64, True)),
}
VARIANTS = {"base": ("a", "b", "f"), "far": ("c",), "huge": ("c",), "wide": ("d",), "still": ("e",), "turned": ("g",)}
STILL_FAMILIES = ("prims", "spheres-plain", "feat0-whole", "feat0-plain")
TURNED_FAMILIES = ("feat2-movers", "feat6")
S45 = 0.7071067811865476                                  # the sine and the cosine of the turned rects' RotateY: the same double


def all_cases():
    return [(f, v) for f in FAMILIES for v in VARIANTS if (v != "still" or f in STILL_FAMILIES) and (v != "turned" or f in TURNED_FAMILIES)]


def case_id(c):
    return "%s-%s" % c


def ray_families(family, variant):
    return tuple(x for x in VARIANTS[variant] if not (x == "b" and FAMILIES[family][1]))


# ---- the scenes --------------------------------------------------------------------------------------------------------------
def _sphere_box(c, r):
    return tuple(x - r - EPS for x in c), tuple(x + r + EPS for x in c)


def _leaves(b, g, feat, sphere_only, still, n_spheres, turned=False):
    """[(ref, lo, hi)]: flipped lights of a colour each; boxes worked out here (a still MovingSphere has no box of its own)."""
    out = []

    def light():
        return b.diffuse_light(tuple(float(x) for x in g.uniform(0.5, 8.0, 3)))

    def ball(c, r, moving):
        if moving or still:
            c1 = (c[0], c[1] + 0.3, c[2])
            t0, t1 = (0.5, 0.5) if still else (0.0, 1.0)
            lo, hi = _sphere_box(c, r)
            out.append((b.moving_sphere(c, c1, t0, t1, r, light(), flip=True), lo, (hi[0], hi[1] + 0.3, hi[2])))
        else:
            out.append((b.sphere(c, r, light(), flip=True), *_sphere_box(c, r)))

    for i in range(n_spheres):                            # (clear of the plane y = K0: an in-plane ray keeps the NaN it finds there)
        r = float(g.uniform(0.45, 0.9))
        x, z = (float(v) for v in g.uniform(-R, R, 2))
        y = float(g.uniform(K0 + r + 0.05, R + 0.4)) if i % 2 else float(g.uniform(-R, K0 - r - 0.4))
        ball((x, y, z), r, moving=i % 4 == 3)
    if not sphere_only:
        for i in range(3):                                # three rects side by side in the plane y = K0, z < 0 (apart: no ordinary ray ties)
            x0, z0 = -R + 2.0 * i + float(g.uniform(0.05, 0.2)), float(g.uniform(-R, -2.0))
            x1, z1 = x0 + float(g.uniform(1.5, 1.75)), float(g.uniform(-1.0, -0.2))
            out.append((b.rect(F.RT_RECT_XZ, x0, x1, z0, z1, K0, light(), flip=True), (x0, K0 - EPS, z0), (x1, K0 + EPS, z1)))
        out.append((b.rect(F.RT_RECT_XY, -2.0, 1.5, -1.5, 2.0, K_XY, light(), flip=True), (-2.0, -1.5, K_XY - EPS), (1.5, 2.0, K_XY + EPS)))
        out.append((b.rect(F.RT_RECT_YZ, -1.0, 2.5, -2.0, 1.0, K_YZ, light(), flip=True), (K_YZ - EPS, -1.0, -2.0), (K_YZ + EPS, 2.5, 1.0)))
    if feat & 1:                                          # a small mesh: a fan of six triangles round an apex
        apex = (0.3, 2.2, 0.4)
        rim = [(0.3 + 1.6 * float(np.cos(a)), 1.2 + 0.2 * (j % 2), 0.4 + 1.6 * float(np.sin(a))) for j, a in enumerate(np.arange(6) * np.pi / 3)]
        for j in range(6):
            pts = np.array([apex, rim[j], rim[(j + 1) % 6]])
            out.append((b.triangle(apex, rim[j], rim[(j + 1) % 6], light(), flip=True), tuple(pts.min(0) - EPS), tuple(pts.max(0) + EPS)))
    if feat & 2:                                          # one sphere under each mover; the flip on the mover's own ref
        s30, c30 = 0.5, 0.8660254037844386
        out.append((b.translate(b.sphere((0.0, 0.0, 0.0), 0.8, light()), (-1.5, 1.0, 1.5), flip=True), *_sphere_box((-1.5, 1.0, 1.5), 0.8)))
        cx, cz = 1.2, -0.8                                # RotateY: the child's centre (cx, cz) shows at (c cx + s cz, -s cx + c cz)
        out.append((b.rotate_y(b.sphere((cx, -1.0, cz), 0.7, light()), s30, c30, flip=True),
                    *_sphere_box((c30 * cx + s30 * cz, -1.0, -s30 * cx + c30 * cz), 0.7)))
        # (a Zoom leaves t in the child's units: at a rate below 1 they are larger than the world's, which the node boxes are in,
        # and the winner does not depend on the order of the visits; at a rate above 1 it does, for ordinary rays too)
        out.append((b.zoom(b.sphere((3.2, 1.6, -4.0), 1.6, light()), 0.5, flip=True), *_sphere_box((1.6, 0.8, -2.0), 0.8)))
        out.append((b.translate(b.rect(F.RT_RECT_XZ, -1.0, 1.0, -1.0, 1.0, 0.0, light()), (0.5, K0 + 1.0, 0.5), flip=True),
                    (-0.5, K0 + 1.0 - EPS, -0.5), (1.5, K0 + 1.0 + EPS, 1.5)))
    if turned:                                            # child (0, y, z') shows at (s z', y, c z'): the plane x = z of the world
        for (z0, z1, y0, y1) in ((-4.0, 0.5, -2.5, 1.0), (-0.5, 4.0, -1.0, 2.5)):
            r = b.rotate_y(b.rect(F.RT_RECT_YZ, y0, y1, z0, z1, 0.0, light()), S45, S45, flip=True)
            out.append((r, (S45 * z0 - EPS, y0, S45 * z0 - EPS), (S45 * z1 + EPS, y1, S45 * z1 + EPS)))
    if feat & 4:
        for i in range(3):                                # three boxes side by side standing on the plane y = K0, z > 0
            x0, z0 = -R + 2.0 * i + float(g.uniform(0.05, 0.2)), float(g.uniform(0.2, 0.6))
            p0, p1 = (x0, K0, z0), (x0 + float(g.uniform(1.5, 1.75)), K0 + float(g.uniform(0.3, 0.6)), z0 + float(g.uniform(1.5, 2.2)))
            out.append((b.box(p0, p1, light(), flip=True), tuple(x - EPS for x in p0), tuple(x + EPS for x in p1)))
        c = (1.8, -1.6, 1.4)                              # one Isotropic medium, a sphere boundary, no FlipFace
        out.append((b.medium(b.sphere(c, 0.9, b.dielectric(1.5)), 1.2, b.isotropic((0.8, 0.8, 0.9))), *_sphere_box(c, 0.9)))
    return out


def _union(boxes):
    return (tuple(min(bx[0][k] for bx in boxes) for k in range(3)), tuple(max(bx[1][k] for bx in boxes) for k in range(3)))


class Case:
    """family, variant, desc (its builder kept alive), tuning, expect = (table, f32 slabs, stack entries, ordered), base_root
    (the ref of the BVH over the ordinary leaves), rays {ray family: RADIANCE_RAY_DTYPE records}, feat."""


def make_case(family, variant, seed=1):
    feat, sphere_only, tuning, need, expect = FAMILIES[family]
    assert variant in VARIANTS and (variant != "still" or family in STILL_FAMILIES)
    # (one stream per scene — the two sphere-only families and the two FEAT 0 ones share theirs — and one per ray family)
    scene_key = [feat, int(sphere_only), need or 0]
    g = np.random.default_rng([seed, 1] + scene_key)
    b = rt.DescBuilder()
    n_spheres = 20 if sphere_only else 9 if need else 12
    assert variant != "turned" or family in TURNED_FAMILIES
    leaves = _leaves(b, g, feat, sphere_only, variant == "still", n_spheres, variant == "turned")
    root = base_root = T.median_split_bvh(b, leaves)
    if variant == "far":
        a = b.sphere((FAR, 0.0, 0.0), 1.0, b.diffuse_light((3.0, 0.25, 7.0)), flip=True)
        box = ((-1e3, -1e3, -1e3), (10.0 * FAR, 1e3, 1e3))
        root = b.node(*box, b.node(*box, a, a), root)
    elif variant == "huge":
        a1 = b.sphere((0.0, 0.0, 0.0), HUGE, b.diffuse_light((3.0, 0.25, 7.0)), flip=True)
        a2 = b.sphere((1.0, 0.0, 0.0), HUGE, b.diffuse_light((0.25, 6.0, 2.0)), flip=True)
        box1, box2 = ((-1e3, -1e3, -1e3), (1e3, 1e3, 1e3)), ((-900.0, -1e3, -1e3), (1100.0, 1e3, 1e3))
        both = _union([box1, box2])
        root = b.node(*both, b.node(*both, b.node(*box1, a1, a1), b.node(*box2, a2, a2)), root)
    if need:
        b.set_root(root)
        links = need - T.stack_need(b.desc())
        lamps = [b.diffuse_light(tuple(float(x) for x in g.uniform(0.5, 8.0, 3))) for _ in range(links)]
        root = T.chain(b, root, links, lambda i: b.sphere((-R + 2.0 * R * i / max(links - 1, 1), 2.6 + 0.3 * (i % 2), -2.0), 0.25, lamps[i], flip=True))
    if variant == "wide":                                 # (each box a little shorter than the one before: the centres differ, the nodes keep an order)
        for i, n in enumerate(b.pools["nodes"]):
            n.bmin[:] = [-BIG] * 3
            n.bmax[:] = [BIG - 1e300 * (i + 1) * (1 + (i + k) % 3) for k in range(3)]
    b.set_root(root)
    c = Case()
    c.family, c.variant, c.tuning, c.expect, c.base_root, c.feat = family, variant, tuning, expect, base_root, feat
    c.desc = b.desc()
    c.desc._builder = b
    c.n_leaves = len(leaves) + {"far": 1, "huge": 2}.get(variant, 0) + (links if need else 0)
    c.rays = {}
    for fam in ray_families(family, variant):
        gr = np.random.default_rng([seed, 2, "abcdefg".index(fam)] + scene_key)
        c.rays[fam] = RAY_FAMILIES[fam](gr, bool(feat & 4))
    assert c.n_leaves <= MAX_LEAVES and sum(len(r) for r in c.rays.values()) <= MAX_RAYS
    return c


def mirrored(desc):
    """The same scene with the two children of every inner node exchanged; boxes and leaves as they are."""
    n = desc.n_nodes
    nodes = (F.rt_bvh_node * max(1, n))()
    C.memmove(nodes, desc.nodes, n * C.sizeof(F.rt_bvh_node))
    for i in range(n):
        nodes[i].left, nodes[i].right = nodes[i].right, nodes[i].left
    m = F.rt_scene_desc.from_buffer_copy(desc)
    m.nodes = C.cast(nodes, C.POINTER(F.rt_bvh_node))
    m._builder = (getattr(desc, "_builder", None), nodes)
    return m


def case_bytes(c):
    """Every pool of the desc and every ray, as bytes."""
    out = [C.string_at(getattr(c.desc, name), getattr(c.desc, "n_" + name) * C.sizeof(ctype))
           for name, ctype in rt.DescBuilder.POOLS if getattr(c.desc, "n_" + name)]
    return b"".join(out) + np.uint32(c.desc.root).tobytes() + b"".join(c.rays[k].tobytes() for k in sorted(c.rays))


# ---- the ray families --------------------------------------------------------------------------------------------------------
def _unit(g, n):
    v = g.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rays(g, o, d, time=None):
    n = len(o)
    return rt.radiance_rays(o, d, time=g.random(n) if time is None else time, rng_state=g.integers(0, 2**63, n, dtype=np.uint64))


def family_a(g, has_boxes=False):
    """A NaN in each direction component in turn, +-inf components, the zero direction, a NaN or infinite origin."""
    o, d = [], []
    for k in range(3):                                    # 3 x 44: a NaN direction component
        oo, dd = g.uniform(-R, R, (44, 3)), _unit(g, 44)
        dd[:, k] = np.nan
        o.append(oo); d.append(dd)
    for k in range(3):                                    # 6: an infinite direction component
        for s in (np.inf, -np.inf):
            dd = _unit(g, 1)
            dd[0, k] = s
            o.append(g.uniform(-R, R, (1, 3))); d.append(dd)
    o.append(g.uniform(-R, R, (24, 3))); d.append(np.zeros((24, 3)))            # 24: the zero direction (half of them -0)
    d[-1][::2] = -0.0
    for k in range(3):                                    # 3 x 12: a NaN origin component
        oo = g.uniform(-R, R, (12, 3))
        oo[:, k] = np.nan
        o.append(oo); d.append(_unit(g, 12))
    for k in range(3):                                    # 6: an infinite origin component
        for s in (np.inf, -np.inf):
            oo = g.uniform(-R, R, (1, 3))
            oo[0, k] = s
            o.append(oo); d.append(_unit(g, 1))
    return _rays(g, np.concatenate(o), np.concatenate(d))


def family_b(g, has_boxes=False):
    """In-plane axis-parallel rays: the origin exactly in a rect's plane (for y = K0 the boxes' bottom faces too), that
    direction component +0 or -0: (k - o) / d = 0 / 0."""
    o, d = [], []
    for axis, k, n in ((1, K0, 148), (2, K_XY, 32), (0, K_YZ, 32)):
        oo, dd = g.uniform(-R, R, (n, 3)), _unit(g, n) * g.uniform(0.5, 2.0, (n, 1))
        oo[:, axis] = k
        dd[:, axis] = np.where(np.arange(n) % 2, 0.0, -0.0)
        o.append(oo); d.append(dd)
    return _rays(g, np.concatenate(o), np.concatenate(d))


def _ordinary(g, n, aim):
    """Rays from a shell of radius 7 towards points of [-aim, aim]^3: a good part of them misses every leaf."""
    o = 7.0 * _unit(g, n)
    return o, g.uniform(-aim, aim, (n, 3)) - o


def family_c(g, has_boxes=False):
    return _rays(g, *_ordinary(g, 160, 4.5))


def family_d(g, has_boxes=False):
    """An origin coordinate of +-1e308, every direction component ordinary and non-zero."""
    o, d = g.uniform(-R, R, (96, 3)), _unit(g, 96)
    o[np.arange(96), np.arange(96) % 3] = np.where(np.arange(96) % 2, 1e308, -1e308)
    d = np.where(np.abs(d) < 1e-3, 1e-3, d)
    return _rays(g, o, d)


def family_e(g, has_boxes=False):
    """Ordinary rays; half of them at the time the still MovingSpheres stand at (0 / 0), the others elsewhere (x / 0)."""
    o, d = _ordinary(g, 160, 3.0)
    return _rays(g, o, d, time=np.where(np.arange(160) % 2, 0.5, g.random(160)))


def family_g(g, has_boxes=False):
    """Rays in the plane x = z of the world, towards it from nowhere: o.x == o.z, d.x == d.z, no zero component."""
    o, d = g.uniform(-R, R, (256, 3)), _unit(g, 256)
    d = np.where(np.abs(d) < 1e-3, 1e-3, d)
    o[:, 2], d[:, 2] = o[:, 0], d[:, 0]
    return _rays(g, o, d)


def family_f(g, has_boxes=False):
    return _rays(g, *_ordinary(g, 96, 3.5))


RAY_FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f, "g": family_g}


def query_form(rays):
    """The rays as rt_query_ray records: ray_color's window (0.001, inf)."""
    return rt.query_rays(rays["origin"], rays["direction"], time=rays["time"], rng_state=rays["rng_state"])


# ---- AABB::hit in Python floats (aabb.rs:15-32) ------------------------------------------------------------------------------
def aabb_hit(bmin, bmax, o, d, t_min, t_max):
    for i in range(3):
        inv_d = np.float64(1.0) / np.float64(d[i])
        t0, t1 = (bmin[i] - o[i]) * inv_d, (bmax[i] - o[i]) * inv_d
        if inv_d < 0.0:
            t0, t1 = t1, t0
        t_min = t0 if t0 > t_min else t_min
        t_max = t1 if t1 < t_max else t_max
        if t_max <= t_min:
            return False
    return True


def nodes_below(desc, ref):
    out, stack = [], [ref]
    while stack:
        r = stack.pop()
        if F.ref_kind(r) == F.RT_KIND_NODE:
            n = desc.nodes[F.ref_index(r)]
            out.append(n)
            stack.append(n.left)
            if n.right != n.left:
                stack.append(n.right)
    return out


def slabs_alone_miss(desc, ref, ray, t_min=0.001):
    """Some node below `ref` whose slabs alone — the window's end replaced by inf — say miss."""
    o, d = [float(x) for x in ray["origin"]], [float(x) for x in ray["direction"]]
    with np.errstate(all="ignore"):
        return any(not aabb_hit(list(n.bmin), list(n.bmax), o, d, t_min, np.inf) for n in nodes_below(desc, ref))
