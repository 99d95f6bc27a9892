"""A closest-hit reference that owes nothing to the BVH: every leaf of an rt_scene_desc against every ray, in extended
precision (numpy longdouble, 64-bit mantissa), written as plain geometry and not op for op after hittable/*.rs.

It reads an rt_scene_desc (include/rt2022.h) through dtypes of its own and nothing else of the project. The walker descends
nodes, lists and movers from desc.root and never reads a node's box: a ray culled by a wrong box on the oracle and on the
device alike is still found here. Node boxes are read by two helpers only, node_boxes() for the enclosure check and
flat_node_paths() for the class-1 classifier.

Definitions the reference keeps (they are the reference renderer's):
  translate   the ray's origin minus the offset
  rotate_y    origin and direction through the rotation matrix of the stored (sin, cos)
  zoom        the origin divided by the rate; direction and t untouched, so t is in OBJECT units
  window      t_min <= t <= t_max
  sphere      the nearer root inside the window, else the farther one
  box         the nearest face crossing inside the window (a ray from inside gets the exit)
  triangle    barycentrics with inclusive edges; ring: dis_min <= x^2 + z^2 <= dis_max in the plane y = 0
  medium      not a solid: recorded with its boundary's leaf paths; chord() gives [t_in, t_out] of ConstantMedium::hit's two
              boundary queries, (-inf, inf) and (t_in + 0.0001, inf)

Every candidate carries a margin, the smallest relative distance to anything that could flip its verdict: disc / half_b^2 for
spheres; the distance of the plane point to the nearest edge (or ring radius) over the primitive's extent; |t - t_min| and
|t - t_max| over max(|t|, t_min); |d . n| / |d| for planar kinds. A hit's margin is the smallest of its conditions, a miss's
the largest of the conditions that fail (all of them would have to flip). A ray is AMBIGUOUS, and left out, when its winner's
margin is below MARGIN. A miss cannot lose accuracy, it can only flip, and that takes a margin within the rounding of one
formula (30 operations at 2^-53, under 1e-14): a ray is ambiguous too when a miss with a margin below NEAR_MISS = 1e-9 would
have come before its winner. A ray whose two nearest candidates are closer than the tolerance is a TIE: nothing is wrong with
its t, which is still compared; only the leaf may be either of the two.

Tolerance: |t_got - t_ref| |d| <= TOL (|o| + |p_ref| + |t_ref| |d|). Each formula is under ~30 f64 operations at 2^-53; a
margin of 1e-4 bounds the amplification through the square root and the divisions by 5e3: under 2e-11. TOL = 1e-9 leaves 50x
over that and stays four orders below the smallest feature of any scene used.
"""
import ctypes as C

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "brute_hits needs an extended-precision longdouble (x87, 64-bit mantissa): this numpy has %d bits" % np.finfo(LD).nmant

MARGIN = 1e-4
NEAR_MISS = 1e-9
TOL = 1e-9

(K_NODE, K_SPHERE, K_MOVING_SPHERE, K_RECT, K_BOX, K_TRIANGLE, K_RING, K_MEDIUM, K_TRANSLATE, K_ROTATE_Y, K_ZOOM, K_LIST) = range(12)
FLIP, KIND_SHIFT, INDEX_MASK, REF_NONE = 0x80000000, 27, 0x07FFFFFF, 0xFFFFFFFF
RECT_AXES = {0: (2, 0, 1), 1: (1, 0, 2), 2: (0, 1, 2)}          # rt_rect_axis → (the plane's axis, the a axis, the b axis)

_f8, _u4 = "<f8", "<u4"
POOL_DTYPES = {
    "nodes": np.dtype([("bmin", _f8, 3), ("bmax", _f8, 3), ("left", _u4), ("right", _u4), ("_pad", _u4, 2)]),
    "spheres": np.dtype([("center", _f8, 3), ("radius", _f8), ("mat", _u4), ("_pad", _u4)]),
    "moving_spheres": np.dtype([("center0", _f8, 3), ("center1", _f8, 3), ("time0", _f8), ("time1", _f8), ("radius", _f8),
                                ("mat", _u4), ("_pad", _u4)]),
    "rects": np.dtype([("a0", _f8), ("a1", _f8), ("b0", _f8), ("b1", _f8), ("k", _f8), ("axis", _u4), ("mat", _u4)]),
    "boxes": np.dtype([("p0", _f8, 3), ("p1", _f8, 3), ("mat", _u4), ("_pad", _u4)]),
    "triangles": np.dtype([("a", _f8, 3), ("b", _f8, 3), ("c", _f8, 3), ("mat", _u4), ("_pad", _u4)]),
    "rings": np.dtype([("r", _f8), ("t", _f8), ("dis_min", _f8), ("dis_max", _f8), ("mat", _u4), ("_pad", _u4)]),
    "media": np.dtype([("boundary", _u4), ("mat", _u4), ("neg_inv_density", _f8)]),
    "xforms": np.dtype([("kind", _u4), ("child", _u4), ("p", _f8, 3)]),
    "lists": np.dtype([("first", _u4), ("count", _u4)]),
    "list_items": np.dtype(_u4),
}
assert [POOL_DTYPES[k].itemsize for k in ("nodes", "spheres", "moving_spheres", "rects", "boxes", "triangles", "rings", "media",
                                          "xforms", "lists")] == [64, 40, 80, 48, 56, 80, 40, 16, 32, 8]


def ref_kind(ref):
    return (int(ref) >> KIND_SHIFT) & 0xF


def ref_index(ref):
    return int(ref) & INDEX_MASK


# ---- the walker -----------------------------------------------------------------------------------------------------------
class LeafPath:
    """One way from the root to a leaf: `movers` [(kind, (p0, p1, p2))] outermost first, `flip` the parity of the FlipFace bits
    on the way (the leaf's own included), `leaf` the leaf's ref as its parent holds it, `nodes` [(node index, movers above it)]
    for every NODE on the way, `medium` the index into Scene.media of the medium whose boundary this is, or None. `flips` is
    the same parity level by level, len(movers) + 1 entries, outermost first: flips[j] is the parity of the bits on the refs
    from below mover j - 1 down to mover j's own ref (the leaf's own for the last entry) — a mover's set_face_normal
    recomputes the flag, so a record needs to know on which side of each mover a bit sits (tests/brute_records.py)."""
    __slots__ = ("movers", "flip", "leaf", "nodes", "medium", "flips")

    def __init__(self, movers, flip, leaf, nodes, medium, flips=None):
        self.movers, self.flip, self.leaf, self.nodes, self.medium = movers, flip, leaf, nodes, medium
        self.flips = (flip,) if flips is None else flips

    @property
    def zoomed(self):
        """Class 2 can take this path: a Zoom of rate != 1 lies on it UNDER a node. The node's box is in the units of its own
        frame, the t the zoomed object reports in the units of the frame below the Zoom; with no node above the Zoom nothing
        compares the two, and inside the Zoom boxes and t agree."""
        return any(k == K_ZOOM and p[0] != 1.0 and any(above <= j for _, above in self.nodes) for j, (k, p) in enumerate(self.movers))


class Medium:
    __slots__ = ("ref", "index", "mat", "nodes", "n_movers", "boundary")

    def __init__(self, ref, index, mat, nodes, n_movers):
        self.ref, self.index, self.mat, self.nodes, self.n_movers, self.boundary = ref, index, mat, nodes, n_movers, []


class Scene:
    """The pools of a desc as numpy records, the solid leaf paths and the media."""

    def __init__(self, desc):
        self.pools = {}
        for name, dt in POOL_DTYPES.items():
            n = int(getattr(desc, "n_" + name))
            raw = C.string_at(getattr(desc, name), n * dt.itemsize) if n else b""
            self.pools[name] = np.frombuffer(raw, dtype=dt)
        self.root = int(desc.root)
        self.paths, self.media = [], []
        stack = [(self.root, (), False, (), None, (), False)]
        while stack:                                             # (explicit: node chains run to 64 links and more)
            ref, movers, flip, nodes, medium, flips, seg = stack.pop()
            kind, idx = ref_kind(ref), ref_index(ref)
            flip = flip != bool(ref & FLIP)
            seg = seg != bool(ref & FLIP)
            if kind == K_NODE:
                n = self.pools["nodes"][idx]
                below = nodes + ((idx, len(movers)),)
                if n["right"] != n["left"]:                      # (a span-1 node holds one object twice: one path)
                    stack.append((int(n["right"]), movers, flip, below, medium, flips, seg))
                stack.append((int(n["left"]), movers, flip, below, medium, flips, seg))
            elif kind == K_LIST:
                l = self.pools["lists"][idx]
                for r in self.pools["list_items"][int(l["first"]):int(l["first"]) + int(l["count"])][::-1]:
                    stack.append((int(r), movers, flip, nodes, medium, flips, seg))
            elif K_TRANSLATE <= kind <= K_ZOOM:
                x = self.pools["xforms"][idx]
                assert int(x["kind"]) == kind
                stack.append((int(x["child"]), movers + ((kind, tuple(float(v) for v in x["p"])),), flip, nodes, medium, flips + (seg,), False))
            elif kind == K_MEDIUM:
                assert medium is None, "a medium inside a medium's boundary"
                m = self.pools["media"][idx]
                self.media.append(Medium(ref, idx, int(m["mat"]), nodes, len(movers)))
                stack.append((int(m["boundary"]), movers, False, nodes, len(self.media) - 1, (False,) * len(movers), False))
            else:
                assert K_SPHERE <= kind <= K_RING, kind
                p = LeafPath(movers, flip, ref, nodes, medium, flips + (seg,))
                (self.paths if medium is None else self.media[medium].boundary).append(p)


# ---- movers ---------------------------------------------------------------------------------------------------------------
def ray_in(movers, o, d):
    """World ray (n, 3) → the leaf's frame, movers outermost first."""
    for kind, p in movers:
        if kind == K_TRANSLATE:
            o = o - np.array(p, dtype=LD)
        elif kind == K_ROTATE_Y:
            s, c = LD(p[0]), LD(p[1])
            o = np.stack([c * o[:, 0] - s * o[:, 2], o[:, 1], s * o[:, 0] + c * o[:, 2]], axis=1)
            d = np.stack([c * d[:, 0] - s * d[:, 2], d[:, 1], s * d[:, 0] + c * d[:, 2]], axis=1)
        else:
            o = o / LD(p[0])
    return o, d


def point_out(movers, p):
    """Points (..., 3) of the leaf's frame → the frame above `movers` (innermost applied first): the inverse maps of ray_in
    on points. Zoom scales points by its rate."""
    for kind, q in reversed(movers):
        if kind == K_TRANSLATE:
            p = p + np.array(q, dtype=LD)
        elif kind == K_ROTATE_Y:
            s, c = LD(q[0]), LD(q[1])
            p = np.stack([c * p[..., 0] + s * p[..., 2], p[..., 1], -s * p[..., 0] + c * p[..., 2]], axis=-1)
        else:
            p = p * LD(q[0])
    return p


# ---- primitives: rays (R, 1, ...) against P primitives (1, P, ...) → (hit, t, margin), each (R, P) -------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def _window(t, t_min, t_max):
    """Signed relative distance of t to the nearer end of [t_min, t_max]: >= 0 inside."""
    with np.errstate(all="ignore"):
        return np.minimum(t - t_min, t_max - t) / np.maximum(np.abs(t), t_min)


def _verdict(conds, safe=()):
    """conds: signed margins that must all be >= 0 for a hit; safe: positive margins that only bound a hit's accuracy."""
    s = np.stack(np.broadcast_arrays(*[np.asarray(c, dtype=np.float64) for c in conds]))
    s = np.where(np.isnan(s), -np.inf, s)
    hit = (s >= 0).all(0)
    m_hit = s.min(0)
    for e in safe:
        m_hit = np.minimum(m_hit, np.where(np.isnan(e), 0.0, np.asarray(e, dtype=np.float64)))
    m_miss = np.where(s < 0, -s, -np.inf).max(0)
    return hit, np.where(hit, m_hit, m_miss)


def hit_sphere(o, d, c, r, t_min, t_max):
    with np.errstate(all="ignore"):
        oc = o - c
        a = _dot(d, d)
        hb = _dot(oc, d)
        l = oc - (hb / a)[..., None] * d                       # the ray's point nearest the centre, from the centre
        dl = np.sqrt(_dot(l, l))
        disc = a * (r - dl) * (r + dl)
        cc = _dot(oc, oc) - r * r
        sq = np.sqrt(np.where(disc > 0, disc, 0))
        q = -(hb + np.where(hb < 0, -sq, sq))                  # the root with no cancellation; the other is cc / q
        r1, r2 = q / a, cc / q
        r2 = np.where(q == 0, r1, r2)
        lo, hi = np.minimum(r1, r2), np.maximum(r1, r2)
        s_disc = np.asarray(disc / (hb * hb), dtype=np.float64)
        s_disc = np.where(np.isnan(s_disc), np.where(disc >= 0, np.inf, -np.inf), s_disc)
        w_lo = np.nan_to_num(np.asarray(_window(lo, t_min, t_max), dtype=np.float64), nan=-np.inf)
        w_hi = np.nan_to_num(np.asarray(_window(hi, t_min, t_max), dtype=np.float64), nan=-np.inf)
    real = disc >= 0
    use_lo = real & (w_lo >= 0)
    use_hi = real & ~use_lo & (w_hi >= 0)
    hit = use_lo | use_hi
    t = np.where(use_lo, lo, hi)
    margin = np.where(~real, -s_disc,
                      np.where(use_lo, np.minimum(s_disc, w_lo),
                               np.where(use_hi, np.minimum(s_disc, np.minimum(-w_lo, w_hi)), np.minimum(np.abs(w_lo), np.abs(w_hi)))))
    t = np.where(real, t, -hb / a)                             # (a near miss's would-be t: the point of closest approach)
    return hit, t, margin


def hit_rect(o, d, axes, a0, a1, b0, b1, k, t_min, t_max):
    """axes: (3, P) int: the plane's axis and the two in-plane axes per primitive."""
    with np.errstate(all="ignore"):
        o2, d2 = o[:, 0, :], d[:, 0, :]
        ok, dk = o2[:, axes[0]], d2[:, axes[0]]
        t = (k - ok) / dk
        a = o2[:, axes[1]] + t * d2[:, axes[1]]
        b = o2[:, axes[2]] + t * d2[:, axes[2]]
        ext = np.maximum(a1 - a0, b1 - b0)
        conds = [_window(t, t_min, t_max), (a - a0) / ext, (a1 - a) / ext, (b - b0) / ext, (b1 - b) / ext]
        steep = np.abs(dk) / np.sqrt(_dot(d, d))
    hit, margin = _verdict(conds, safe=[steep])
    return hit, t, margin


def hit_triangle(o, d, a, b, c, t_min, t_max):
    with np.errstate(all="ignore"):
        n = np.cross(b - a, c - a)
        nn = _dot(n, n)
        dn = _dot(d, n)
        t = _dot(a - o, n) / dn
        p = o + t[..., None] * d
        edges = ((b, c), (c, a), (a, b))
        ext = np.sqrt(np.maximum(np.maximum(_dot(b - a, b - a), _dot(c - b, c - b)), _dot(a - c, a - c)))
        conds = [_window(t, t_min, t_max)]
        for u, v in edges:                                      # the signed distance of p to the edge's line, inside positive
            e = v - u
            conds.append(_dot(np.cross(e, p - u), n) / (np.sqrt(nn) * np.sqrt(_dot(e, e))) / ext)
        steep = np.abs(dn) / np.sqrt(nn * _dot(d, d))
    hit, margin = _verdict(conds, safe=[steep])
    return hit, t, margin


def hit_ring(o, d, r_in, r_out, t_min, t_max):
    with np.errstate(all="ignore"):
        t = -o[..., 1] / d[..., 1]
        p = o + t[..., None] * d
        rho = np.sqrt(p[..., 0] * p[..., 0] + p[..., 2] * p[..., 2])
        conds = [_window(t, t_min, t_max), (rho - r_in) / r_out, (r_out - rho) / r_out]
        steep = np.abs(d[..., 1]) / np.sqrt(_dot(d, d))
    hit, margin = _verdict(conds, safe=[steep])
    return hit, np.broadcast_to(t, hit.shape), margin


def _ld(x):
    return np.asarray(x, dtype=LD)


def leaf_hits(scene, kind, idx, o, d, tm, t_min, t_max):
    """Rays in the leaves' frame, o, d (R, 3), tm / t_min / t_max (R,), against the primitives `idx` of one kind →
    (hit, t, margin) of shape (R, C) and the column → position-in-idx map (a box makes six columns, one per face)."""
    P = scene.pools
    o3, d3 = o[:, None, :], d[:, None, :]
    lo, hi = _ld(t_min)[:, None], _ld(t_max)[:, None]
    cols = np.arange(len(idx))
    if kind == K_SPHERE:
        s = P["spheres"][idx]
        out = hit_sphere(o3, d3, _ld(s["center"])[None], _ld(s["radius"])[None], lo, hi)
    elif kind == K_MOVING_SPHERE:
        s = P["moving_spheres"][idx]
        f = (_ld(tm)[:, None] - _ld(s["time0"])[None]) / (_ld(s["time1"]) - _ld(s["time0"]))[None]
        c = _ld(s["center0"])[None] + f[..., None] * (_ld(s["center1"]) - _ld(s["center0"]))[None]
        out = hit_sphere(o3, d3, c, _ld(s["radius"])[None], lo, hi)
    elif kind == K_RECT:
        q = P["rects"][idx]
        axes = np.array([RECT_AXES[int(a)] for a in q["axis"]]).T.reshape(3, -1)
        out = hit_rect(o3, d3, axes, *(_ld(q[f])[None] for f in ("a0", "a1", "b0", "b1", "k")), lo, hi)
    elif kind == K_BOX:
        bx = P["boxes"][idx]
        p0, p1 = _ld(bx["p0"]), _ld(bx["p1"])
        axes, par = [], []
        for ka, aa, ba in RECT_AXES.values():
            for side in (p1, p0):
                axes.append(np.tile(np.array([[ka], [aa], [ba]]), (1, len(idx))))
                par.append((p0[:, aa], p1[:, aa], p0[:, ba], p1[:, ba], side[:, ka]))
        axes = np.concatenate(axes, axis=1)
        par = [np.concatenate([f[j] for f in par])[None] for j in range(5)]
        cols = np.tile(np.arange(len(idx)), 6)
        out = hit_rect(o3, d3, axes, *par, lo, hi)
    elif kind == K_TRIANGLE:
        tr = P["triangles"][idx]
        out = hit_triangle(o3, d3, _ld(tr["a"])[None], _ld(tr["b"])[None], _ld(tr["c"])[None], lo, hi)
    else:
        assert kind == K_RING
        g = P["rings"][idx]
        out = hit_ring(o3, d3, np.sqrt(_ld(g["dis_min"]))[None], np.sqrt(_ld(g["dis_max"]))[None], lo, hi)
    return out + (cols,)


def candidates(scene, paths, o, d, tm, t_min, t_max, chunk=400_000):
    """Every path against every ray → hit (R, C) bool, t (R, C) longdouble, margin (R, C) float64, col_path (C,): the index
    into `paths` of each column."""
    R = len(o)
    groups = {}
    for i, p in enumerate(paths):
        groups.setdefault((p.movers, ref_kind(p.leaf)), []).append(i)
    H, T, M, col_path = [], [], [], []
    for (movers, kind), members in groups.items():
        oo, dd = ray_in(movers, o, d)
        members = np.array(members)
        step = max(1, chunk // max(R, 1) // (6 if kind == K_BOX else 1))
        for s in range(0, len(members), step):
            part = members[s:s + step]
            idx = np.array([ref_index(paths[i].leaf) for i in part])
            h, t, m, cols = leaf_hits(scene, kind, idx, oo, dd, tm, t_min, t_max)
            H.append(h); T.append(t); M.append(m); col_path.append(part[cols])
    if not H:
        return np.zeros((R, 0), bool), np.zeros((R, 0), LD), np.zeros((R, 0)), np.zeros(0, int)
    return np.concatenate(H, 1), np.concatenate(T, 1), np.concatenate(M, 1), np.concatenate(col_path)


# ---- the nearest candidate of every ray --------------------------------------------------------------------------------------
class Answer:
    """Per ray: hit, t (longdouble), path (index into scene.paths, -1 on a miss), leaf (the winner's ref, REF_NONE on a miss),
    margin, ambiguous (a winner's margin below MARGIN, or a near miss before it), tie (the two nearest candidates closer than
    the tolerance: t is still compared, the leaf may be either's), zoomed (class 2: an in-window candidate under a Zoom of
    rate != 1 that has a node above it), front (the winner's front_face where its path has no mover: the ray runs against the
    leaf's outward normal, turned over by the FlipFace bits on the path; moved says the path has movers), ring_parallel (class 3: t_max = +inf and, in some Ring's frame, a direction with y == 0 and x or z == 0), p (the winner's point,
    world frame), scale (|o| + |p| + |t| |d|: the tolerance is TOL * scale / |d|)."""
    pass


def tolerance(ans, d):
    """The bound on |t_got - t_ref| per ray."""
    return TOL * ans.scale / np.sqrt((np.asarray(d, dtype=np.float64) ** 2).sum(1))


def solve(scene, origin, direction, time, t_min, t_max, block=500):
    n = len(origin)
    o_all, d_all = _ld(origin).reshape(n, 3), _ld(direction).reshape(n, 3)
    tm_all, lo_all, hi_all = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in (time, t_min, t_max))
    a = Answer()
    a.hit = np.zeros(n, bool); a.t = np.full(n, np.inf, dtype=LD); a.path = np.full(n, -1); a.margin = np.full(n, np.inf)
    a.ambiguous = np.zeros(n, bool); a.zoomed = np.zeros(n, bool); a.p = np.zeros((n, 3)); a.scale = np.zeros(n)
    a.tie = np.zeros(n, bool); a.ring_parallel = np.zeros(n, bool); a.front = np.zeros(n, bool); a.moved = np.zeros(n, bool)
    for movers in {p.movers for p in scene.paths if ref_kind(p.leaf) == K_RING}:
        dd = ray_in(movers, o_all, d_all)[1]
        a.ring_parallel |= (dd[:, 1] == 0) & ((dd[:, 0] == 0) | (dd[:, 2] == 0)) & (hi_all == np.inf)
    zoomed_path = np.array([p.zoomed for p in scene.paths], dtype=bool)
    for s in range(0, n, block):
        sl = slice(s, min(n, s + block))
        o, d = o_all[sl], d_all[sl]
        H, T, M, cp = candidates(scene, scene.paths, o, d, tm_all[sl], lo_all[sl], hi_all[sl])
        r = np.arange(len(o))
        if H.shape[1] == 0:
            continue
        Th = np.where(H, T, np.inf)
        order = np.argsort(Th, axis=1)[:, :2]
        w = order[:, 0]
        hit = H[r, w]
        t = Th[r, w]
        dlen = np.sqrt(_dot(d, d))
        p = np.zeros((len(o), 3), dtype=LD)
        for movers in {scene.paths[cp[c]].movers for c in w[hit]}:
            sel = hit & np.array([scene.paths[cp[c]].movers == movers for c in w])
            oo, dd = ray_in(movers, o[sel], d[sel])
            p[sel] = point_out(movers, oo + t[sel][:, None] * dd)
        for c in set(w[hit]):                                    # the winners' faces, leaf by leaf
            path = scene.paths[cp[c]]
            sel = hit & (w == c)
            a.moved[s + np.flatnonzero(sel)] = bool(path.movers)
            if not path.movers:
                a.front[s + np.flatnonzero(sel)] = (outward_dot(scene, path.leaf, o[sel] + t[sel][:, None] * d[sel], d[sel], tm_all[sl][sel]) < 0) != path.flip
        scale = np.sqrt(_dot(o, o)) + np.sqrt(_dot(p, p)) + np.where(hit, np.abs(t), 0) * dlen
        tol = np.asarray(TOL * scale / dlen, dtype=np.float64)
        amb = hit & (M[r, w] < MARGIN)
        if H.shape[1] > 1:
            with np.errstate(invalid="ignore"):
                a.tie[sl] = hit & (Th[r, order[:, 1]] - t <= tol)
        with np.errstate(invalid="ignore"):
            near_miss = ~H & (M < NEAR_MISS) & ~(T > (np.where(hit, t, np.inf) + tol)[:, None])
        amb |= near_miss.any(1)
        a.hit[sl], a.t[sl], a.margin[sl], a.ambiguous[sl] = hit, t, M[r, w], amb
        a.path[sl] = np.where(hit, cp[w], -1)
        a.zoomed[sl] = (H & zoomed_path[cp][None, :]).any(1)
        a.p[sl], a.scale[sl] = p, scale
    leafs = np.array([p.leaf for p in scene.paths] + [REF_NONE], dtype=np.uint32)
    a.leaf = leafs[a.path]
    return a


def outward_dot(scene, leaf, p, d, tm):
    """d . n for the leaf's outward normal n at the points p (both in the leaf's frame): the sphere's radius vector; +axis for a
    rect and for every face of a box (Boxes is six plain rects, boxes.rs:24-66); (b - a) x (c - a); +y for a ring."""
    P, kind, i = scene.pools, ref_kind(leaf), ref_index(leaf)
    if kind == K_SPHERE:
        return _dot(d, p - _ld(P["spheres"][i]["center"])[None])
    if kind == K_MOVING_SPHERE:
        q = P["moving_spheres"][i]
        f = (_ld(tm) - LD(q["time0"])) / (LD(q["time1"]) - LD(q["time0"]))
        return _dot(d, p - (_ld(q["center0"])[None] + f[:, None] * (_ld(q["center1"]) - _ld(q["center0"]))[None]))
    if kind == K_RECT:
        return d[:, RECT_AXES[int(P["rects"][i]["axis"])][0]]
    if kind == K_BOX:
        q = P["boxes"][i]
        gap = np.minimum(np.abs(p - _ld(q["p0"])[None]), np.abs(p - _ld(q["p1"])[None])) / (_ld(q["p1"]) - _ld(q["p0"]))[None]
        return d[np.arange(len(d)), np.argmin(gap, axis=1)]         # (the face the point lies on)
    if kind == K_TRIANGLE:
        q = P["triangles"][i]
        return _dot(d, np.cross(_ld(q["b"]) - _ld(q["a"]), _ld(q["c"]) - _ld(q["a"]))[None])
    return d[:, 1]


def matches_a_candidate(scene, origin, direction, time, t_min, t_max, t_got, leaf_got=None):
    """The weaker claim of class-2 rays: (t_got[, leaf_got]) is SOME in-window candidate's own (t, leaf), within tolerance."""
    n = len(origin)
    o, d = _ld(origin).reshape(n, 3), _ld(direction).reshape(n, 3)
    bc = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))
    H, T, _, cp = candidates(scene, scene.paths, o, d, bc(time), bc(t_min), bc(t_max))
    dlen = np.sqrt(_dot(d, d))
    tol = TOL * (2 * np.sqrt(_dot(o, o)) + 2 * np.abs(_ld(t_got)) * dlen) / dlen         # (|p| <= |o| + |t| |d|)
    ok = H & (np.abs(T - _ld(t_got)[:, None]) <= tol[:, None])
    if leaf_got is not None:
        leafs = np.array([p.leaf for p in scene.paths], dtype=np.uint32)
        ok &= leafs[cp][None, :] == np.asarray(leaf_got, dtype=np.uint32)[:, None]
    return ok.any(1)


def chord(scene, medium, origin, direction, time, t_min, t_max):
    """[t_in, t_out] of a medium for every ray, as ConstantMedium::hit cuts it: the boundary's nearest hit over (-inf, inf),
    its nearest hit after t_in + 0.0001, both clamped to the window and t_in to >= 0. crossed: both boundary hits exist
    and the clamped chord is not empty."""
    n = len(origin)
    o, d = _ld(origin).reshape(n, 3), _ld(direction).reshape(n, 3)
    tm = np.broadcast_to(np.asarray(time, dtype=np.float64), (n,))
    inf = np.full(n, np.inf)
    H, T, _, _ = candidates(scene, medium.boundary, o, d, tm, -inf, inf)
    t_in = np.where(H, T, np.inf).min(1)
    H2, T2, _, _ = candidates(scene, medium.boundary, o, d, tm, t_in + LD(0.0001), inf)
    t_out = np.where(H2, T2, np.inf).min(1)
    crossed = np.isfinite(t_in) & np.isfinite(t_out)
    t_in = np.maximum(np.maximum(t_in, _ld(t_min)), 0)
    t_out = np.minimum(t_out, _ld(t_max))
    return t_in, t_out, crossed & (t_in < t_out)


# ---- node boxes: the only two readers ------------------------------------------------------------------------------------------
def node_boxes(scene):
    """(bmin, bmax) arrays of the node pool, for the enclosure check."""
    return np.array(scene.pools["nodes"]["bmin"]), np.array(scene.pools["nodes"]["bmax"])


def flat_node_paths(scene):
    """Class 1: per solid path, whether it lies under a node whose box has bmin == bmax on an axis (AABB::hit answers a miss for
    t_max <= t_min: such a node hides everything under it)."""
    lo, hi = node_boxes(scene)
    flat = (lo == hi).any(1) if len(lo) else np.zeros(0, bool)
    return np.array([any(flat[i] for i, _ in p.nodes) for p in scene.paths], dtype=bool)


# ---- enclosure -------------------------------------------------------------------------------------------------------------------
def surface_points(scene, path, times, n_samples=24, seed=0):
    """Points of the leaf's surface in its own frame, (len(times), k, 3): the corners / vertices (the extremes of every affine
    image), the sphere's and the ring's axis extremes, and sampled points between."""
    P = scene.pools
    kind, i = ref_kind(path.leaf), ref_index(path.leaf)
    g = np.random.default_rng(seed)
    nt = len(times)
    if kind in (K_SPHERE, K_MOVING_SPHERE):
        v = g.normal(size=(n_samples, 3))
        v = np.concatenate([v / np.linalg.norm(v, axis=1, keepdims=True), np.eye(3), -np.eye(3)])
        if kind == K_SPHERE:
            s = P["spheres"][i]
            c = np.broadcast_to(_ld(s["center"]), (nt, 3))
        else:
            s = P["moving_spheres"][i]
            f = (_ld(times) - LD(s["time0"])) / (LD(s["time1"]) - LD(s["time0"]))
            c = _ld(s["center0"])[None] + f[:, None] * (_ld(s["center1"]) - _ld(s["center0"]))[None]
        return c[:, None, :] + LD(s["radius"]) * _ld(v)[None]
    if kind == K_RECT:
        q = P["rects"][i]
        ka, aa, ba = RECT_AXES[int(q["axis"])]
        uv = np.concatenate([g.random((n_samples, 2)), [[0, 0], [0, 1], [1, 0], [1, 1]]])
        pts = np.zeros((len(uv), 3), dtype=LD)
        pts[:, ka] = LD(q["k"])
        pts[:, aa] = LD(q["a0"]) + _ld(uv[:, 0]) * (LD(q["a1"]) - LD(q["a0"]))
        pts[:, ba] = LD(q["b0"]) + _ld(uv[:, 1]) * (LD(q["b1"]) - LD(q["b0"]))
    elif kind == K_BOX:
        bx = P["boxes"][i]
        u = np.concatenate([g.random((n_samples, 3)), np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])])
        u[:n_samples, g.integers(0, 3, n_samples)] = g.integers(0, 2, n_samples)          # (onto a face)
        pts = _ld(bx["p0"])[None] + _ld(u) * (_ld(bx["p1"]) - _ld(bx["p0"]))[None]
    elif kind == K_TRIANGLE:
        tr = P["triangles"][i]
        w = np.concatenate([g.dirichlet((1, 1, 1), n_samples), np.eye(3)])
        pts = _ld(w) @ np.stack([_ld(tr["a"]), _ld(tr["b"]), _ld(tr["c"])])
    else:
        rg = P["rings"][i]
        ang = np.concatenate([g.uniform(0, 2 * np.pi, n_samples), np.arange(4) * np.pi / 2])
        rad = np.concatenate([np.sqrt(g.uniform(rg["dis_min"], rg["dis_max"], n_samples)), np.full(4, np.sqrt(rg["dis_max"]))])
        pts = np.stack([_ld(rad * np.cos(ang)), np.zeros(len(ang), dtype=LD), _ld(rad * np.sin(ang))], axis=1)
        pts[-4:] = np.sqrt(LD(rg["dis_max"])) * _ld([[1, 0, 0], [0, 0, 1], [-1, 0, 0], [0, 0, -1]])
    return np.broadcast_to(pts, (nt,) + pts.shape)


def round_extremes(scene, path, movers, times):
    """The axis extremes of a sphere (or of a ring's outer circle) in the frame above `movers`: rotations keep it round, a Zoom
    scales its radius, so they are centre' +- radius' e_axis there and no sampled point of the leaf's own frame."""
    P = scene.pools
    kind, i = ref_kind(path.leaf), ref_index(path.leaf)
    if kind not in (K_SPHERE, K_MOVING_SPHERE, K_RING):
        return np.zeros((len(times), 0, 3), dtype=LD)
    if kind == K_RING:
        c = np.zeros((len(times), 3), dtype=LD)
        r, axes = np.sqrt(LD(P["rings"][i]["dis_max"])), (0, 2)
    else:
        c = surface_points(scene, path, times, n_samples=0).mean(1)                      # (the six axis points average to the centre)
        r, axes = LD((P["spheres"] if kind == K_SPHERE else P["moving_spheres"])[i]["radius"]), (0, 1, 2)
    c = point_out(movers, c)
    for k, q in movers:
        if k == K_ZOOM:
            r = r * abs(LD(q[0]))
    e = np.concatenate([np.eye(3)[list(axes)], -np.eye(3)[list(axes)]])
    return c[:, None, :] + r * _ld(e)[None]


def enclosure_violations(scene, times, slack=1e-12):
    """Every NODE against every leaf path under it (solid and boundary paths alike): the leaf's surface, carried out through
    the movers BETWEEN the node and the leaf (a mover above the node does not apply), must lie in the node's box, give or take
    `slack` x the box's diagonal. → (violations [(node, leaf ref, worst excess / diagonal)], flat [(node, axis)] — nodes with
    a zero-extent axis, reported and not failed: class 1)."""
    lo, hi = node_boxes(scene)
    lo, hi = _ld(lo), _ld(hi)
    times = np.asarray(times, dtype=np.float64)
    worst, flat = {}, set()
    every = list(scene.paths) + [p for m in scene.media for p in m.boundary]
    for p in every:
        pts_cache = {}
        for node, above in p.nodes:
            if above not in pts_cache:
                between = p.movers[above:]
                pts = point_out(between, surface_points(scene, p, times, seed=len(p.movers) + ref_index(p.leaf)))
                pts_cache[above] = np.concatenate([pts, round_extremes(scene, p, between, times)], axis=1).reshape(-1, 3)
            pts = pts_cache[above]
            diag = np.sqrt(((hi[node] - lo[node]) ** 2).sum())
            for ax in range(3):
                if lo[node][ax] == hi[node][ax]:
                    flat.add((node, ax))
            excess = np.maximum(lo[node][None] - pts, pts - hi[node][None]).max()
            if not np.isfinite(diag):
                continue
            if excess > slack * diag:
                rel = float(excess / diag) if diag > 0 else np.inf
                if rel > worst.get((node, p.leaf), 0.0):
                    worst[(node, p.leaf)] = rel
    return [(n, l, e) for (n, l), e in sorted(worst.items())], sorted(flat)


# ---- ray families ------------------------------------------------------------------------------------------------------------
RAY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("direction", "<f8", (3,)), ("time", "<f8"), ("t_min", "<f8"), ("t_max", "<f8"),
                      ("rng_state", "<u8")])                   # rt_query_ray


def _rays(o, d, time, t_min, t_max, g):
    n = len(o)
    r = np.zeros(n, dtype=RAY_DTYPE)
    r["origin"], r["direction"], r["time"], r["t_min"], r["t_max"] = o, d, time, t_min, t_max
    r["rng_state"] = g.integers(1, 2**63, n, dtype=np.uint64)
    return r


def _unit(g, n):
    v = g.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def scene_bounds(scene):
    """A box round the scene's objects for aiming rays, from the leaves themselves (no node box): the extremes of every solid
    leaf at mid-shutter, leaving out leaves over 20 times the median size (a ground sphere of radius 1000) where there are more
    than four."""
    lo, hi = [], []
    for p in scene.paths:
        pts = point_out(p.movers, surface_points(scene, p, [0.5], n_samples=0))
        pts = np.concatenate([pts, round_extremes(scene, p, p.movers, [0.5])], axis=1).reshape(-1, 3)
        lo.append(pts.min(0)); hi.append(pts.max(0))
    lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    size = (hi - lo).max(1)
    keep = size <= 20 * np.median(size) if len(size) > 4 else np.ones(len(size), bool)
    return lo[keep].min(0), hi[keep].max(0)


FAMILIES = ("camera", "bounce", "random", "axis")


def ray_families(scene, cam_origin, cam_llc, cam_h, cam_v, shutter, n, seed):
    """{family: rays}: n / 4 rays each. camera: pinhole rays of the view at times across the shutter, windows {0.001, 0.5} x
    {inf, finite}; bounce: from the reference's own hit points of the camera rays in random directions, t_min 0.001 or 0.5;
    random: through the scene's bounds; axis: parallel to an axis (two zero components) or to an axis plane (one), from random
    origins. Everything is decided here and by the reference, before any result exists."""
    g = np.random.default_rng(seed)
    k = n // 4
    t0, t1 = shutter
    times = lambda m: g.uniform(t0, t1, m)

    def windows(m, reach, d):
        """t_min 0.001 or 0.5; t_max +inf for 15 % of the rays, else so that the ray ends between 0.4 and 1.1 `reach`."""
        lo = g.choice([0.001, 0.5], m)
        return lo, np.where(g.random(m) < 0.15, np.inf, lo + g.uniform(0.4, 1.1, m) * reach / np.linalg.norm(d, axis=1))
    lo_b, hi_b = scene_bounds(scene)
    span = np.maximum(hi_b - lo_b, 1e-3 * np.linalg.norm(hi_b - lo_b))
    far = float(np.linalg.norm(span))
    out = {}
    s, t = g.random(k), g.random(k)
    o = np.broadcast_to(np.asarray(cam_origin, dtype=np.float64), (k, 3))
    d = np.asarray(cam_llc)[None] + s[:, None] * np.asarray(cam_h)[None] + t[:, None] * np.asarray(cam_v)[None] - o
    out["camera"] = _rays(o, d, times(k), *windows(k, float(np.linalg.norm(0.5 * (lo_b + hi_b) - o[0])), d), g)
    first = solve(scene, out["camera"]["origin"], out["camera"]["direction"], out["camera"]["time"], 0.001, np.inf)
    h = np.flatnonzero(first.hit)
    if len(h):
        pick = h[g.integers(0, len(h), k)]
        d = _unit(g, k)
        out["bounce"] = _rays(first.p[pick], d, out["camera"]["time"][pick], *windows(k, far, d), g)
    else:
        out["bounce"] = out["camera"][:0]
    d = _unit(g, k)
    out["random"] = _rays(lo_b - 0.25 * span + g.random((k, 3)) * 1.5 * span, d, times(k), *windows(k, far, d), g)
    d = _unit(g, k)
    zero = g.integers(0, 3, k)
    d[np.arange(k), zero] = 0.0
    two = g.random(k) < 0.5
    d[two, (zero[two] + 1) % 3] = 0.0
    out["axis"] = _rays(lo_b - 0.1 * span + g.random((k, 3)) * 1.2 * span, d, times(k), *windows(k, far, d), g)
    return out


def camera_of(cam):
    """(origin, lower_left_corner, horizontal, vertical, (time0, time1)) of an rt_camera."""
    return (np.array(cam.origin[:]), np.array(cam.lower_left_corner[:]), np.array(cam.horizontal[:]), np.array(cam.vertical[:]),
            (float(cam.time0), float(cam.time1)))


# ---- the comparison ----------------------------------------------------------------------------------------------------------
class Tally:
    """One scene and ray family: rays, compared, ambiguous, ties, classes 1 to 3, the worst error in units of the tolerance,
    and the failures [(ray index, what)]."""

    def __init__(self):
        self.rays = self.compared = self.ambiguous = self.ties = self.class1 = self.class2 = self.class3 = 0
        self.worst = 0.0
        self.failures = []

    def line(self, scene, family, who):
        return "%-22s %-7s %-6s rays %5d compared %5d ambiguous %4d class1 %4d class2 %4d class3 %4d ties %4d worst %.3e tol%s" % (
            scene, family, who, self.rays, self.compared, self.ambiguous, self.class1, self.class2, self.class3, self.ties,
            self.worst, "" if not self.failures else "  FAILURES %d" % len(self.failures))


def classify(scene, ans, flat=None):
    """→ (class1, class2, class3, ambiguous) per ray, from the reference alone. Class 1: the winner sits under a node with a
    zero-extent axis. Class 2: an in-window candidate under a Zoom of rate != 1. Class 3: t_max = +inf and a direction with
    y == 0 and x == 0 or z == 0 in some Ring's frame. A ray counts in the first class that takes it, and as ambiguous only if none does."""
    flat = flat_node_paths(scene) if flat is None else flat
    class1 = ans.hit & np.concatenate([flat, [False]])[ans.path]
    class2 = ans.zoomed & ~class1
    class3 = ans.ring_parallel & ~class1 & ~class2
    return class1, class2, class3, ans.ambiguous & ~class1 & ~class2 & ~class3


def compare(scene, rays, got_hit, got_t, got_draws, got_prim=None, ans=None, flat=None):
    """A set of results (the oracle's rto_hit, or the device's rt_intersect with got_prim) against the reference:
      - ambiguous rays are left out;
      - class 1 rays are left out; class 2 rays assert the weaker claim that a hit is SOME candidate's own (t, leaf); class 3
        rays that the result is the reference's, or a hit at t = +inf where the reference has none (ring.rs:37-47);
      - every other ray that drew no RNG: the same hit / miss, t within the tolerance, prim the winner's leaf (a tie: either
        of the tied leaves);
      - every other ray that drew (a medium took part): the nearest solid by the same rule, or a medium hit whose t lies in
        that medium's chord and at or before the nearest solid."""
    ans = ans or solve(scene, rays["origin"], rays["direction"], rays["time"], rays["t_min"], rays["t_max"])
    ta = Tally()
    ta.rays = len(rays)
    got_hit = np.asarray(got_hit).astype(bool)
    got_t = np.asarray(got_t, dtype=np.float64)
    got_draws = np.asarray(got_draws)
    prim = None if got_prim is None else np.asarray(got_prim, dtype=np.uint32)
    tol = tolerance(ans, rays["direction"])
    class1, class2, class3, amb = classify(scene, ans, flat)
    ta.ambiguous, ta.class1, ta.class2, ta.class3 = int(amb.sum()), int(class1.sum()), int(class2.sum()), int(class3.sum())
    check = ~(amb | class1 | class2 | class3)
    ta.compared, ta.ties = int(check.sum()), int((check & ans.tie).sum())
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        units = np.asarray(np.where(ans.hit & got_hit, np.abs(_ld(got_t) - ans.t) / tol, 0), dtype=np.float64)
    solid = (got_hit == ans.hit) & (~ans.hit | (units <= 1))                     # the nearest solid, as far as t says
    if prim is not None:
        leaf_ok = np.where(ans.hit, prim == ans.leaf, prim == REF_NONE)
        tied = np.flatnonzero(solid & ~leaf_ok & ans.tie & check)
        if len(tied):
            r = rays[tied]
            leaf_ok[tied] = matches_a_candidate(scene, r["origin"], r["direction"], r["time"], r["t_min"], r["t_max"], got_t[tied], prim[tied])
    else:
        leaf_ok = np.ones(len(rays), bool)

    def describe(i):
        return "hit %d t %r prim %s draws %d; reference hit %d t %r leaf %#x margin %.2e (%.3g tolerances)" % (
            got_hit[i], float(got_t[i]), "-" if prim is None else "%#x" % int(prim[i]), int(got_draws[i]), ans.hit[i], float(ans.t[i]),
            int(ans.leaf[i]), ans.margin[i], units[i])
    # class 2 and class 3: the weaker claims
    c2 = np.flatnonzero(class2 & got_hit & (got_draws == 0))
    if len(c2):
        r = rays[c2]
        ok = matches_a_candidate(scene, r["origin"], r["direction"], r["time"], r["t_min"], r["t_max"], got_t[c2], None if prim is None else prim[c2])
        ta.failures += [(int(i), "class 2, no candidate's own: " + describe(i)) for i in c2[~ok]]
    for i in np.flatnonzero(class3 & (got_draws == 0) & ~(solid & leaf_ok)):
        if not (got_hit[i] and got_t[i] == np.inf and not ans.hit[i]):
            ta.failures.append((int(i), "class 3: " + describe(i)))
    # rays that drew nothing
    plain = check & (got_draws == 0)
    ta.failures += [(int(i), describe(i)) for i in np.flatnonzero(plain & ~(solid & leaf_ok))]
    ok = check & solid & leaf_ok & got_hit
    # rays that drew: a medium took part
    drew = np.flatnonzero(check & (got_draws > 0) & ~(solid & leaf_ok))
    if len(drew):
        assert scene.media, "draws without a medium in the scene"
        r = rays[drew]
        chords = [chord(scene, m, r["origin"], r["direction"], r["time"], r["t_min"], r["t_max"]) for m in scene.media]
        for j, i in enumerate(drew):
            inside = False
            slack = tol[i] if np.isfinite(tol[i]) else TOL * max(1.0, abs(got_t[i]))
            for m, (t_in, t_out, crossed) in zip(scene.media, chords):
                if not got_hit[i] or (prim is not None and int(prim[i]) != m.ref):
                    continue
                inside |= bool(crossed[j] and t_in[j] - slack <= got_t[i] <= t_out[j] + slack and got_t[i] <= ans.t[i] + slack)
            if not inside:
                ta.failures.append((int(i), "neither the nearest solid nor inside a medium's chord: " + describe(i)))
    if ok.any():
        ta.worst = float(units[ok].max())
    return ta, ans
