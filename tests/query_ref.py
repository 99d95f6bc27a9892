"""The reference of the closest-hit queries (rt_intersect*) and what the query tests share: rto_hit ray by ray, the record
comparison, the counters of a query and the ray families. The reference itself needs no GPU."""
import numpy as np

from raytracer_2022_amd import _ffi as F

from compare import same_bits

FLOATS = ("t", "u", "v", "p", "normal")
LEAF_POOLS = {F.RT_KIND_SPHERE: "spheres", F.RT_KIND_MOVING_SPHERE: "moving_spheres", F.RT_KIND_RECT: "rects",
              F.RT_KIND_BOX: "boxes", F.RT_KIND_TRIANGLE: "triangles", F.RT_KIND_RING: "rings", F.RT_KIND_MEDIUM: "media"}


def oracle_hits(O, desc, rays):
    """rto_hit(desc, desc.root, ray, ...) for every ray → (HIT_DTYPE records without prim, summed rt_stats)."""
    out = np.zeros(len(rays), dtype=F.HIT_DTYPE)
    st = F.rt_stats()
    for i, r in enumerate(rays):
        rec = O.hit(desc, desc.root, r["origin"], r["direction"], tm=float(r["time"]), t_min=float(r["t_min"]),
                    t_max=float(r["t_max"]), rng_state=int(r["rng_state"]), stats=st)
        o = out[i]
        o["hit"], o["front_face"], o["rng_draws"] = rec.hit, rec.front_face, rec.rng_draws
        if rec.hit:
            o["t"], o["u"], o["v"], o["mat"] = rec.t, rec.u, rec.v, rec.mat
            o["p"], o["normal"] = rec.p[:], rec.normal[:]
    return out, st


def assert_records_equal(dev, ref, what=""):
    assert np.array_equal(dev["hit"], ref["hit"]), what
    assert np.array_equal(dev["rng_draws"], ref["rng_draws"]), what
    h = ref["hit"] == 1
    for f in FLOATS:
        assert same_bits(dev[f][h], ref[f][h]), (what, f)
    assert np.array_equal(dev["front_face"][h], ref["front_face"][h]), what
    assert np.array_equal(dev["mat"][h], ref["mat"][h]), what
    m = ~h
    assert np.all(dev["prim"][m] == F.RT_REF_NONE), what
    for f in FLOATS + ("front_face", "mat"):
        assert not np.any(dev[f][m]), (what, f)


def assert_prims_consistent(desc, hits):
    for rec in hits[hits["hit"] == 1]:
        kind, idx = F.ref_kind(int(rec["prim"])), F.ref_index(int(rec["prim"]))
        assert kind in LEAF_POOLS, kind
        assert idx < getattr(desc, "n_" + LEAF_POOLS[kind])
        assert getattr(desc, LEAF_POOLS[kind])[idx].mat == rec["mat"]


def query_counters(st, hits=None):
    """The counters a query reports; with `hits`, rng_draws is the sum of the per-ray draws (what rto_hit reports per ray)."""
    return st.node_visits, list(st.prim_tests), int(hits["rng_draws"].sum()) if hits is not None else st.rng_draws


def scene_bounds(desc):
    if F.ref_kind(desc.root) == F.RT_KIND_NODE:
        n = desc.nodes[F.ref_index(desc.root)]
        lo, hi = np.array(n.bmin[:]), np.array(n.bmax[:])
        if np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)):
            return lo, hi
    return np.full(3, -8.0), np.full(3, 8.0)


def unit_vectors(g, n):
    v = g.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def camera_rays(rt, cam, n, g, time=None):
    """Pinhole rays of the camera's view (get_ray without the lens), at random points of the image."""
    s, t = g.random(n), g.random(n)
    o = np.array(cam.origin[:])
    d = (np.array(cam.lower_left_corner[:]) + s[:, None] * np.array(cam.horizontal[:]) + t[:, None] * np.array(cam.vertical[:]) - o)
    return rt.query_rays(o, d, time=g.uniform(cam.time0, cam.time1, n) if time is None else time)


def bounce_rays(rt, hits, g, n):
    h = hits[hits["hit"] == 1][:n]
    d = h["normal"] + unit_vectors(g, len(h))
    return rt.query_rays(h["p"], d, time=g.random(len(h)))


def mixed_rays(rt, desc, cam, n, seed):
    """Camera rays, one bounce from their hits, and random rays through the scene's bounds, with random per-ray windows,
    times and RNG states (t_max = inf included)."""
    g = np.random.default_rng(seed)
    cam_r = camera_rays(rt, cam, n // 3, g)
    lo, hi = scene_bounds(desc)
    span = hi - lo
    rnd_o = lo - 0.25 * span + g.random((n // 3, 3)) * 1.5 * span
    rnd_r = rt.query_rays(rnd_o, unit_vectors(g, n // 3))
    first = np.concatenate([cam_r, rnd_r])
    return first, g


def randomise_windows(rays, g):
    n = len(rays)
    rays["time"] = g.random(n)
    rays["t_min"] = g.choice([0.001, 0.0, 1e-9, 0.5], n)
    tmax = g.choice([np.inf, 1e300, 0.0], n, p=[0.6, 0.2, 0.2])
    far = tmax == 0.0
    rays["t_max"] = np.where(far, rays["t_min"] + g.exponential(50.0, n), tmax)
    rays["rng_state"] = g.integers(0, 2**63, n, dtype=np.uint64)
    return rays
