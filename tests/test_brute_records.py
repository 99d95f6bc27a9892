"""The oracle's hit RECORD (rto_hit: p, normal, front_face, u, v, mat) and its textures (rto_texture_value) against the
BVH-free extended-precision reference of tests/brute_records.py, which shares no code with oracle/ or csrc/.
tests/test_brute_hits.py holds hit / miss, t and the leaf; this module holds what a hit produces from them, through movers and
FlipFace refs, and the texture value and albedo there. CPU only; tests/test_brute_records_gpu.py holds the device to the same
reference.

Where the reference renderer is not geometric the reference keeps its definitions (hittable/mod.rs, triangle.rs:65-72,
texture/mod.rs, perlin.rs); each such quirk has a known-answer test below with numbers worked out by hand."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import brute_hits as B
import brute_records as BR
import brute_scenes as S
import raytracer_2022_amd as rt
from raytracer_2022_amd import _ffi as F

mp.mp.dps = 40
KINDS = ("sphere", "moving_sphere", "rect", "box", "triangle", "ring")
MOVERS = {"none": (), "translate": ("T",), "rotate_y": ("R",), "zoom": ("Z",), "translate(rotate_y(zoom))": ("T", "R", "Z")}
FLIPS = ("leaf", "mover", "both")
OFFSET, RATE, SIN, COS = (0.7, -0.4, 1.1), 1.7, 0.8, 0.6            # (an angle of 53 degrees: the mixed-frame rule gives both flags)
ROOT_SCENES = ("every_kind", "cornell_box", "final_scene", "earth", "two_perlin_spheres", "wwscene")
NEW_CLASS_SHARE = 0.03


def to_mp(x):
    """A longdouble (or float) as an mpf, both halves."""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - B.LD(hi)))


# ---- 1. the reference against itself: mpmath at 40 digits ----------------------------------------------------------------------
def test_sphere_uv_against_mpmath():
    """300 points of the unit sphere, the pole and the seam among them: acos and atan2 of the longdouble libm to 1e-17."""
    g = np.random.default_rng(1)
    n = g.normal(size=(300, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[:6] = [[0, 1, 0], [0, -1, 0], [-1, 0, 0], [-1, 0, 1e-12], [-1, 0, -1e-12], [1e-9, -1, 0]]
    b = rt.DescBuilder()
    ref = b.sphere((0, 0, 0), 1.0, b.lambertian((0.5, 0.5, 0.5)))
    b.set_root(ref)
    sc = B.Scene(b.desc())
    rays = B._rays(3 * n, -n, 0.0, 0.001, np.inf, g)                  # radial rays: the hit point is n itself, at t = 2
    ans = B.solve(sc, rays["origin"], rays["direction"], 0.0, 0.001, np.inf)
    R = BR.records(sc, rays, ans)
    assert ans.hit.all()
    for i in range(len(n)):
        x, y, z = (to_mp(v) for v in R.p[i])                      # (centre 0, radius 1: the outward normal is the reference's own p)
        u = (mp.atan2(-z, x) + mp.pi) / (2 * mp.pi)
        v = mp.acos(max(-1, min(1, -y))) / mp.pi
        du = abs(to_mp(R.u[i]) - u)                              # (the seam: mpmath has no -0.0, atan2(-0.0, -1) = -pi is u = 0 there)
        assert min(du, abs(1 - du)) < mp.mpf("1e-17") and abs(to_mp(R.v[i]) - v) < mp.mpf("1e-17"), i
    assert R.pole[:2].all() and R.pole[5] and not R.pole[6:].any()


def mp_rotate_record(d, n_leaf, p_leaf, s, c):
    """RotateY::hit's way out (mod.rs:247-260) on a leaf record with a face normal: → (p, normal, front)."""
    rd = [c * d[0] - s * d[2], d[1], s * d[0] + c * d[2]]
    p = [c * p_leaf[0] + s * p_leaf[2], p_leaf[1], -s * p_leaf[0] + c * p_leaf[2]]
    n = [c * n_leaf[0] + s * n_leaf[2], n_leaf[1], -s * n_leaf[0] + c * n_leaf[2]]
    front = sum(a * b for a, b in zip(rd, n)) < 0
    return p, (n if front else [-x for x in n]), front


def test_rotate_y_record_against_mpmath():
    """A rect under a RotateY, 300 rays at 12 angles: p, normal and the flag as mod.rs:235-264 gives them, in 40 digits."""
    g = np.random.default_rng(2)
    seen = set()
    for angle in np.linspace(-170, 170, 12):
        s, c = float(np.sin(np.radians(angle))), float(np.cos(np.radians(angle)))
        b = rt.DescBuilder()
        ref = b.rotate_y(b.rect(F.RT_RECT_XY, -2.0, 2.0, -2.0, 2.0, 0.25, b.lambertian((0.5, 0.5, 0.5))), s, c)
        b.set_root(ref)
        sc = B.Scene(b.desc())
        rays = B._rays(g.normal(size=(25, 3)) * 2, g.normal(size=(25, 3)), 0.0, 0.001, np.inf, g)
        ans = B.solve(sc, rays["origin"], rays["direction"], 0.0, 0.001, np.inf)
        R = BR.records(sc, rays, ans)
        S_, C_ = mp.mpf(s), mp.mpf(c)
        for i in np.flatnonzero(ans.hit & ~ans.ambiguous & ~R.face_ambiguous):
            o, d = [mp.mpf(float(x)) for x in rays["origin"][i]], [mp.mpf(float(x)) for x in rays["direction"][i]]
            ro = [C_ * o[0] - S_ * o[2], o[1], S_ * o[0] + C_ * o[2]]
            rd = [C_ * d[0] - S_ * d[2], d[1], S_ * d[0] + C_ * d[2]]
            t = (mp.mpf(0.25) - ro[2]) / rd[2]
            pl = [a + t * b_ for a, b_ in zip(ro, rd)]
            nl = [0, 0, 1] if rd[2] < 0 else [0, 0, -1]
            p, nrm, front = mp_rotate_record(d, nl, pl, S_, C_)
            assert bool(R.front[i]) == front
            assert max(abs(to_mp(R.p[i][k]) - p[k]) for k in range(3)) < mp.mpf("1e-16") * (1 + abs(t))
            assert max(abs(to_mp(R.normal[i][k]) - nrm[k]) for k in range(3)) < mp.mpf("1e-17")
            seen.add(front)
    assert seen == {True, False}


def mp_noise(tab, p):
    fl = [mp.floor(x) for x in p]
    f = [x - y for x, y in zip(p, fl)]
    f = [x * x * (3 - 2 * x) for x in f]
    ff = [x * x * (3 - 2 * x) for x in f]
    ijk = [int(x) for x in fl]
    acc = mp.mpf(0)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                gv = tab["randvec"][int(tab["perm_x"][(ijk[0] + di) & 255]) ^ int(tab["perm_y"][(ijk[1] + dj) & 255]) ^ int(tab["perm_z"][(ijk[2] + dk) & 255])]
                w = sum(mp.mpf(float(gv[k])) * (f[k] - (di, dj, dk)[k]) for k in range(3))
                for k, dd in enumerate((di, dj, dk)):
                    w *= ff[k] if dd else 1 - ff[k]
                acc += w
    return acc


def mp_turb(tab, p, depth=7):
    acc, w = mp.mpf(0), mp.mpf(1)
    for _ in range(depth):
        acc += w * mp_noise(tab, p)
        w /= 2
        p = [2 * x for x in p]
    return abs(acc)


@pytest.mark.parametrize("name", ["two_perlin_spheres", "final_scene"])
def test_noise_and_turb_against_mpmath(name):
    """Perlin::noise and turb(p, 7) with the scene's own tables, 200 points with negative and large coordinates."""
    d, _ = S.make(name)
    sh = BR.Shading(d)
    tab = sh.pools["perlins"][0]
    g = np.random.default_rng(3)
    p = g.normal(size=(200, 3)) * np.repeat([1.0, 30.0, 1e3, 1e5], 50)[:, None]
    p[:4] = [[-0.5, -1.0, -255.5], [256.0, -256.0, 0.0], [-1e-9, 1e-9, 511.999], [3.0, 4.0, 5.0]]
    got_n, got_t = BR.perlin_noise(tab, B.LD(1) * p), BR.perlin_turb(tab, B.LD(1) * p)
    for i in range(len(p)):
        q = [mp.mpf(float(x)) for x in p[i]]
        assert abs(to_mp(got_n[i]) - mp_noise(tab, q)) < mp.mpf("2e-17"), (i, p[i])
        assert abs(to_mp(got_t[i]) - mp_turb(tab, q)) < mp.mpf("2e-17"), (i, p[i])


def test_noise_gradient_bound_against_finite_differences():
    """NOISE_G bounds |grad noise| of the reference's own noise: central differences at 20000 points never exceed it, and
    come within a factor of 8 of it (the bound is not vacuous: the tolerance it gives is within a decade of the slope)."""
    d, _ = S.make("two_perlin_spheres")
    tab = BR.Shading(d).pools["perlins"][0]
    g = np.random.default_rng(4)
    p = B.LD(1) * g.uniform(-40, 40, (20000, 3))
    h = B.LD(1e-6)
    grad = np.stack([(BR.perlin_noise(tab, p + h * e) - BR.perlin_noise(tab, p - h * e)) / (2 * h) for e in np.eye(3)], axis=1)
    worst = float(np.sqrt((grad ** 2).sum(1)).max())
    print("largest |grad noise| by finite differences: %.3f; NOISE_G = %.1f" % (worst, BR.NOISE_G))
    assert BR.NOISE_G / 8 < worst <= BR.NOISE_G


def test_image_indexing_against_mpmath():
    """Texel choice of 400 (u, v) on an 8 x 4 image: clamp, truncate, clamp to W - 1 / H - 1, row 0 at the bottom."""
    b = rt.DescBuilder()
    img = (np.arange(8 * 4 * 3, dtype=np.uint8).reshape(4, 8, 3) * 7) % 251
    b.set_root(b.sphere((0, 0, 0), 1.0, b.lambertian(tex=b.image(img))))
    sh = BR.Shading(b.desc())
    tex = b.pools["materials"][-1].tex
    g = np.random.default_rng(5)
    uv = g.uniform(-0.3, 1.3, (400, 2))
    uv[:6] = [[0, 0], [1, 1], [0.125, 0.25], [0.9999999, 0.9999999], [-5, 7], [0.5, 0.75]]
    val = BR.texture_value_ref(sh, tex, uv[:, 0], uv[:, 1], np.zeros((400, 3)))
    for k in range(400):
        u, v = (min(mp.mpf(1), max(mp.mpf(0), mp.mpf(float(x)))) for x in uv[k])
        i, j = min(int(mp.floor(u * 8)), 7), min(int(mp.floor(v * 4)), 3)
        want = [mp.mpf(int(c)) * mp.mpf(1.0 / 255.999) for c in img[j, i]]
        assert max(abs(to_mp(val.value[k][c]) - want[c]) for c in range(3)) < mp.mpf("1e-18"), (k, uv[k])
    assert val.edge[[2, 5]].all() and not val.edge[[0, 1, 4]].any() and val.seam[[0, 1]].all()


# ---- 2. leaf by leaf ---------------------------------------------------------------------------------------------------------------
def leaf_scene(kind, movers, flip, g):
    """(desc, outer ref) of one leaf of `kind`, size about 1, under `movers` (outermost first); the FlipFace bit on the leaf, on
    every mover, or on both."""
    b = rt.DescBuilder()
    m = b.lambertian((0.5, 0.5, 0.5))
    c = g.uniform(-0.3, 0.3, 3)
    fl = flip in ("leaf", "both")
    if kind == "sphere":
        ref = b.sphere(tuple(c), float(g.uniform(0.5, 1.0)), m, flip=fl)
    elif kind == "moving_sphere":
        ref = b.moving_sphere(tuple(c), tuple(c + g.uniform(-0.5, 0.5, 3)), 0.0, 1.0, float(g.uniform(0.5, 1.0)), m, flip=fl)
    elif kind == "rect":
        ref = b.rect(int(g.integers(0, 3)), c[0] - 0.8, c[0] + 0.6, c[1] - 0.5, c[1] + 0.9, float(c[2]), m, flip=fl)
    elif kind == "box":
        ref = b.box(tuple(c - g.uniform(0.3, 0.8, 3)), tuple(c + g.uniform(0.3, 0.8, 3)), m, flip=fl)
    elif kind == "triangle":
        ref = b.triangle(tuple(c + (-1.2, -0.9, g.uniform(-0.4, 0.4))), tuple(c + (1.1, -0.8, g.uniform(-0.4, 0.4))),
                         tuple(c + (0.1, 1.2, g.uniform(-0.4, 0.4))), m, flip=fl)
    else:
        ref = b.ring(float(g.uniform(0.5, 0.7)), float(g.uniform(0.3, 0.45)), m, flip=fl)
    fm = flip in ("mover", "both")
    for k in reversed(movers):
        ref = {"T": lambda r: b.translate(r, OFFSET, flip=fm), "R": lambda r: b.rotate_y(r, SIN, COS, flip=fm),
               "Z": lambda r: b.zoom(r, RATE, flip=fm)}[k](ref)
    b.set_root(ref)
    d = b.desc()
    d._builder = b
    return d, ref


def leaf_rays(g, movers, n=240):
    """Rays through the object's extent in the world frame: a quarter parallel to an axis (one or two zero components), a
    quarter from inside, windows {0.001, 0.5} x {inf, finite}."""
    chain = tuple({"T": (B.K_TRANSLATE, OFFSET), "R": (B.K_ROTATE_Y, (SIN, COS, 0.0)), "Z": (B.K_ZOOM, (RATE, 0.0, 0.0))}[k] for k in movers)
    centre = np.asarray(B.point_out(chain, np.zeros((1, 3), dtype=B.LD))[0], dtype=np.float64)
    scale = RATE if "Z" in movers else 1.0
    o = g.normal(size=(n, 3)) * 3.0 * scale
    d = (g.uniform(-0.6, 0.6, (n, 3)) * scale - o) * g.uniform(0.3, 3.0, (n, 1))
    k = n // 4
    zero = g.integers(0, 3, k)
    d[np.arange(k), zero] = 0.0
    two = np.flatnonzero(np.arange(k) % 2 == 0)
    d[two, (zero[two] + 1) % 3] = 0.0
    o[:k] = g.uniform(-0.6, 0.6, (k, 3)) * scale - 2.0 * d[:k] / np.abs(d[:k]).max(1, keepdims=True) * scale
    o[k:2 * k] = g.uniform(-0.25, 0.25, (k, 3)) * scale
    lo = g.choice([0.001, 0.5], n)
    hi = np.where(g.random(n) < 0.5, np.inf, lo + g.uniform(0.2, 1.5, n))
    return B._rays(o + centre, d, g.uniform(-0.5, 1.5, n), lo, hi, g)


LEAF_CASES = [(k, m, f) for k in KINDS for m in MOVERS for f in (FLIPS if MOVERS[m] else ("none", "leaf"))]


@pytest.mark.parametrize("kind,mover,flip", LEAF_CASES, ids=["%s-%s-%s" % c for c in LEAF_CASES])
def test_leaf_by_leaf(O, kind, mover, flip):
    g = np.random.default_rng(2000 + KINDS.index(kind) * 10 + list(MOVERS).index(mover))
    d, ref = leaf_scene(kind, MOVERS[mover], flip, g)
    sc = B.Scene(d)
    (path,) = sc.paths
    assert path.flips == tuple([flip in ("mover", "both")] * len(MOVERS[mover]) + [flip in ("leaf", "both")])
    assert path.flip == (sum(path.flips) % 2 == 1)
    rays = leaf_rays(g, MOVERS[mover])
    ans = B.solve(sc, rays["origin"], rays["direction"], rays["time"], rays["t_min"], rays["t_max"])
    R = BR.records(sc, rays, ans)
    left_out = sum(int(v.sum()) for v in BR.new_classes(sc, ans, R).values())
    assert left_out <= NEW_CLASS_SHARE * len(rays), left_out                               # (before any result is looked at)
    got = S.oracle_records(O, d, rays, ref)
    ta = BR.compare(sc, rays, ans, R, got)
    print(ta.line("%s/%s/%s" % (kind, mover, flip), "leaf", "oracle"))
    assert not ta.failures, ta.failures[:5]
    assert ta.worst_ratio <= 1.0
    assert ta.compared >= 30
    held = ans.hit & ~ans.ambiguous & ~ans.tie & ~R.face_ambiguous & ~ans.ring_parallel
    if "R" in MOVERS[mover] and kind != "ring":
        assert len(set(R.front[held])) == 2                      # both flag values behind a RotateY (a ring's +y is the rotation's axis)


# ---- 3. the root of the named scenes -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(name):
        if name not in cache:
            d, cam = S.mover_records() if name == "mover_records" else S.make(name)
            cache[name] = (d, cam, B.Scene(d), BR.Shading(d))
        return cache[name]
    return get


def root_check(O, d, cam, sc, sh, seed, name):
    """Every family through rto_hit at the root: the record, and the feature header's albedo by the oracle's composition
    against albedo_ref at the reference's own record → {family: RecordTally}."""
    out = {}
    for family, rays in S.families(B, sc, cam, seed).items():
        ans = B.solve(sc, rays["origin"], rays["direction"], rays["time"], rays["t_min"], rays["t_max"])
        R = BR.records(sc, rays, ans)
        want = BR.albedo_ref(sh, R.mat, R.front, R.u, R.v, R.p)
        classes = BR.new_classes(sc, ans, R, want)
        left_out = np.zeros(len(rays), bool)
        for v in classes.values():
            left_out |= v
        assert left_out.sum() <= NEW_CLASS_SHARE * len(rays), (name, family, {k: int(v.sum()) for k, v in classes.items()})
        got = S.oracle_records(O, d, rays)
        ta = BR.compare(sc, rays, ans, R, got, got_value=S.oracle_albedo(O, d, got), want_value=albedo_mask(want, R))
        print(ta.line(name, family, "oracle"))
        out[family] = ta
    return out


def albedo_mask(want, R):
    """A light's albedo depends on the face: leave the value out where the face is ambiguous."""
    want.skip = want.skip | R.face_ambiguous
    return want


@pytest.mark.parametrize("name", ROOT_SCENES + ("mover_records",))
def test_root_records_against_brute_force(O, scenes, name):
    d, cam, sc, sh = scenes(name)
    tallies = root_check(O, d, cam, sc, sh, 700 + len(name), name)
    for family, ta in tallies.items():
        assert not ta.failures, (name, family, ta.failures[:5])
        assert ta.worst_ratio <= 1.0, (name, family, ta.worst)
    assert sum(ta.compared for ta in tallies.values()) >= (150 if name == "wwscene" else 400)


def test_mover_records_floors(scenes):
    """The scene is built so that the reference alone gives enough winners of every sort (no oracle, no device)."""
    d, cam, sc, sh = scenes("mover_records")
    assert not sc.media and not any(p.nodes for p in sc.paths) and all(p.movers for p in sc.paths)
    moved = rotated_back = flip_below = 0
    for family, rays in S.families(B, sc, cam, 321).items():
        ans = B.solve(sc, rays["origin"], rays["direction"], rays["time"], rays["t_min"], rays["t_max"])
        R = BR.records(sc, rays, ans)
        c1, c2, c3, amb = B.classify(sc, ans)
        assert not c1.any() and not c2.any()
        held = ans.hit & ~(c3 | amb | ans.tie) & ~R.face_ambiguous
        moved += int((held & R.moved).sum())
        rotated_back += int((held & R.rotated & ~R.front).sum())
        flip_below += int((held & R.flip_below).sum())
    print("mover_records: %d winners under a mover, %d with front_face 0 behind a RotateY, %d with a flip below a mover" % (moved, rotated_back, flip_below))
    assert moved >= 500 and rotated_back >= 100 and flip_below >= 100


# ---- 4. textures ------------------------------------------------------------------------------------------------------------------
def texture_points(g, n):
    """(u, v, p): u, v in [-0.5, 1.5] and exactly 0 and 1; p of size 1, 30, 1e3 and 1e5 of either sign, lattice points among them."""
    u, v = g.uniform(-0.5, 1.5, n), g.uniform(-0.5, 1.5, n)
    u[:4], v[:4] = [0, 1, 0.5, 1], [0, 1, 1, 0.5]
    p = g.normal(size=(n, 3)) * np.resize([1.0, 1.0, 30.0, 1e3, 1e5], n)[:, None]
    p[:3] = [[0, 0, 0], [-1, 2, -3], [255, -256, 0.5]]
    return u, v, p


@pytest.mark.parametrize("name", ["final_scene", "earth", "two_perlin_spheres", "every_kind", "mover_records"])
def test_texture_value_against_reference(O, scenes, name):
    """rto_texture_value against texture_value_ref on 10^4 points per texture of the scene."""
    d, _, _, sh = scenes(name)
    L = O.lib()
    kinds = {}
    for tex in range(d.n_textures):
        u, v, p = texture_points(np.random.default_rng(50 + tex), 10000)
        want = BR.texture_value_ref(sh, tex, u, v, p)
        assert want.edge.sum() <= NEW_CLASS_SHARE * len(u), (name, tex, int(want.edge.sum()))
        got = np.zeros((len(u), 3))
        pc, out = np.ascontiguousarray(p), (C.c_double * 3)()
        for i in range(len(u)):
            assert L.rto_texture_value(C.byref(d), tex, u[i], v[i], pc[i].ctypes.data_as(C.POINTER(C.c_double)), out) == 0
            got[i] = out[:]
        ratio = BR._ratio(np.abs(B.LD(1) * got - want.value).max(1), want.tolerance(0.0))
        ok = ~want.edge
        bad = np.flatnonzero(ok & (ratio > 1))
        kind = int(sh.pools["textures"][tex]["kind"])
        kinds[kind] = max(kinds.get(kind, 0.0), float(ratio[ok].max()))
        assert len(bad) == 0, (name, tex, kind, [(int(i), u[i], v[i], p[i].tolist(), got[i].tolist(), [float(x) for x in want.value[i]]) for i in bad[:3]])
    print("%s: %d textures, worst error / tolerance by kind %s" % (name, d.n_textures, {k: "%.2e" % w for k, w in sorted(kinds.items())}))


# ---- 5. the quirks, pinned by name -------------------------------------------------------------------------------------------------
def one(O, d, ref, o, dr, **kw):
    rec = O.hit(d, ref, o, dr, **kw)
    sc = B.Scene(d)
    rays = B._rays([o], [dr], kw.get("tm", 0.0), 0.001, np.inf, np.random.default_rng(0))
    ans = B.solve(sc, rays["origin"], rays["direction"], rays["time"], 0.001, np.inf)
    return rec, BR.records(sc, rays, ans), ans


def test_a_flip_under_a_translate_is_erased(O):
    """Translate::hit calls set_face_normal on the record's face normal (mod.rs:169): the flag comes out true whatever a
    FlipFace below made of it; a FlipFace ON the Translate still turns it over. The same for Zoom (mod.rs:325)."""
    for mover in ("translate", "zoom"):
        for leaf_flip, mover_flip, want in ((False, False, 1), (True, False, 1), (False, True, 0), (True, True, 0)):
            b = rt.DescBuilder()
            s = b.sphere((0, 0, -3), 1.0, b.lambertian((0.5, 0.5, 0.5)), flip=leaf_flip)
            ref = b.translate(s, (0, 0, 0.5), flip=mover_flip) if mover == "translate" else b.zoom(s, 1.0, flip=mover_flip)
            b.set_root(ref)
            rec, R, ans = one(O, b.desc(), ref, (0, 0, 0), (0, 0, -1))
            assert rec.hit == 1 and rec.front_face == want and bool(R.front[0]) == bool(want), (mover, leaf_flip, mover_flip)
            assert list(rec.normal) == [0.0, 0.0, 1.0] and [float(x) for x in R.normal[0]] == [0.0, 0.0, 1.0]
            assert O.hit(b.desc(), s, (0, 0, 0), (0, 0, -1)).front_face == (0 if leaf_flip else 1)          # (the leaf alone keeps its flip)


def test_rotate_y_gives_both_flag_values_and_a_normal_along_the_ray(O):
    """RotateY::hit tests the OBJECT-frame direction against the PARENT-frame normal (mod.rs:258). sin = 0.8, cos = 0.6, a YZ
    rect at x = 5 seen from the origin, by hand:
      d = (0, 0, -1): d' = (0.8, 0, -0.6); leaf back face, n = (-1, 0, 0); out (-0.6, 0, 0.8); d' . n = -0.96: FRONT, normal kept;
      d = (1, 0, 0):  d' = (0.6, 0, 0.8);  leaf back face, n = (-1, 0, 0); out (-0.6, 0, 0.8); d' . n = +0.28: back, normal
                      negated to (0.6, 0, -0.8) — which points ALONG the world ray (d . normal = +0.6)."""
    b = rt.DescBuilder()
    ref = b.rotate_y(b.rect(F.RT_RECT_YZ, -100, 100, -100, 100, 5.0, b.lambertian((0.5, 0.5, 0.5))), 0.8, 0.6)
    b.set_root(ref)
    d = b.desc()
    for dr, front, normal in (((0, 0, -1), 1, (-0.6, 0.0, 0.8)), ((1, 0, 0), 0, (0.6, 0.0, -0.8))):
        rec, R, ans = one(O, d, ref, (0, 0, 0), dr)
        assert rec.hit == 1 and rec.front_face == front and bool(R.front[0]) == bool(front)
        assert np.allclose(rec.normal[:], normal, atol=1e-15) and np.allclose(np.asarray(R.normal[0], dtype=float), normal, atol=1e-15)
    # a Translate above it takes a real decision on that normal: d . normal = +0.6 > 0 turns it back, flag 0
    top = b.translate(ref, (0, 0, 0))
    b.set_root(top)
    rec, R, ans = one(O, b.desc(), top, (0, 0, 0), (1, 0, 0))
    assert rec.front_face == 0 and not R.front[0] and np.allclose(rec.normal[:], (-0.6, 0.0, 0.8), atol=1e-15)
    assert np.allclose(np.asarray(R.normal[0], dtype=float), (-0.6, 0.0, 0.8), atol=1e-15)


def test_a_triangle_in_a_plane_x_const_has_no_finite_uv(O):
    """beta and gamma are barycentrics of the xy-projection (triangle.rs:65-72): a triangle in x = 1 projects onto a segment,
    a1 b2 - b1 a2 = 0, and u, v come out inf or NaN. The reference names the class and compares p, normal and the flag."""
    b = rt.DescBuilder()
    ref = b.triangle((1, -1, -1), (1, 1, -1), (1, 0, 1), b.lambertian((0.5, 0.5, 0.5)))
    b.set_root(ref)
    rec, R, ans = one(O, b.desc(), ref, (0, 0.1, 0.2), (1, 0, 0))
    assert rec.hit == 1 and rec.t == 1.0 and not np.isfinite(rec.u) and not np.isfinite(rec.v)
    assert ans.hit[0] and R.uv_degenerate[0] and not R.face_ambiguous[0]
    rays = B._rays([(0, 0.1, 0.2)], [(1, 0, 0)], 0.0, 0.001, np.inf, np.random.default_rng(0))
    got = S.oracle_records(O, b.desc(), rays)
    ta = BR.compare(B.Scene(b.desc()), rays, ans, R, got)
    assert ta.compared == 1 and not ta.failures and ta.classes["uv-degenerate"] == 1


def test_constant_records(O):
    """A Ring's u, v are 0, 0 (ring.rs:49); every face of a box is a plain rect with a +axis outward normal (boxes.rs:24-66):
    entering through the p0 side is a BACK face; a medium's record is (1, 0, 0), flag true (constantmedium.rs:66-74)."""
    b = rt.DescBuilder()
    m = b.lambertian((0.5, 0.5, 0.5))
    ring, box = b.ring(1.0, 0.5, m), b.box((-1, -1, -1), (1, 1, 1), m)
    fog = b.medium(b.sphere((0, 0, 0), 1.0, b.dielectric(1.5)), 1e9, b.isotropic((0.5, 0.5, 0.5)))
    b.set_root(ring)
    d = b.desc()
    rec, R, _ = one(O, d, ring, (0.9, 2, 0.1), (0, -1, 0))
    assert (rec.u, rec.v, R.u[0], R.v[0]) == (0, 0, 0, 0) and list(rec.normal) == [0, 1, 0] and rec.front_face == 1
    b.set_root(box)
    rec, R, _ = one(O, b.desc(), box, (-3, 0.2, 0.1), (1, 0, 0))
    assert rec.front_face == 0 and not R.front[0] and list(rec.normal) == [-1, 0, 0] and [float(x) for x in R.normal[0]] == [-1, 0, 0]
    assert (rec.u, rec.v) == (0.6, 0.55) == (float(R.u[0]), float(R.v[0]))
    rec = O.hit(b.desc(), fog, (-3, 0, 0), (1, 0, 0))
    assert rec.hit == 1 and list(rec.normal) == [1, 0, 0] and rec.front_face == 1 and (rec.u, rec.v) == (0, 0)


# ---- 6. the test must be able to fail -------------------------------------------------------------------------------------------------
def test_a_negated_sine_is_flagged(O):
    """A sphere centred on the rotation's axis: with the RotateY's sine negated every ray still hits at the same t and p (which
    is why brute_hits alone cannot see it), but u turns by twice the angle and the mixed-frame flag changes."""
    g = np.random.default_rng(9)
    b = rt.DescBuilder()
    ref = b.rotate_y(b.sphere((0, 0.2, 0), 0.9, b.lambertian((0.5, 0.5, 0.5))), SIN, COS)
    b.set_root(ref)
    d = b.desc()
    rays = leaf_rays(g, ("R",))
    got = S.oracle_records(O, d, rays, ref)
    wrong = F.rt_scene_desc.from_buffer_copy(d)
    xf = (F.rt_xform * 1)(F.rt_xform(kind=F.RT_KIND_ROTATE_Y, child=d.xforms[0].child, p=F.d3(-SIN, COS, 0.0)))
    wrong.xforms = C.cast(xf, C.POINTER(F.rt_xform))
    for desc, fails in ((d, False), (wrong, True)):
        sc = B.Scene(desc)
        ans = B.solve(sc, rays["origin"], rays["direction"], rays["time"], rays["t_min"], rays["t_max"])
        ta_t, _ = B.compare(sc, rays, got["hit"], got["t"], got["rng_draws"], ans=ans)
        assert not ta_t.failures                                   # hit / miss and t agree either way
        ta = BR.compare(sc, rays, ans, BR.records(sc, rays, ans), got)
        what = {w.split(":")[0] for _, w in ta.failures}
        print("sine %s: %d failures %s" % ("negated" if fails else "as built", len(ta.failures), sorted(what)))
        assert (what >= {"u", "front_face", "normal"}) if fails else not ta.failures


@pytest.mark.parametrize("name,edit,kind", [("earth", "rows", BR.TEX_IMAGE), ("two_perlin_spheres", "scale", BR.TEX_NOISE)])
def test_a_wrong_texture_table_is_flagged(O, scenes, name, edit, kind):
    """The reference built from pools that differ from the oracle's — an image's rows top-down, a noise scale 1 % off — is told
    apart from it by the albedo comparison at the root, and by nothing else."""
    d, cam, sc, _ = scenes(name)

    def spoil(pools):
        if edit == "rows":
            im = pools["images"][0]
            w, h, off = int(im["width"]), int(im["height"]), int(im["offset"])
            pools["image_data"][off:off + 3 * w * h] = pools["image_data"][off:off + 3 * w * h].reshape(h, w, 3)[::-1].ravel()
        else:
            t = pools["textures"]
            t["scale"][np.flatnonzero(t["kind"] == BR.TEX_NOISE)[0]] *= 1.01
    tallies = root_check(O, d, cam, sc, BR.Shading(d, edit=spoil), 700 + len(name), name)
    what = {w.split(":")[0] for ta in tallies.values() for _, w in ta.failures}
    flagged = sum(len(ta.failures) for ta in tallies.values())
    print("%s with %s spoiled: %d rays flagged, fields %s" % (name, edit, flagged, sorted(what)))
    assert what == {"texture"} and flagged >= 20
