"""The probe stage and the cases of tests/test_brute_paths.py, its GPU module and tools/brute_paths_report.py.

To see a scattered direction from outside the kernel, every stage sits inside a cube of six emissive rects, DiffuseLight on an
image texture each, flipped where needed so that the inside is the front face, and none of them in the light list. Face f
carries its own 256 x 256 image whose texel (i, j) has the bytes (i, j, 16 + 40 f): a neighbouring texel or face is always
another colour and the blue channel always shows the weight. With ray_color at depth 2 a sample is emitted_1 + weight x
texel(where the scattered ray leaves) — or weight x a stage light's own solid colour — and tests/brute_paths.py predicts that
value outright; nothing is decoded from a result. The images are generated here, not stored.

A case: 2000 first rays from a fixed set of origins aimed at the stage object, 2 samples a ray (sample s of a ray draws from
path_key(rng_state, 0, 0, s)), a list root (no BVH, so no pruning enters), the depth, and the arms it is named for, each of
which must hold FLOOR compared samples by the reference alone. reference(name) computes a case's paths once per process."""
import numpy as np

import raytracer_2022_amd as rt

import brute_paths as BP

HALF, TEXELS = 4.0, 256
N_RAYS, SPP, FLOOR = 2000, 2, 100
BACKGROUND = (0.25, 0.5, 0.75)
LEFT_OUT_SHARE, COMPARED_SHARE = 0.03, 0.90
XY, XZ, YZ = 0, 1, 2                                       # rt_rect_axis
FLIP = 0x80000000


def face_image(f):
    i, j = np.meshgrid(np.arange(TEXELS), np.arange(TEXELS))
    return np.stack([i, j, np.full_like(i, 16 + 40 * f)], axis=-1).astype(np.uint8)             # [j, i]: row j is v, column i is u


def cube(b):
    """The six faces → refs. A rect's outward normal is +axis: the face at -HALF is seen from inside against it (front), the
    face at +HALF along it (back), so that one is flipped."""
    refs = []
    for a, axis in enumerate((YZ, XZ, XY)):
        for side, k in enumerate((-HALF, HALF)):
            m = b.diffuse_light(tex=b.image(face_image(2 * a + side)))
            refs.append(b.rect(axis, -HALF, HALF, -HALF, HALF, k, m, flip=bool(side)))
    return refs


def _aimed(g, origins, targets):
    o = np.asarray(origins, dtype=np.float64)[g.integers(0, len(origins), len(targets))]
    return o, targets - o


def _in_ball(g, n, radius):
    v = g.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * radius * g.random((n, 1)) ** (1 / 3)


ABOVE = [(1.0, 2.0, 0.5), (-1.2, 1.5, 0.8), (0.3, 2.4, -1.1), (-0.6, 1.8, -0.4)]
ROUND_ABOUT = [(2.5, 0.7, 0.4), (-2.2, 1.2, -1.0), (0.5, 2.0, 2.0), (-0.8, -2.3, -1.1)]
INSIDE = [(0.8, 0.0, 0.0), (-0.8, 0.0, 0.0), (0.0, 0.8, 0.0), (0.0, 0.0, -0.8)]
LOW = [(-2.2, 0.35, 0.0), (2.2, 0.35, 0.0), (0.0, 0.35, -2.2), (0.0, 0.35, 2.2)]
LIGHT = (5.0, 4.0, 3.0)


def _lights(b, which):
    """Stage lights above a floor at y = 0 → (world refs, light-list refs). The XZ and XY rects are seen from their back
    and flipped in the world; the list holds the plain ref, as the reference renderer's own light lists do."""
    world, listed = [], []
    for w in which:
        if w == "xz":
            r = b.rect(XZ, -0.5, 0.5, -0.4, 0.8, 3.0, b.diffuse_light(LIGHT))       # (no square: the area is not that of another axis pair)
            world.append(r | FLIP); listed.append(r)
        elif w == "xy":
            r = b.rect(XY, -0.5, 0.5, 0.5, 1.7, 2.5, b.diffuse_light((3.0, 5.0, 4.0)))
            world.append(r | FLIP); listed.append(r)
        elif w == "yz":
            r = b.rect(YZ, 0.5, 1.5, -0.5, 0.9, -2.5, b.diffuse_light((4.0, 3.0, 5.0)))
            world.append(r); listed.append(r)
        elif w == "sphere":
            r = b.sphere((0.5, 2.5, -0.5), 0.4, b.diffuse_light((6.0, 5.0, 4.0)))
            world.append(r); listed.append(r)
        elif w == "flipped":                               # a flipped entry of the list: the trait default (1, 0, 0), pdf_value 0
            r = b.rect(XZ, -1.0, -0.2, -1.0, -0.2, 3.2, b.diffuse_light((2.0, 2.0, 6.0)))
            world.append(r | FLIP); listed.append(r | FLIP)
    return world, listed


def _floor(which, arms, yz=0):
    def build(g):
        b = rt.DescBuilder()
        m = b.lambertian((0.7, 0.6, 0.5))
        if yz:                                               # a floor whose normal is +-x: the other Onb branch
            floor = b.rect(YZ, -1.5, 1.5, -1.5, 1.5, 0.0, m)
            r = b.rect(YZ, -0.5, 0.5, -0.4, 0.8, 3.0 * yz, b.diffuse_light(LIGHT))
            world, listed = [r | FLIP if yz > 0 else r], [r]
            if which:                                        # seen from -x the default direction (1, 0, 0) is below the horizon: pdf_val 0
                s = b.sphere((-2.5, 0.5, -0.5), 0.4, b.diffuse_light((6.0, 5.0, 4.0)))
                f = b.rect(YZ, -1.0, -0.2, -1.0, -0.2, -3.2, b.diffuse_light((2.0, 2.0, 6.0)))
                world, listed = world + [s, f], listed + [s, f | FLIP]
            pts = np.stack([np.zeros(N_RAYS), g.uniform(-1.4, 1.4, N_RAYS), g.uniform(-1.4, 1.4, N_RAYS)], axis=1)
            origins = [(y * yz, x, z) for x, y, z in ABOVE]
        else:
            floor = b.rect(XZ, -1.5, 1.5, -1.5, 1.5, 0.0, m)
            world, listed = _lights(b, which)
            pts = np.stack([g.uniform(-1.4, 1.4, N_RAYS), np.zeros(N_RAYS), g.uniform(-1.4, 1.4, N_RAYS)], axis=1)
            origins = ABOVE
        for r in listed:
            b.light(r)
        b.set_root(b.list([floor] + world + cube(b)))
        return b, _aimed(g, origins, pts)
    return build, 2, arms


def _ball(material, depth, arms, origins=ROUND_ABOUT, lights=("xz",)):
    def build(g):
        b = rt.DescBuilder()
        s = b.sphere((0.0, 0.0, 0.0), 1.0, material(b))
        world, listed = _lights(b, lights)
        for r in listed:
            b.light(r)
        b.set_root(b.list([s] + world + cube(b)))
        if origins is INSIDE:                                # rays born inside, in every direction: half of them meet the
            o = np.asarray(INSIDE)[g.integers(0, 4, N_RAYS)]  # surface past the critical angle
            return b, (o, _in_ball(g, N_RAYS, 1.0))
        return b, _aimed(g, origins, _in_ball(g, N_RAYS, 0.9))
    return build, depth, arms


def _pane(g):
    b = rt.DescBuilder()
    pane = b.rect(XZ, -2.0, 2.0, -2.0, 2.0, 0.0, b.dielectric(1.5))
    b.set_root(b.list([pane] + cube(b)))
    pts = _in_ball(g, N_RAYS, 0.4)
    pts[:, 1] = 0.0
    return b, _aimed(g, LOW, pts)                          # 80 degrees off the normal: Schlick's reflectance is about 0.39


def _moved_box(g):
    b = rt.DescBuilder()
    box = b.translate(b.rotate_y(b.box((-0.6, 0.0, -0.6), (0.6, 1.2, 0.6), b.lambertian((0.6, 0.7, 0.5))), 0.6, 0.8), (0.2, -0.5, 0.1))
    world, listed = _lights(b, ("xz",))
    b.light(listed[0])
    b.set_root(b.list([box] + world + cube(b)))
    return b, _aimed(g, ROUND_ABOUT, _in_ball(g, N_RAYS, 0.5) + (0.2, 0.1, 0.1))


def _fog(g):
    """One medium in a sphere boundary, first in the list: half the rays through the chord, half born inside. Density 2 on
    chords up to 2.4 long: well over half of the samples that cross it scatter."""
    b = rt.DescBuilder()
    fog = b.medium(b.sphere((0.0, 0.0, 0.0), 1.2, b.dielectric(1.5)), 2.0, b.isotropic((0.8, 0.7, 0.6)))
    b.set_root(b.list([fog] + cube(b)))
    h = N_RAYS // 2
    o1, d1 = _aimed(g, ROUND_ABOUT, _in_ball(g, h, 1.0))
    o2 = np.asarray(INSIDE)[g.integers(0, 4, N_RAYS - h)]
    return b, (np.concatenate([o1, o2]), np.concatenate([d1, _in_ball(g, N_RAYS - h, 1.0)]))


def _checker(b):
    return b.lambertian(tex=b.checker(b.solid((0.8, 0.3, 0.2)), b.solid((0.2, 0.4, 0.9))))


CASES = {
    "floor-no-lights": _floor((), ("cosine-only",)),
    "floor-xz-light": _floor(("xz",), ("light-rect", "cosine-half")),                      # a one-entry list: gen_index(1) rejects half its words
    "floor-xy-yz-lights": _floor(("xy", "yz"), ("light-rect", "cosine-half")),
    "floor-sphere-light": _floor(("sphere",), ("light-sphere", "cosine-half")),
    "floor-three-lights": _floor(("yz", "sphere", "flipped"), ("light-rect", "light-sphere", "light-default", "zero-pdf", "cosine-half"), yz=-1),
    "floor-yz": _floor((), ("light-rect", "cosine-half", "onb-x"), yz=1),
    "checker-ball": _ball(_checker, 2, ("light-rect", "cosine-half")),
    "metal-0": _ball(lambda b: b.metal((0.9, 0.8, 0.7), 0.0), 2, ("metal", "fuzz-retry"), lights=()),
    "metal-0.3": _ball(lambda b: b.metal((0.9, 0.8, 0.7), 0.3), 2, ("metal", "fuzz-retry"), lights=()),
    "metal-1": _ball(lambda b: b.metal((0.9, 0.8, 0.7), 1.0), 2, ("metal", "fuzz-retry"), lights=()),
    "glass-outside-2": _ball(lambda b: b.dielectric(1.5), 2, ("reflect", "refract"), lights=()),
    "glass-outside-3": _ball(lambda b: b.dielectric(1.5), 3, ("reflect", "refract"), lights=()),
    "glass-inside": _ball(lambda b: b.dielectric(1.5), 2, ("cannot-refract", "refract"), origins=INSIDE, lights=()),
    "glass-pane-80": (_pane, 2, ("reflect", "refract")),
    "moved-box": (_moved_box, 2, ("light-rect", "cosine-half")),
    "fog-ball": (_fog, 2, ("medium-scattered", "medium-passed", "isotropic")),
}
NAMES = list(CASES)


class Case:
    """desc (keeps its builder), rays (the package's radiance ray records), depth, arms; stage, paths (brute_paths.Paths of
    all N_RAYS x SPP samples, sample s of ray i at i SPP + s), and per ray the summed value, its tolerance and keep."""
    pass


_cache = {}


def reference(name):
    if name in _cache:
        return _cache[name]
    build, depth, arms = CASES[name]
    g = np.random.default_rng(4000 + NAMES.index(name))
    b, (o, d) = build(g)
    c = Case()
    c.name, c.depth, c.arms = name, depth, arms
    c.desc = b.desc()
    c.desc._builder = b
    c.rays = rt.radiance_rays(o, d, time=0.0, rng_state=g.integers(1, 2 ** 63, len(o), dtype=np.uint64))
    c.stage = BP.Stage(c.desc)
    state = BP.path_key(np.repeat(c.rays["rng_state"], SPP), 0, 0, np.tile(np.arange(SPP), len(o)))
    c.paths = BP.ray_color(c.stage, np.repeat(o, SPP, axis=0), np.repeat(d, SPP, axis=0), np.zeros(len(o) * SPP), BP.Stream(state), BACKGROUND, depth)
    c.value, c.tol, c.keep = BP.sum_samples(c.paths, SPP)
    _cache[name] = c
    return c


# ---- camera cases: a 48 x 32 frame at 2 samples inside the same cube -------------------------------------------------------------
W, H, SEED = 48, 32, 77
EYE, AT = (0.6, 1.2, 3.0), (0.0, 0.2, 0.0)


def _view(aperture, focus, t0=0.0, t1=1.0):
    return rt.camera_new(EYE, AT, (0, 1, 0), 50.0, W / H, aperture, focus, t0, t1)


def _cam_cube(aperture, focus):
    def build():
        b = rt.DescBuilder()
        b.set_root(b.list(cube(b)))
        return b, _view(aperture, focus)
    return build


def _cam_floor():
    """Depth 2 over a Lambertian floor with one rect light, through a lens: the floor's draws start where get_ray's variable
    number of tries left the stream."""
    b = rt.DescBuilder()
    floor = b.rect(XZ, -2.5, 2.5, -2.5, 2.5, 0.0, b.lambertian((0.7, 0.6, 0.5)))
    world, listed = _lights(b, ("xz",))
    b.light(listed[0])
    b.set_root(b.list([floor] + world + cube(b)))
    return b, _view(0.5, 3.0)


def _cam_mover():
    """An emissive MovingSphere crossing the view during the shutter [0.25, 0.75]: whether a sample sees it is its drawn time."""
    b = rt.DescBuilder()
    s = b.moving_sphere((-2.0, 0.3, 0.0), (2.0, 0.3, 0.0), 0.25, 0.75, 0.5, b.diffuse_light((2.0, 3.0, 4.0)))
    b.set_root(b.list([s] + cube(b)))
    return b, _view(0.0, 3.0, 0.25, 0.75)


CAMERA_CASES = {"cam-pinhole": (_cam_cube(0.0, 3.0), 1), "cam-lens-focus-1": (_cam_cube(0.5, 1.0), 1), "cam-lens-focus-4": (_cam_cube(0.5, 4.0), 1),
                "cam-floor-depth-2": (_cam_floor, 2), "cam-moving-sphere": (_cam_mover, 1)}
CAMERA_NAMES = list(CAMERA_CASES)


def camera_reference(name):
    """→ Case with cam, params (rt_params of the frame), paths over H W SPP samples (pixel y W + x, sample s at (y W + x) SPP
    + s), value / tol / keep per pixel (H W,), camera_draws (words get_ray and the jitters took, per sample)."""
    key = "camera:" + name
    if key in _cache:
        return _cache[key]
    build, depth = CAMERA_CASES[name]
    b, cam = build()
    c = Case()
    c.name, c.depth, c.cam, c.arms = name, depth, cam, ()
    c.desc = b.desc()
    c.desc._builder = b
    c.params = rt.make_params(W, H, SPP, max_depth=depth, background=BACKGROUND, seed=SEED)
    c.stage = BP.Stage(c.desc)
    o, d, tm, stream, info = BP.camera_rays(cam, W, H, SPP, SEED)
    c.camera_draws, c.lens_tries, c.camera = stream.draws.copy(), info["tries"], dict(info, o=o, d=d, tm=tm)
    c.paths = BP.ray_color(c.stage, o, d, tm, stream, BACKGROUND, depth)
    c.paths.left_out["accept-edge"] |= info["accept-edge"]
    c.value, c.tol, c.keep = BP.sum_samples(c.paths, SPP)
    _cache[key] = c
    return c


def hold(c, got, who, rng_draws=None, quiet=False):
    """The assertions both modules make on a set of sums (per ray, or per pixel for a camera case): every kept entry within
    its tolerance, NaN where the reference has NaN; with rng_draws, the words drawn by all samples, left-out ones included
    → the line for the log."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 3)
    worst, bad = BP.compare(got, c.value, c.tol, c.keep)
    want_draws = int(c.paths.draws.sum()) + int(getattr(c, "camera_draws", np.zeros(1)).sum())
    nan = int((np.isnan(got).any(1) & c.keep).sum())
    line = "%-20s %-6s entries %5d compared %5d NaN %4d words %7d worst error / tolerance %.3e%s" % (
        c.name, who, len(c.keep), c.keep.sum(), nan, want_draws, worst, "" if not len(bad) else "  FAILURES %d" % len(bad))
    if not quiet:
        print(line)
    assert not len(bad), (c.name, who, [(int(i), got[i].tolist(), [float(x) for x in c.value[i]], float(c.tol[i])) for i in bad[:5]])
    assert worst <= 1.0
    if rng_draws is not None:
        assert int(rng_draws) == want_draws, (c.name, who, int(rng_draws), want_draws)
    return line


# ---- the oracle's single steps on the cases' first hits --------------------------------------------------------------------------
GOLDEN, MASK = 0x9E3779B97F4A7C15, (1 << 64) - 1


def _dbl(v):
    import ctypes as C
    return (C.c_double * len(v))(*[float(x) for x in v])


def first_bounce(c):
    """Per sample of a radiance case: the first ray, the stream's state where ray_color starts, and bounces[0]."""
    o = np.repeat(c.rays["origin"], SPP, axis=0)
    d = np.repeat(c.rays["direction"], SPP, axis=0)
    state = BP.path_key(np.repeat(c.rays["rng_state"], SPP), 0, 0, np.tile(np.arange(SPP), len(c.rays)))
    return o, d, state, c.paths.bounces[0]


def scatter_step(O, c, n=300):
    """rto_scatter on the reference's own first-hit record (rounded to f64) and first ray, on n compared samples of a case
    whose object is specular: the specular ray's origin, time and the attenuation are asserted → the worst direction error
    / tolerance. rto_scatter does not report its draws; the end-to-end sums hold their count."""
    import ctypes as C
    import brute_hits as B
    import brute_records as BR
    o, d, state, b0 = first_bounce(c)
    sc = c.stage.scene
    rays = np.zeros(len(o), dtype=BP.RAY_LD)
    rays["origin"], rays["direction"] = o, d
    ans = B.solve(sc, o, d, 0.0, 0.001, np.inf)
    R = BR.records(sc, rays, ans)
    pick = np.flatnonzero(c.paths.compared() & b0["alive"])[:n]
    assert len(pick) == n
    worst = 0.0
    out_ray, att, emitted = (C.c_double * 7)(), (C.c_double * 3)(), (C.c_double * 3)()
    for i in pick:
        rec = O.rto_hit_record(hit=1, front_face=int(R.front[i]), p=_dbl(R.p[i]), normal=_dbl(R.normal[i]), t=float(ans.t[i]),
                               u=float(R.u[i]), v=float(R.v[i]), mat=int(R.mat[i]))
        kind = O.lib().rto_scatter(C.byref(c.desc), int(R.mat[i]), _dbl(list(o[i]) + list(d[i]) + [0.0]), C.byref(rec), int(state[i]), out_ray, att, emitted)
        assert kind == 1 and list(emitted) == [0.0, 0.0, 0.0]
        want_d = b0["d"][i]
        err = np.sqrt(((B.LD(1) * np.array(out_ray[3:6]) - want_d) ** 2).sum())
        worst = max(worst, float(err) / ((b0["ddir"][i] + BR.ROUND) * float(np.sqrt((want_d * want_d).sum()))))
        assert out_ray[6] == float(b0["tm"][i]) and list(out_ray[0:3]) == [float(x) for x in R.p[i]]
        assert np.allclose(att[:], np.asarray(b0["attenuation"][i], dtype=np.float64), rtol=1e-15, atol=0)
    return worst


def lights_step(O, c, n=400):
    """rto_lights_random from the reference's first hit point with the stream where the mixture word left it — the words
    drawn are asserted — and rto_lights_pdf_value of the reference's direction against light_pdf → the worst direction and
    pdf error / tolerance over n compared light-half samples."""
    import ctypes as C
    import brute_records as BR
    LD = BP.LD
    o, d, state, b0 = first_bounce(c)
    P = c.paths
    pick = np.flatnonzero(P.compared() & (P.arms["light-rect"] | P.arms["light-sphere"] | P.arms["light-default"]))[:n]
    assert len(pick) == n
    out = (C.c_double * 3)()
    worst_d = worst_p = 0.0
    p64 = np.asarray(b0["o"], dtype=np.float64)
    lp, lp_tol, _, _ = BP.light_pdf(c.stage, LD(1) * p64[pick], b0["d"][pick], 0.0, b0["ddir"][pick])
    ratio = lambda e, t: e / t if t else (0.0 if e == 0 else np.inf)
    for j, i in enumerate(pick):
        draws = O.lib().rto_lights_random(C.byref(c.desc), _dbl(p64[i]), (int(state[i]) + GOLDEN) & MASK, out)
        assert draws == int(b0["draws"][i]) - 1, (i, draws, int(b0["draws"][i]))
        want = b0["d"][i]
        err = float(np.sqrt(((LD(1) * np.array(out[:]) - want) ** 2).sum()))
        worst_d = max(worst_d, ratio(err, (b0["ddir"][i] + BR.ROUND) * float(np.sqrt((want * want).sum()))))
        got = O.lib().rto_lights_pdf_value(C.byref(c.desc), _dbl(p64[i]), _dbl(np.asarray(want, dtype=np.float64)))
        worst_p = max(worst_p, ratio(abs(float(LD(got) - lp[j])), lp_tol[j] + BR.ROUND * float(lp[j])))
    return worst_d, worst_p


def check_camera_floors(c):
    """The same for a camera case: the caps; lens tries beyond the first where there is a lens; both mixture halves over the
    floor; samples that see the moving sphere and samples that do not."""
    P = c.paths
    counts = {k: int(v.sum()) for k, v in P.left_out.items()}
    compared = P.compared()
    assert len(compared) - compared.sum() <= LEFT_OUT_SHARE * len(compared), (c.name, counts)
    assert c.keep.sum() >= COMPARED_SHARE * len(c.keep), (c.name, int(c.keep.sum()))
    if float(c.cam.lens_radius) > 0:
        counts["lens tries > 1"] = int((compared & (c.lens_tries > 1)).sum())
        assert counts["lens tries > 1"] >= FLOOR
    if c.name == "cam-floor-depth-2":
        for arm in ("light-rect", "cosine-half"):
            assert (P.arms[arm] & compared).sum() >= FLOOR, (c.name, arm)
    if c.name == "cam-moving-sphere":
        mover = ((P.first_leaf >> 27) & 0xF) == 2                 # RT_KIND_MOVING_SPHERE
        counts["sees the sphere"] = int((compared & mover).sum())
        assert counts["sees the sphere"] >= FLOOR and (compared & ~mover).sum() >= FLOOR
    return counts


def check_floors(c):
    """The caps and floors of a case, from the reference alone → the per-class counts (printed by the callers)."""
    P = c.paths
    counts = {k: int(v.sum()) for k, v in P.left_out.items()}
    compared = P.compared()
    n = len(compared)
    assert n - compared.sum() <= LEFT_OUT_SHARE * n, (c.name, counts)
    assert c.keep.sum() >= COMPARED_SHARE * len(c.keep), (c.name, int(c.keep.sum()))
    for arm in c.arms:
        assert (P.arms[arm] & compared).sum() >= FLOOR, (c.name, arm, int((P.arms[arm] & compared).sum()))
    return counts
