"""Scenes whose mean radiance has a closed form, and the statistical criterion that holds an estimator to it. Not a test: the
table tests/test_radiometry.py (CPU oracle) and tests/test_radiometry_gpu.py (HIP path) share, like adaptive_ref.py.

Every expectation is derived from the reference's own lines — ray_color (main.rs:233-278), the pdfs (pdf.rs), the materials
(material/mod.rs), aarect.rs, sphere.rs, constantmedium.rs, camera.rs — in Python floats, by the formula beside each case;
none comes from a simulation or from this repository's restatement of those lines.

The criterion (judge / check below), with m_i the per-ray batch means, M their average, se = std(m_i, ddof=1) / sqrt(R)
and L the closed form, per channel:
  * no NaN or inf in any sum;
  * |M - L| <= 6 se — a two-sided normal tail of 2e-9 per assertion; the seeds are fixed, so a green run stays green;
  * the resolution cap se <= 1.25 * SE_REL[case][log2 N] * L, without which a noisy run passes anything. SE_REL is the
    largest se / L the CPU oracle showed for the case at that N (over the tests' seed and a second one); 1.25 covers the
    estimate's own scatter (about 1 % at 4096 batches, about 4.5 % at 256) and another seed.
tools/radiometry_report.py measures SE_REL and writes profiles/radiometry.log."""
import math

import numpy as np

PI = math.pi
T_MIN = 0.001
Z_MAX = 6.0
CAP_MARGIN = 1.25
SEED_CPU, SEED_GPU = 20221, 20222            # of the rng_state generators (numpy default_rng)


# ---- closed forms -------------------------------------------------------------------------------------------------------
def _G(x, z, h):
    a, b = math.sqrt(h * h + x * x), math.sqrt(h * h + z * z)
    return (x / a * math.atan(z / a) + z / b * math.atan(x / b)) / (2.0 * PI)


def F_rect(x0, x1, z0, z1, h):
    """Form factor of the rectangle [x0, x1] x [z0, z1] in the plane at height h over a point with the plane's normal as its
    own: the integral of cos / pi over the rectangle's solid angle."""
    return _G(x1, z1, h) - _G(x0, z1, h) - _G(x1, z0, h) + _G(x0, z0, h)


def F_sphere(c, r, n=(0.0, 1.0, 0.0)):
    """Form factor of a sphere (centre c relative to the point, radius r) wholly above the horizon of normal n:
    (r^2 / |c|^2) (c . n / |c|)."""
    d = math.sqrt(sum(x * x for x in c))
    cn = sum(a * b for a, b in zip(c, n))
    assert cn > r, "the sphere must clear the horizon"
    return (r * r / (d * d)) * (cn / d)


def furnace(rho, le, f):
    """Radiosity of a Lambertian sphere wall (albedo rho) around a concentric lamp of radiance le that fills the fraction f
    of every wall point's cosine-weighted hemisphere: the fixed point of B = rho (le f + (1 - f) B)."""
    return rho * le * f / (1.0 - rho * (1.0 - f))


def schlick(cos_theta, ir=1.5):
    """reflectance(cos, 1 / ir), material/mod.rs:112-116: r0 + (1 - r0)(1 - cos)^5 with r0 = ((1 - 1/ir) / (1 + 1/ir))^2."""
    r0 = ((1.0 - 1.0 / ir) / (1.0 + 1.0 / ir)) ** 2
    return r0 + (1.0 - r0) * (1.0 - cos_theta) ** 5


def _v(*x):
    return np.array(x, dtype=np.float64)


# ---- scenes: every one a root list; a ceiling light is flipped in the world and listed unflipped (scene.rs) --------------
RHO = _v(0.8, 0.5, 0.2)                      # the floor of cases A-D
LE_RECT, LE_BALL = _v(6.0, 5.0, 4.0), _v(9.0, 10.0, 11.0)
RECT = (-0.5, 1.5, -1.0, 0.7, 2.0)           # x0, x1, z0, z1, y of the rect light, P = (0, 0, 0)
BALL_C, BALL_R = (-2.5, 2.0, 1.0), 0.8
SHADOW = (0.0, 1.0, -0.4, 0.4, 2.0)          # the occluder [0, 0.5] x [-0.2, 0.2] at y = 1 projected from P onto y = 2
FLOOR_RAY = ((0.2, 0.6, -0.1), (-0.2, -0.6, 0.1))
UNFLIP = 0x7FFFFFFF


def _axis(rt, axis):
    F = rt._ffi
    return {"xz": F.RT_RECT_XZ, "xy": F.RT_RECT_XY, "yz": F.RT_RECT_YZ}[axis]


def floor_scene(rt, rect=0, ball=False, occluder=False, axis="xz"):
    """The floor [-50, 50]^2 through P = 0 with normal +k, `rect` entries of the rect light in the light list (it is in the
    world once), the sphere light, the black occluder."""
    b = rt.DescBuilder()
    ax = _axis(rt, axis)
    refs = [b.rect(ax, -50.0, 50.0, -50.0, 50.0, 0.0, b.lambertian(tuple(RHO)))]
    if rect:
        x0, x1, z0, z1, h = RECT
        light = b.rect(ax, x0, x1, z0, z1, h, b.diffuse_light(tuple(LE_RECT)), flip=True)
        refs.append(light)
        for _ in range(rect):
            b.light(light & UNFLIP)
    if ball:
        light = b.sphere(BALL_C, BALL_R, b.diffuse_light(tuple(LE_BALL)))
        refs.append(light)
        b.light(light)
    if occluder:
        refs.append(b.rect(ax, 0.0, 0.5, -0.2, 0.2, 1.0, b.lambertian((0.0, 0.0, 0.0))))
    b.set_root(b.list(refs))
    return b, b.desc()


def furnace_scene(rt):
    b = rt.DescBuilder()
    lamp = b.sphere((0, 0, 0), 1.0, b.diffuse_light((4.0, 5.0, 6.0)))
    b.set_root(b.list([b.sphere((0, 0, 0), 5.0, b.lambertian((0.5, 0.3, 0.7))), lamp]))
    b.light(lamp)
    return b, b.desc()


def medium_scene(rt):
    b = rt.DescBuilder()
    b.set_root(b.list([b.medium(b.sphere((0, 0, 0), 1.0, b.lambertian((0.5, 0.5, 0.5))), 0.9, b.isotropic((0.0, 0.0, 0.0)))]))
    return b, b.desc()


def glass_scene(rt):
    b = rt.DescBuilder()
    F = rt._ffi
    light = b.rect(F.RT_RECT_XY, -50.0, 50.0, -50.0, 50.0, -3.0, b.diffuse_light((2.0, 3.0, 4.0)))
    b.set_root(b.list([b.rect(F.RT_RECT_XY, -5.0, 5.0, -5.0, 5.0, 0.0, b.dielectric(1.5)), light]))
    b.light(light)
    return b, b.desc()


def _perm(axis, v):
    """A vector of the XZ layout (x, y, z) = (a, k, b) in the layout of `axis`."""
    a, k, b = v
    return {"xz": (a, k, b), "xy": (a, b, k), "yz": (k, a, b)}[axis]


F1, F2 = F_rect(*RECT), F_sphere(BALL_C, BALL_R)
BG_C = _v(0.3, 0.2, 0.1)
BG_F = _v(0.7, 0.8, 0.9)
BG_G, LE_G = _v(0.5, 0.25, 0.125), _v(2.0, 3.0, 4.0)
RHO_W, LE_LAMP, F_LAMP = _v(0.5, 0.3, 0.7), _v(4.0, 5.0, 6.0), (1.0 / 5.0) ** 2


def _glass(deg):
    th = math.radians(deg)
    r = schlick(math.cos(th))
    return dict(scene=glass_scene, ray=((0.0, 0.0, 0.5), (math.sin(th), 0.0, -math.cos(th))), background=BG_G, depth=50,
                expected=r * BG_G + (1.0 - r) * LE_G)


# name -> scene(rt) -> (builder, desc), ray (origin, direction), background, depth, expected mean radiance (3,)
CASES = {
    # A: rho Le F_rect — one bounce to the light; depth 2 and depth 50 trace the same paths (the same sums, bit for bit)
    "A_rect_d2": dict(scene=lambda rt: floor_scene(rt, rect=1), ray=FLOOR_RAY, background=_v(0, 0, 0), depth=2, expected=RHO * LE_RECT * F1),
    "A_rect_d50": dict(scene=lambda rt: floor_scene(rt, rect=1), ray=FLOOR_RAY, background=_v(0, 0, 0), depth=50, expected=RHO * LE_RECT * F1),
    # the light listed twice: HittableList::pdf_value (p + p) / 2 = p, random picks either — the same mean
    "A_listed_twice": dict(scene=lambda rt: floor_scene(rt, rect=2), ray=FLOOR_RAY, background=_v(0, 0, 0), depth=2, expected=RHO * LE_RECT * F1),
    # the same geometry with the coordinates renamed: the XY and YZ arms of aarect.rs
    "A_rect_xy": dict(scene=lambda rt: floor_scene(rt, rect=1, axis="xy"), ray=tuple(_perm("xy", v) for v in FLOOR_RAY),
                      background=_v(0, 0, 0), depth=2, expected=RHO * LE_RECT * F1),
    "A_rect_yz": dict(scene=lambda rt: floor_scene(rt, rect=1, axis="yz"), ray=tuple(_perm("yz", v) for v in FLOOR_RAY),
                      background=_v(0, 0, 0), depth=2, expected=RHO * LE_RECT * F1),
    # B: rho Le (r^2 / |C|^2)(C_y / |C|)
    "B_sphere": dict(scene=lambda rt: floor_scene(rt, ball=True), ray=FLOOR_RAY, background=_v(0, 0, 0), depth=2, expected=RHO * LE_BALL * F2),
    # C: rho (Le1 F1 + Le2 F2 + bg (1 - F1 - F2)); the lights' cones from P do not overlap
    "C_two_lights_bg": dict(scene=lambda rt: floor_scene(rt, rect=1, ball=True), ray=FLOOR_RAY, background=BG_C, depth=2,
                            expected=RHO * (LE_RECT * F1 + LE_BALL * F2 + BG_C * (1.0 - F1 - F2))),
    # D: rho Le (F_rect(light) - F_rect(shadow)); the black occluder's paths go on, times 0
    "D_occluder": dict(scene=lambda rt: floor_scene(rt, rect=1, occluder=True), ray=FLOOR_RAY, background=_v(0, 0, 0), depth=50,
                       expected=RHO * LE_RECT * (F1 - F_rect(*SHADOW))),
    # E: rho_w Le f / (1 - rho_w (1 - f)), f = (r / R)^2, exact by symmetry; the depth cut leaves 0.672^100
    "E_furnace": dict(scene=furnace_scene, ray=((2.0, 0.0, 0.0), (1.0, 0.3, 0.2)), background=_v(0, 0, 0), depth=100,
                      expected=furnace(RHO_W, LE_LAMP, F_LAMP)),
    # F: bg exp(-density * chord); the direction is not normalised (constantmedium.rs:57-58 scales by its length)
    "F_medium_chord": dict(scene=medium_scene, ray=((-3.0, 0.3, 0.4), (2.0, 0.0, 0.0)), background=BG_F, depth=50,
                           expected=BG_F * math.exp(-0.9 * 2.0 * math.sqrt(0.75))),
    # F': the origin inside: the entry is clamped to t_min = 0.001 (constantmedium.rs:52), not to 0
    "F_medium_inside": dict(scene=medium_scene, ray=((0.2, 0.3, 0.4), (2.0, 0.0, 0.0)), background=BG_F, depth=50,
                            expected=BG_F * math.exp(-0.9 * ((math.sqrt(0.75) - 0.2) / 2.0 - T_MIN) * 2.0)),
    # G: R bg + (1 - R) Le, R = 0.04 + 0.96 (1 - cos)^5: the reflected ray leaves, the refracted one ends on the light
    "G_glass_0": _glass(0.0),
    "G_glass_60": _glass(60.0),
    "G_glass_80": _glass(80.0),
}

# Largest se / L over the channels, CPU oracle, by log2 N (18: 256 rays x 1024 spp, 24: 4096 rays x 4096 spp); the larger of
# the tests' seed and a second one. Measured by tools/radiometry_report.py (profiles/radiometry.log).
SE_REL = {
    "A_rect_d2": {18: 1.693e-03, 24: 2.119e-04},
    "A_rect_d50": {18: 1.693e-03, 24: 2.119e-04},
    "A_listed_twice": {18: 1.673e-03, 24: 2.108e-04},
    "A_rect_xy": {18: 1.710e-03, 24: 2.114e-04},
    "A_rect_yz": {18: 1.710e-03, 24: 2.114e-04},
    "B_sphere": {18: 1.838e-03, 24: 2.410e-04},
    "C_two_lights_bg": {18: 1.532e-03, 24: 1.830e-04},
    "D_occluder": {18: 2.290e-03, 24: 2.821e-04},
    "E_furnace": {18: 3.191e-03, 24: 3.281e-04},
    "F_medium_chord": {18: 3.717e-03, 24: 4.761e-04},
    "F_medium_inside": {18: 1.694e-03, 24: 2.201e-04},
    "G_glass_0": {18: 4.000e-04, 24: 4.882e-05},
    "G_glass_60": {18: 5.172e-04, 24: 6.506e-05},
    "G_glass_80": {18: 1.460e-03, 24: 1.918e-04},
}

# the same for case H by (aperture, spp) and for case C through the narrow camera by spp (64 x 48 and 64 x 64 pixels)
H_SE_REL = {0.0: {64: 1.701e-03, 4096: 2.104e-04}, 0.5: {64: 3.151e-03, 4096: 3.964e-04}}
C_CAM_SE_REL = {64: 1.494e-03, 4096: 1.832e-04}

# ---- C through a render (the megakernel engine takes no caller rays): a pinhole at the floor ray's origin looking at P with
# a field of view so narrow that every pixel sees P's neighbourhood, where L is constant far below the resolution ----------
C_CAM_W = C_CAM_H = 64
C_CAM_VFOV = 0.002                           # degrees: the image's footprint on the floor stays within C_CAM_REACH of P
C_CAM_REACH = 2e-5


def expected_C_at(px, pz):
    """Case C's closed form with the floor point at (px, 0, pz) in place of P = 0."""
    x0, x1, z0, z1, h = RECT
    f1 = F_rect(x0 - px, x1 - px, z0 - pz, z1 - pz, h)
    f2 = F_sphere((BALL_C[0] - px, BALL_C[1], BALL_C[2] - pz), BALL_R)
    return RHO * (LE_RECT * f1 + LE_BALL * f2 + BG_C * (1.0 - f1 - f2))


def narrow_camera(rt):
    return rt.camera_new(FLOOR_RAY[0], (0, 0, 0), (0, 1, 0), C_CAM_VFOV, 1.0, 0.0, 1.0, 0.0, 1.0)


def narrow_camera_footprint(cam):
    """The largest |x|, |z| on the floor y = 0 over the corners of the image, the (W - 1) overshoot of main.rs:147-148 included."""
    o, llc, hor, ver = (np.array(v[:]) for v in (cam.origin, cam.lower_left_corner, cam.horizontal, cam.vertical))
    reach = 0.0
    for s in (0.0, C_CAM_W / (C_CAM_W - 1.0)):
        for t in (0.0, C_CAM_H / (C_CAM_H - 1.0)):
            d = llc + s * hor + t * ver - o
            p = o + d * (-o[1] / d[1])
            reach = max(reach, abs(p[0]), abs(p[2]))
    return reach


# ---- H: the camera (camera.rs, main.rs:141-152) through a render ---------------------------------------------------------
H_W, H_H, H_VFOV, H_FOCUS, H_DIST = 64, 48, 40.0, 10.0, 6.0
H_RECT = (0.6, 1.9, -1.6, -0.5)              # x0, x1, y0, y1 at z = -6: centre 13.5 px right of and 11.3 px below the centre
H_LE = _v(2.0, 3.0, 4.0)
H_APERTURES = (0.0, 0.5)                     # lens radius 0.25: a blur of 0.1 at z = -6, about one pixel, inside the frame
H_VER = 2.0 * math.tan(math.radians(H_VFOV) / 2.0) * H_FOCUS      # |vertical|, |horizontal| of camera.rs:40-48
H_HOR = H_VER * H_W / H_H


def camera_expected():
    """(mean over all pixels of L / Le, the rect's projected centre in (pixel, row) coordinates, row 0 at the bottom).
    A sample of pixel (x, y) aims at the focus-plane point llc + (x + r) / (W - 1) hor + (y + r') / (H - 1) ver: a pixel's
    footprint there is |hor| / (W - 1) by |ver| / (H - 1) — the (W - 1) divisor of main.rs:147-148 — and the rect, projected
    from the lens (a point, or a disk whose offset the uniform footprint integrates out), covers (x1 - x0)(y1 - y0)(10 / 6)^2."""
    x0, x1, y0, y1 = H_RECT
    k = H_FOCUS / H_DIST
    mean = (x1 - x0) * (y1 - y0) * k * k / (H_HOR * H_VER * H_W / (H_W - 1) * H_H / (H_H - 1))
    cx = ((x0 + x1) / 2.0 * k + H_HOR / 2.0) / H_HOR * (H_W - 1)
    cy = ((y0 + y1) / 2.0 * k + H_VER / 2.0) / H_VER * (H_H - 1)
    return mean, (cx, cy)


def camera_scene(rt):
    b = rt.DescBuilder()
    x0, x1, y0, y1 = H_RECT
    b.set_root(b.list([b.rect(rt._ffi.RT_RECT_XY, x0, x1, y0, y1, -H_DIST, b.diffuse_light(tuple(H_LE)))]))
    return b, b.desc()


def camera(rt, aperture):
    cam = rt.camera_new((0, 0, 0), (0, 0, -1), (0, 1, 0), H_VFOV, H_W / H_H, aperture, H_FOCUS, 0.0, 1.0)
    assert abs(np.linalg.norm(cam.horizontal[:]) - H_HOR) < 1e-12 and abs(np.linalg.norm(cam.vertical[:]) - H_VER) < 1e-12
    return cam


def check_camera(sums, spp, cap=None, log=None, tag=""):
    """The two assertions of case H on a render's sums (H, W, 3), rows in image order from the bottom. A sample is Le or 0, so
    a pixel's mean is Le p with variance p (1 - p) / spp; se sums that over the pixels."""
    s = np.asarray(sums, dtype=np.float64)
    assert s.shape == (H_H, H_W, 3) and np.isfinite(s).all()
    p = s / spp / H_LE                                            # per pixel and channel: the fraction of samples on the light
    L, (cx, cy) = camera_expected()
    M = p.mean(axis=(0, 1))
    se = np.sqrt((p * (1.0 - p) / spp).sum(axis=(0, 1))) / (H_W * H_H)
    z = (M - L) / se
    w = p[..., 1]
    gx = (w * (np.arange(H_W) + 0.5)[None, :]).sum() / w.sum()
    gy = (w * (np.arange(H_H) + 0.5)[:, None]).sum() / w.sum()
    line = "%-22s N=%d M=%s L=%.9g z=%s se/L=%.3e centroid=(%.3f, %.3f) expected=(%.3f, %.3f)" % (
        tag, s.shape[0] * s.shape[1] * spp, _fmt(M), L, _fmt(z, "%+.2f"), (se / L).max(), gx, gy, cx, cy)
    print(line)
    if log is not None:
        log.append(line)
    assert np.all(np.abs(M - L) <= Z_MAX * se), line
    if cap is not None:
        assert np.all(se <= CAP_MARGIN * cap * L), line
    assert abs(gx - cx) <= 0.5 and abs(gy - cy) <= 0.5, line
    return (se / L).max()


# ---- the criterion ------------------------------------------------------------------------------------------------------
def _fmt(v, f="%.9g"):
    return "(" + ", ".join(f % x for x in np.ravel(v)) + ")"


def case_rays(rt, case, n_rays, seed):
    """n_rays copies of the case's ray with rng_states drawn over [0, 2^63) from a seeded numpy generator."""
    states = np.random.default_rng(seed).integers(0, 2 ** 63, n_rays, dtype=np.uint64)
    return rt.radiance_rays(case["ray"][0], case["ray"][1], rng_state=states)


def judge(sums, spp, expected):
    """Per channel: (M, se, z) of the per-ray batch means sums / spp against the closed form."""
    m = np.asarray(sums, dtype=np.float64) / spp
    M = m.mean(axis=0)
    se = m.std(axis=0, ddof=1) / math.sqrt(len(m))
    with np.errstate(divide="ignore", invalid="ignore"):
        return M, se, (M - expected) / se


def check(name, sums, spp, cap=None, tag="", log=None):
    """The criterion of the module docstring on the (R, 3) sums of case `name`; cap: SE_REL's figure for this N or None
    (no resolution cap: measuring). Prints (and appends to `log`) N, M, L, z, se / L before it asserts; → max se / L."""
    L = CASES[name]["expected"]
    s = np.asarray(sums, dtype=np.float64)
    assert np.isfinite(s).all(), "%s: NaN or inf in %d sums" % (name, (~np.isfinite(s)).sum())
    M, se, z = judge(s, spp, L)
    line = "%-4s %-16s N=%d M=%s L=%s z=%s se/L=%.3e" % (tag, name, len(s) * spp, _fmt(M), _fmt(L), _fmt(z, "%+.2f"), (se / L).max())
    print(line)
    if log is not None:
        log.append(line)
    assert np.all(np.abs(M - L) <= Z_MAX * se), line
    if cap is not None:
        assert np.all(se <= CAP_MARGIN * cap * L), line
    return (se / L).max()
