"""The CPU oracle's radiance against closed forms (tests/radiometry_cases.py): what no HIP-vs-oracle test can see — a misreading
of ray_color, the pdfs or the materials that kernels and oracle share. First the closed forms themselves against independent
numerical quadrature, then every case through rto_radiance at N = 2^18 samples (256 rays x 1024 spp, batch means per ray),
case H through rt_render_cpu at 64 spp.

Detection floor: an assertion fails for sure once the bias exceeds 6 se plus the run's own deviation, so a relative bias of
8 se / L fails with probability 0.98. At 2^18 that is 1.2 % (rect light) to 3 % (medium chord, the noisiest case); the GPU
module repeats the cases at 2^24, where it is 0.15 % to 0.4 %. The seeded defects this was tried against (a 0.6 / 0.4 mixture
value, a cos / 3 scattering pdf, a Schlick exponent of 4) shift the cases they touch by 3 % to 16 %, the furnace by more.
Not pinned here: bits, variance, textures and the BVH code (the scenes are lists of a few solid-coloured primitives)."""
import math
import os

import numpy as np
import pytest

import radiometry_cases as RC
from compare import same_bits
from query_scenes import every_kind_lit_scene
from radiance_ref import oracle_radiance, radiance_camera_rays, radiance_counters

N_RAYS, SPP = 256, 1024
THREADS = max(1, min(8, os.cpu_count() or 1))


# ---- the closed forms against quadrature ---------------------------------------------------------------------------------
def gauss(n, a, b):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (b - a) * x + 0.5 * (b + a), 0.5 * (b - a) * w


@pytest.mark.parametrize("rect", [RC.RECT, RC.SHADOW, (0.3, 0.9, -2.0, -1.5, 0.7), (-1e-4 - 0.5, 1.5 - 1e-4, -1.0, 0.7, 2.0)])
def test_F_rect_against_gauss_legendre(rect):
    """cos cos' / (pi r^2) dA = h^2 / (pi r^4) dx dz over the rectangle, 80 x 80 nodes."""
    x0, x1, z0, z1, h = rect
    x, wx = gauss(80, x0, x1)
    z, wz = gauss(80, z0, z1)
    r2 = x[:, None] ** 2 + z[None, :] ** 2 + h * h
    quad = float((wx[:, None] * wz[None, :] * h * h / (math.pi * r2 * r2)).sum())
    assert abs(RC.F_rect(*rect) - quad) <= 1e-12


@pytest.mark.parametrize("c,r", [(RC.BALL_C, RC.BALL_R), ((0.0, 5.0, 0.0), 1.0), ((1.0, 1.0, -2.0), 0.9)])
def test_sphere_cap_against_quadrature(c, r):
    """(n . w) / pi over the cone of directions that meet the sphere, in polar coordinates about the cone's axis: Gauss-Legendre
    in the polar angle, the rectangle rule (exact for a trigonometric polynomial) in the azimuth."""
    c = np.array(c)
    d = np.linalg.norm(c)
    w_axis = c / d
    a = np.cross(w_axis, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(w_axis, a)
    th, wth = gauss(64, 0.0, math.asin(r / d))
    ph = np.arange(64) * (2.0 * math.pi / 64)
    dirs_y = (np.sin(th)[:, None] * (np.cos(ph)[None, :] * a[1] + np.sin(ph)[None, :] * b[1]) + np.cos(th)[:, None] * w_axis[1])
    assert dirs_y.min() > 0.0                                     # the whole cone above the horizon
    quad = float((wth[:, None] * np.sin(th)[:, None] * dirs_y / math.pi).sum() * (2.0 * math.pi / 64))
    assert abs(RC.F_sphere(tuple(c), r) - quad) <= 1e-12


def test_furnace_fixed_point_by_iteration():
    f = RC.F_sphere((0.0, 5.0, 0.0), 1.0)                         # the lamp from a wall point, along its inward normal
    assert abs(f - RC.F_LAMP) <= 1e-17
    B = np.zeros(3)
    for _ in range(200):
        B = RC.RHO_W * (RC.LE_LAMP * f + (1.0 - f) * B)
    assert np.abs(B - RC.CASES["E_furnace"]["expected"]).max() <= 1e-15
    assert (RC.RHO_W * (1.0 - f)).max() ** 100 < 1e-17            # what depth 100 cuts off


def test_the_cases_geometry():
    """What the table's formulas assume: the occluder's shadow from P lies inside the light, the two lights' cones from P
    do not overlap, the glass rays meet the pane and their refractions the light, Schlick's r0 is 0.04."""
    sx0, sx1, sz0, sz1, _ = RC.SHADOW
    assert (sx0, sx1, sz0, sz1) == (2 * 0.0, 2 * 0.5, 2 * -0.2, 2 * 0.2)
    x0, x1, z0, z1, h = RC.RECT
    assert x0 < sx0 and sx1 < x1 and z0 < sz0 and sz1 < z1
    axis = np.array(RC.BALL_C) / np.linalg.norm(RC.BALL_C)
    cone = math.asin(RC.BALL_R / np.linalg.norm(RC.BALL_C))
    t = np.linspace(0.0, 1.0, 201)
    edge = np.concatenate([np.stack([x0 + (x1 - x0) * t, np.full_like(t, h), np.full_like(t, zz)], 1) for zz in (z0, z1)] +
                          [np.stack([np.full_like(t, xx), np.full_like(t, h), z0 + (z1 - z0) * t], 1) for xx in (x0, x1)])
    ang = np.arccos(edge @ axis / np.linalg.norm(edge, axis=1))
    assert ang.min() > cone + 0.05 and not (x0 < RC.BALL_C[0] * h / RC.BALL_C[1] < x1)      # (nor is the axis inside the rect)
    assert abs(RC.schlick(1.0) - 0.04) <= 1e-16
    for deg in (0.0, 60.0, 80.0):
        o, d = RC.CASES["G_glass_%d" % deg]["ray"]
        x_pane = o[0] + d[0] * (o[2] / -d[2])
        sin_t = math.sin(math.radians(deg)) / 1.5
        assert abs(x_pane) < 5.0 and abs(x_pane + 3.0 * sin_t / math.sqrt(1.0 - sin_t * sin_t)) < 50.0


def test_narrow_camera_sees_only_the_neighbourhood_of_P(rt):
    """Case C through a camera: the image's footprint on the floor stays within C_CAM_REACH of P, and over that square the
    closed form moves by less than a hundredth of the finest resolution any test has (se / L at 2^24)."""
    assert RC.narrow_camera_footprint(RC.narrow_camera(rt)) <= RC.C_CAM_REACH
    L = RC.CASES["C_two_lights_bg"]["expected"]
    assert np.array_equal(RC.expected_C_at(0.0, 0.0), L)
    for px in (-RC.C_CAM_REACH, RC.C_CAM_REACH):
        for pz in (-RC.C_CAM_REACH, RC.C_CAM_REACH):
            assert np.all(np.abs(RC.expected_C_at(px, pz) - L) <= 0.01 * min(RC.C_CAM_SE_REL.values()) * L)


# ---- the batched oracle entry equals the established loop ------------------------------------------------------------------
def test_rto_radiance_equals_the_ray_color_loop(rt, O):
    """rto_radiance against the Python loop over rto_ray_color (radiance_ref.oracle_radiance) on every_kind_lit_scene: the same
    sums bit for bit and the same counters, for any number of worker threads."""
    _, d, cam = every_kind_lit_scene(rt)
    g = np.random.default_rng(5)
    rays = radiance_camera_rays(rt, cam, 160, g)
    up = rt.radiance_rays((0.0, 3.0, 0.0), g.normal(size=(40, 3)), time=g.random(40), rng_state=g.integers(0, 2 ** 63, 40, dtype=np.uint64))
    odd = rt.radiance_rays([(-4, 1, 2), (0, 1, 8), (0, 0, 0)], [(0, 0, 0), (np.nan, 0, -1), (1e-300, 0, -1)], time=0.3, rng_state=7)
    rays = np.concatenate([rays, up, odd])
    for spp, bg, depth in ((3, (0.0, 0.0, 0.0), 50), (2, (0.3, 0.2, 0.7), 2)):
        ref, st_ref = oracle_radiance(O, d, rays, spp, bg, 0.001, depth)
        for threads in (1, 3, 7):
            got, st = O.radiance(d, rays, spp=spp, background=bg, depth=depth, n_threads=threads, want_stats=True)
            assert same_bits(got, ref), (spp, threads)
            assert radiance_counters(st) == radiance_counters(st_ref) and st.paths == len(rays) * spp, (spp, threads)
    assert np.any(ref != 0) and st_ref.prim_tests[rt._ffi.RT_KIND_MEDIUM] > 0 and st_ref.light_pdf_tests > 0
    empty, st = O.radiance(d, rays[:0], spp=4, want_stats=True)
    assert empty.shape == (0, 3) and st.paths == 0 and st.rays == 0
    zero = O.radiance(d, rays, spp=0)
    assert not np.any(zero.view(np.uint64))


# ---- every case on the oracle --------------------------------------------------------------------------------------------
_sums = {}


def oracle_sums(rt, O, name):
    if name not in _sums:
        case = RC.CASES[name]
        _, desc = case["scene"](rt)
        _sums[name] = O.radiance(desc, RC.case_rays(rt, case, N_RAYS, RC.SEED_CPU), spp=SPP, background=tuple(case["background"]),
                                 depth=case["depth"], n_threads=THREADS)
        _sums[name].setflags(write=False)
    return _sums[name]


@pytest.mark.parametrize("name", list(RC.CASES))
def test_case_on_the_oracle(rt, O, name):
    RC.check(name, oracle_sums(rt, O, name), SPP, cap=RC.SE_REL[name][18], tag="cpu")


def test_rect_light_depth_2_and_50_are_the_same_paths(rt, O):
    assert same_bits(oracle_sums(rt, O, "A_rect_d2"), oracle_sums(rt, O, "A_rect_d50"))


@pytest.mark.parametrize("aperture", RC.H_APERTURES)
def test_camera_on_the_oracle(rt, O, aperture):
    _, desc = RC.camera_scene(rt)
    p = rt.make_params(RC.H_W, RC.H_H, 64, 50, (0, 0, 0), seed=RC.SEED_CPU)
    sums = O.render_cpu(desc, RC.camera(rt, aperture), p, np.arange(RC.H_H), n_threads=THREADS)
    RC.check_camera(sums, 64, cap=RC.H_SE_REL[aperture][64], tag="cpu  H_camera_ap%.1f" % aperture)


def test_case_C_through_the_narrow_camera_on_the_oracle(rt, O):
    _, desc = RC.CASES["C_two_lights_bg"]["scene"](rt)
    p = rt.make_params(RC.C_CAM_W, RC.C_CAM_H, 64, 2, tuple(RC.BG_C), seed=RC.SEED_CPU)
    sums = O.render_cpu(desc, RC.narrow_camera(rt), p, np.arange(RC.C_CAM_H), n_threads=THREADS)
    RC.check("C_two_lights_bg", sums.reshape(-1, 3), 64, cap=RC.C_CAM_SE_REL[64], tag="cpu camera")
