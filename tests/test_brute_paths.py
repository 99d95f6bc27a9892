"""The oracle's scatter step, light sampling, mixture pdfs and camera against tests/brute_paths.py: a third statement of what
happens between two hits, per sample, in extended precision and with no code of oracle/ or csrc/ (rt_math.h's Onb, reflect,
refract and RNG conversions included). CPU only; tests/test_brute_paths_gpu.py holds the device to the same reference, computed
once per process in tests/path_cases.py. Classes, tolerances and their derivations: brute_paths' docstring."""
import ctypes as C
import struct

import mpmath as mp
import numpy as np
import pytest

import brute_hits as B
import brute_paths as BP
import brute_records as BR
import path_cases as PC
from radiometry_cases import F_rect

mp.mp.dps = 40
MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
LD = B.LD


def to_mp(x):
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


# ---- 1. the stream, by value ----------------------------------------------------------------------------------------------------
def py_mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def py_words(state, n):
    out = []
    for _ in range(n):
        state = (state + GOLDEN) & MASK
        out.append(py_mix64(state))
    return out


def test_stream_known_answers():
    """SplitMix64 from state 0: the published vector tests/test_math.py holds the oracle to; then the three conversions of
    rand 0.8.5 as that module states them, on Python integers."""
    every = np.ones(1, bool)
    st = BP.Stream([0])
    assert [hex(int(st.next_u64(every)[0])) for _ in range(3)] == ["0xe220a8397b1dcdaf", "0x6e789e6aa1b965f4", "0x6c45d188009454f"]
    words = py_words(123, 4096)
    st = BP.Stream([123])
    assert [float(st.gen_f64(every)[0]) for _ in range(64)] == [(w >> 11) * 2.0 ** -53 for w in words[:64]]
    st = BP.Stream([123])
    v12 = [struct.unpack("<d", struct.pack("<Q", (w >> 12) | 0x3FF0000000000000))[0] for w in words[:64]]
    got = [float(st.gen_range(every, -1.0, 1.0)[0]) for _ in range(64)]
    assert got == [(v - 1.0) * 2.0 + (-1.0) for v in v12] and min(got) >= -1.0 and max(got) < 1.0
    for n in (1, 3, 7):
        zone, k, want = ((n << (64 - n.bit_length())) - 1) & MASK, 0, []
        for _ in range(64):
            while True:
                m = words[k] * n
                k += 1
                if (m & MASK) <= zone:
                    want.append(m >> 64)
                    break
        st = BP.Stream([123])
        assert [int(st.gen_index(every, n)[0]) for _ in range(64)] == want and int(st.draws[0]) == k
    st = BP.Stream([123])
    [st.gen_index(every, 1) for _ in range(64)]
    assert 100 <= int(st.draws[0]) <= 160                        # gen_index(1): the zone is 2^63 - 1, half the words are drawn again


def test_path_key_restatement():
    def py_key(seed, frame, pixel, sample):
        h = py_mix64((seed + GOLDEN * (frame + 1)) & MASK)
        h = py_mix64(h ^ ((0xD1B54A32D192ED03 * (pixel + 1)) & MASK))
        return py_mix64(h ^ ((0x8CB92BA72F3D8DD7 * (sample + 1)) & MASK))
    g = np.random.default_rng(1)
    seeds = [0, 1, 2022, MASK] + [int(x) for x in g.integers(0, 2 ** 63, 20, dtype=np.uint64)]
    for seed in seeds:
        px = g.integers(0, 2 ** 40, 8)
        got = BP.path_key(seed, 3, px, np.arange(8))
        assert [int(x) for x in got] == [py_key(seed, 3, int(p), s) for s, p in enumerate(px)]
    lanes = BP.path_key(np.array(seeds, dtype=np.uint64), 0, 0, 1)
    assert [int(x) for x in lanes] == [py_key(s, 0, 0, 1) for s in seeds]


def test_masked_lanes_keep_their_state():
    st = BP.Stream([5, 5, 5])
    st.gen_range(np.array([True, False, True]), -1.0, 1.0)
    p, tries, _ = BP.unit_ball(st, np.array([True, False, False]))
    assert int(st.draws[1]) == 0 and int(st.s[1]) == 5 and int(st.draws[0]) == 1 + 3 * int(tries[0]) and int(st.draws[2]) == 1
    assert np.linalg.norm(p[0]) < 1


# ---- 2. the formulas against another form of themselves, mpmath at 40 digits -------------------------------------------------------
def test_cosine_density_is_the_jacobian():
    """The density of (r1, r2) -> direction on the sphere is 1 / |d dir / d r1 x d dir / d r2|, and must be cos / pi = z / pi."""
    def direction(r1, r2):
        phi = 2 * mp.pi * r1
        return mp.matrix([mp.cos(phi) * mp.sqrt(r2), mp.sin(phi) * mp.sqrt(r2), mp.sqrt(1 - r2)])
    for r1, r2 in ((0.1, 0.2), (0.77, 0.5), (0.3, 0.95), (0.999, 0.01), (0.5, 0.5)):
        mine = BP.cosine_direction(LD(r1), LD(r2))
        want = direction(mp.mpf(r1), mp.mpf(r2))
        assert max(abs(to_mp(mine[k]) - want[k]) for k in range(3)) < mp.mpf("1e-18")
        a = mp.matrix([mp.diff(lambda x: direction(x, mp.mpf(r2))[k], mp.mpf(r1)) for k in range(3)])
        b = mp.matrix([mp.diff(lambda y: direction(mp.mpf(r1), y)[k], mp.mpf(r2)) for k in range(3)])
        cross = mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        assert abs(1 / mp.norm(cross) - want[2] / mp.pi) < mp.mpf("1e-25")


def test_onb_is_orthonormal_and_right_handed():
    g = np.random.default_rng(2)
    n = g.normal(size=(40, 3)) * g.uniform(0.1, 30, (40, 1))
    n[:6] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0.95, 0.2, -0.1], [0.899, 0.3, 0.3], [0, 0, -7]]
    u, v, w, edge = BP.onb(LD(1) * n, np.zeros(40))
    assert not edge.any()
    for i in range(40):
        U, V, Wv = ([to_mp(x) for x in vec[i]] for vec in (u, v, w))
        dot = lambda a, b: sum(x * y for x, y in zip(a, b))
        for a in (U, V, Wv):
            assert abs(dot(a, a) - 1) < mp.mpf("1e-17")
        assert max(abs(dot(U, V)), abs(dot(U, Wv)), abs(dot(V, Wv))) < mp.mpf("1e-17")
        nn = [mp.mpf(float(x)) for x in n[i]]
        assert abs(dot(Wv, nn) - mp.sqrt(dot(nn, nn))) < mp.mpf("1e-16") * mp.sqrt(dot(nn, nn))      # w is unit(n), same sense
        cross = [Wv[1] * V[2] - Wv[2] * V[1], Wv[2] * V[0] - Wv[0] * V[2], Wv[0] * V[1] - Wv[1] * V[0]]
        assert max(abs(c - x) for c, x in zip(cross, U)) < mp.mpf("1e-17")                           # u = w x v
        a = [0, 1, 0] if abs(nn[0]) / mp.sqrt(dot(nn, nn)) > mp.mpf("0.9") else [1, 0, 0]
        assert abs(dot(V, a)) < mp.mpf("1e-17")                                                     # v is perpendicular to the chosen a
    assert BP.onb(LD(1) * np.array([[0.9 + 1e-14, np.sqrt(1 - 0.81), 0.0]]), np.zeros(1))[3][0]     # the class


def test_refract_obeys_snell():
    g = np.random.default_rng(3)
    for ratio in (1 / 1.5, 1.5, 1 / 2.4):
        for _ in range(30):
            unit = lambda a: a / np.sqrt((a * a).sum())            # (in longdouble: an f64 "unit" vector is one to 1e-16 only)
            n = unit(LD(1) * g.normal(size=3))
            t = unit(np.cross(n, LD(1) * g.normal(size=3)))
            sin_i = g.uniform(0.01, min(0.99, 0.99 / ratio))
            uv = unit(np.sqrt(1 - LD(sin_i) ** 2) * -n + LD(sin_i) * t)
            out, _, _ = BP.refract(uv[None], (LD(1) * n)[None], np.array([LD(ratio)]))
            O_, N, T, U = ([to_mp(x) for x in vec] for vec in (out[0], LD(1) * n, LD(1) * t, uv))
            dot = lambda a, b: sum(x * y for x, y in zip(a, b))
            assert abs(dot(O_, O_) - 1) < mp.mpf("1e-16")                                           # a unit vector
            sin_in = mp.sqrt(1 - dot(U, N) ** 2)
            sin_out = mp.sqrt(1 - dot(O_, N) ** 2)
            assert abs(sin_out - mp.mpf(ratio) * sin_in) < mp.mpf("1e-16")                            # Snell
            assert dot(O_, N) < 0 and dot(O_, T) > 0                                                # through the surface, same side of the normal
            b = [N[1] * U[2] - N[2] * U[1], N[2] * U[0] - N[0] * U[2], N[0] * U[1] - N[1] * U[0]]
            assert abs(dot(O_, b)) < mp.mpf("1e-16")                                                # in the plane of incidence
            r = BP.reflect(uv[None], (LD(1) * n)[None])[0]
            assert abs(dot([to_mp(x) for x in r], N) + dot(U, N)) < mp.mpf("1e-17")


def test_rect_density_integrates_to_the_form_factor():
    """pdf_value is a density over solid angle: d omega = dA / (area pdf). The integral of cos / pi d omega over the light is
    the point-to-rectangle form factor tests/radiometry_cases.py holds the estimator's mean to (F_rect), here by Gauss-Legendre
    quadrature of this module's own light_pdf."""
    c = PC.reference("floor-xz-light")
    (kind, q), = c.stage.lights
    a0, a1, b0, b1, h = (float(q[f]) for f in ("a0", "a1", "b0", "b1", "k"))
    nodes = mp.calculus.quadrature.GaussLegendre(mp.mp).calc_nodes(4, 200)
    x = np.array([float(n[0]) for n in nodes]); wq = np.array([float(n[1]) for n in nodes])
    X, Z = np.meshgrid(x, x)
    WQ = np.outer(wq, wq).ravel() * (a1 - a0) * (b1 - b0) / 4
    for p in ((0.0, 0.0, 0.0), (0.7, 0.0, -0.9), (-1.3, 0.0, 1.2)):
        pts = np.stack([(a0 + a1) / 2 + X.ravel() * (a1 - a0) / 2, np.full(X.size, h), (b0 + b1) / 2 + Z.ravel() * (b1 - b0) / 2], axis=1)
        o = np.broadcast_to(LD(1) * np.array(p), pts.shape)
        v = LD(1) * pts - o
        pdf, _, grazing, rim = BP.light_pdf(c.stage, o, v, 0.0, 0.0)
        assert not grazing.any() and (pdf > 0).all()
        cos = v[:, 1] / np.sqrt((v * v).sum(1))
        area = LD(a1 - a0) * LD(b1 - b0)
        total = float((LD(1) * WQ * cos / BP.PI / (area * pdf)).sum())
        want = F_rect(a0 - p[0], a1 - p[0], b0 - p[2], b1 - p[2], h)
        assert abs(total - want) < 1e-12 * want, (p, total, want)


# ---- 3. step by step --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["metal-0.3", "metal-1", "glass-outside-2", "glass-inside", "glass-pane-80"])
def test_scatter_step_against_reference(O, name):
    worst = PC.scatter_step(O, PC.reference(name))
    print("%-18s rto_scatter: 300 samples, worst direction error / tolerance %.3e" % (name, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["floor-xy-yz-lights", "floor-three-lights", "floor-sphere-light"])
def test_lights_random_and_pdf_value_step(O, name):
    worst_d, worst_p = PC.lights_step(O, PC.reference(name))
    print("%-18s rto_lights_random: worst direction error / tolerance %.3e; rto_lights_pdf_value: %.3e" % (name, worst_d, worst_p))
    assert worst_d <= 1.0 and worst_p <= 1.0


def test_scatter_on_hand_made_records(O, rt):
    """rto_scatter on records no geometry made: 600 unit normals in general position, rays against them, both flags, a Metal of
    fuzz 0.5 and a Dielectric of ir 1.5 — the specular ray from the reference's own functions and the stream's restatement."""
    g = np.random.default_rng(8)
    b = rt.DescBuilder()
    mats = {"metal": b.metal((0.9, 0.8, 0.7), 0.5), "glass": b.dielectric(1.5)}
    b.set_root(b.sphere((0, 0, 0), 1.0, mats["metal"]))
    desc = b.desc()
    n_rec = 600
    n64 = g.normal(size=(n_rec, 3)); n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    d64 = g.normal(size=(n_rec, 3)) * g.uniform(0.2, 5.0, (n_rec, 1))
    d64 -= n64 * np.maximum((d64 * n64).sum(1), 0)[:, None] * 2                  # against the normal, as set_face_normal leaves it
    front = g.random(n_rec) < 0.5
    state = g.integers(1, 2 ** 63, n_rec, dtype=np.uint64)
    p = g.normal(size=(n_rec, 3))
    every = np.ones(n_rec, bool)
    nrm, unit_d = LD(1) * n64, LD(1) * d64 / np.sqrt(((LD(1) * d64) ** 2).sum(1))[:, None]
    out_ray, att, emitted = (C.c_double * 7)(), (C.c_double * 3)(), (C.c_double * 3)()
    dbl = lambda v: (C.c_double * len(v))(*[float(x) for x in v])
    for name, mat in mats.items():
        st = BP.Stream(state)
        if name == "metal":
            ball, tries, edge = BP.unit_ball(st, every)
            want = BP.reflect(unit_d, nrm) + LD(0.5) * (LD(1) * ball)
            want_tm, arms, amp = 0.0, {"tries > 1": tries > 1}, np.ones(n_rec)
        else:
            word = LD(1) * st.gen_range(every, 0.0, 1.0)
            reflects, cannot, edge, ratio = BP.dielectric_choice(unit_d, nrm, front, LD(1.5), word, BR.ROUND)
            refr, perp, root = BP.refract(unit_d, nrm, ratio)
            want = np.where(reflects[:, None], BP.reflect(unit_d, nrm), refr)
            with np.errstate(all="ignore"):                          # (refract's root: the derivative of sqrt, as in the docstring)
                amp = np.where(reflects, 1.0, 1 + np.asarray(np.sqrt((perp * perp).sum(1)) / root, dtype=np.float64))
            want_tm, arms = 0.375, {"reflect": reflects & ~cannot, "cannot": cannot, "refract": ~reflects}
        assert edge.sum() <= 0.03 * n_rec and all((a & ~edge).sum() >= 50 for a in arms.values()), {k: int(a.sum()) for k, a in arms.items()}
        worst = 0.0
        for i in np.flatnonzero(~edge):
            rec = O.rto_hit_record(hit=1, front_face=int(front[i]), p=dbl(p[i]), normal=dbl(n64[i]), t=1.0, u=0.25, v=0.5, mat=mat)
            kind = O.lib().rto_scatter(C.byref(desc), mat, dbl(list(p[i] - d64[i]) + list(d64[i]) + [0.375]), C.byref(rec), int(state[i]), out_ray, att, emitted)
            assert kind == 1 and out_ray[6] == want_tm and list(out_ray[0:3]) == list(p[i])
            err = float(np.sqrt(((LD(1) * np.array(out_ray[3:6]) - want[i]) ** 2).sum()))
            worst = max(worst, err / (BR.ROUND * amp[i] * max(1.0, float(np.sqrt((want[i] ** 2).sum())))))
        print("hand-made records, %s: %d compared, worst direction error / (ROUND x amplification) %.3e; %s" % (
            name, (~edge).sum(), worst, {k: int((a & ~edge).sum()) for k, a in arms.items()}))
        assert worst <= 1.0


@pytest.mark.parametrize("name", ["cam-lens-focus-1", "cam-moving-sphere"])
def test_get_ray_step(O, name):
    c = PC.camera_reference(name)
    cam = c.camera
    ray = (C.c_double * 7)()
    worst = 0.0
    for i in range(0, len(cam["s"]), 3):
        draws = O.lib().rto_get_ray(C.byref(c.cam), float(cam["s"][i]), float(cam["t"][i]), (int(cam["key"][i]) + 2 * GOLDEN) & MASK, ray)
        assert draws == int(c.camera_draws[i]) - 2 == 2 * int(c.lens_tries[i]) + 1
        assert ray[6] == float(cam["tm"][i])
        scale = float(np.abs(cam["o"][i]).max() + np.abs(cam["d"][i]).max())
        err = max(float(np.abs(LD(1) * np.array(ray[0:3]) - cam["o"][i]).max()), float(np.abs(LD(1) * np.array(ray[3:6]) - cam["d"][i]).max()))
        worst = max(worst, err / (BR.ROUND * scale))
    print("%-18s rto_get_ray: worst error / (ROUND scale) %.3e, tries up to %d" % (name, worst, c.lens_tries.max()))
    assert worst <= 1.0 and c.lens_tries.max() >= 3
    if name == "cam-moving-sphere":
        assert 0.25 <= cam["tm"].min() < 0.3 and 0.7 < cam["tm"].max() < 0.75


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.NAMES)
def test_radiance_against_reference(O, name):
    c = PC.reference(name)
    print(name, PC.check_floors(c))                              # caps and floors, before the oracle is called
    got, st = O.radiance(c.desc, c.rays, spp=PC.SPP, background=PC.BACKGROUND, t_min=0.001, depth=c.depth, want_stats=True)
    PC.hold(c, got, "oracle", st.rng_draws)


@pytest.mark.parametrize("name", PC.CAMERA_NAMES)
def test_camera_frames_against_reference(O, name):
    c = PC.camera_reference(name)
    print(name, PC.check_camera_floors(c))
    got, st = O.render_cpu(c.desc, c.cam, c.params, np.arange(PC.H, dtype=np.uint32), want_stats=True)
    PC.hold(c, got, "oracle", st.rng_draws)
