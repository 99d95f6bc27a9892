"""The numpy restatements of the two denoisers (tests/denoise_ref.py `restate`, tests/denoise_dual_ref.py `restate_dual`), which
the GPU modules compare the kernels with bit for bit, held to what shares no code with them or with the kernels: the plain
loop of tests/denoise_exact.py in doubles (the same bits), in 53-bit intervals (every value inside its enclosure, every
enclosure narrower than 1e-12 relative) and at 200 bits (which pins the enclosure), and the closed forms of
tests/denoise_cases.py. No GPU. tests/test_denoise_exact_gpu.py asks the same of the library itself.

What is pinned: the definition on finite buffers — steps, sigmas, skipped taps, the normalisations, the variance
propagation, demodulation and the floor, row lists, n_iter = 0 and var_iter = 0. What is not: how NaN and inf travel; the
hostile buffers (NaN radiance and albedo, 1e30s, all-zero records) are a bit-for-bit matter between the restatements and
the plain loop in doubles, and between the restatements and the kernels.

Shown to fail. tools/denoise_report.py --mutants seeds each mistake into a scratch copy of the restatements and runs the
enclosure cases (21: 10 single, 11 dual) and the closed forms on it. "Widths" is the worst distance of a value from the
middle of its interval in interval widths (inside is at most 0.5):

    mistake                                enclosure names it in          widths    closed forms that name it
    1 step k + 1 instead of 2^k            16 of 21 cases (n_iter >= 3)   2.1e13    impulse n_iter 3 (both filters); two scales
    2 sigma_k not halved                   7 of 10 single (n_iter >= 2)   1.1e14    two scales
    3 taps clamped, not skipped            20 of 21 (not single 1x1)      1.9e14    impulse at the borders (both); two regions;
                                                                                    variance propagation n_iter 1; two scales
    4 u = su / sw                          10 of 11 dual cases            2.0e14    two regions; variance propagation n_iter 1
    5 2 u_p for u_p + u_q                  9 of 11 dual cases             2.2e13    two regions
    6 third albedo from another plane      19 of 21 (not the 1x1s)        1.7e14    edge stop, albedo (both)
    7 rows and columns exchanged (W, H     19 of 21 (not the 1x1s)        NaN       impulse n_iter 1, 2, 3; impulse at the
      swapped in the inside test)                                                   borders; ramp; edge stops; fixed point >= 4
    8 remodulation without the floor       9 of 21 (all six tight ones)   3.1e14    fixed point, every n_iter (both)

(The enclosure cases that cannot see a mistake are the ones where it changes nothing: one pixel has no taps to clamp, n_iter
= 1 has one step and one sigma, identical halves have no variance to propagate, a floor of 1e-3 is rarely above an albedo.)"""
import numpy as np
import pytest

import raytracer_2022_amd as rt

import denoise_cases as DC
import denoise_dual_ref as RD
import denoise_exact as X
import denoise_ref as RS
from compare import assert_same_bits

SHAPES = [(1, 1), (1, 9), (9, 1), (5, 3), (12, 9), (67, 9), (9, 67)]
BUFFERS = {"hostile": dict(hostile=True, nan_albedo=True), "hostile, finite albedo": dict(hostile=True, nan_albedo=False),
           "clean": dict(hostile=False)}
LOOP, RESTATED = DC.Loop(X.Float64()), DC.Restated()


def test_the_written_out_defaults_are_the_packages():
    p, q = rt.denoise_params(3, 2, DC.SINGLE["spp"]), rt.denoise_dual_params()
    for k in ("n_iter", "sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo", "albedo_floor"):
        assert getattr(p, k) == DC.SINGLE[k], k
    assert p.flags == 0 and DC.SINGLE["demodulate"]
    assert (rt.DUAL_DEFAULTS["sigma_color"], q.var_iter, q.var_floor) == (DC.DUAL["sigma_color"], DC.DUAL["var_iter"], DC.DUAL["var_floor"])


# ---- the restatements against the plain loop in doubles, bit for bit --------------------------------------------------------
def single_bits(sums, feat, prm, rows=None, what=""):
    g = DC.unpack(feat)
    assert_same_bits(RESTATED.single(sums, g, prm, rows), LOOP.single(sums, g, prm, rows), what)


def dual_bits(h, prm, rows=None, what=""):
    ga, gb = DC.unpack(h[2]), DC.unpack(h[3])
    got, ref = RESTATED.dual(h[0], h[1], ga, gb, prm, rows), LOOP.dual(h[0], h[1], ga, gb, prm, rows)
    assert_same_bits(got[0], ref[0], what)
    assert_same_bits(got[1], ref[1], (what, "variance"))


@pytest.mark.parametrize("kind", list(BUFFERS))
@pytest.mark.parametrize("W, H", SHAPES)
def test_restate_is_the_plain_loop(W, H, kind):
    sums, feat = RS.buffers(W, H, seed=W * 16 + H, **BUFFERS[kind])
    for n_iter in (0, 1, 2, 5):
        single_bits(sums, feat, dict(DC.SINGLE, n_iter=n_iter), what=(kind, n_iter))


@pytest.mark.parametrize("kind", list(BUFFERS))
@pytest.mark.parametrize("W, H", SHAPES)
def test_restate_dual_is_the_plain_loop(W, H, kind):
    h = RD.halves(W, H, seed=W * 16 + H, **BUFFERS[kind])
    for n_iter, var_iter in ((0, 0), (0, 3), (1, 1), (2, 0), (5, 1), (5, 3)):
        dual_bits(h, dict(DC.DUAL, n_iter=n_iter, var_iter=var_iter), what=(kind, n_iter, var_iter))


@pytest.mark.parametrize("name", list(RS.SWITCHES))
def test_restate_is_the_plain_loop_under_every_switch(name):
    """The buffers of tests/test_denoise.py's test_switches."""
    prm = dict(DC.SINGLE, **RS.SWITCHES[name])
    sums, feat = RS.buffers(70, 9, spp=prm["spp"], seed=5, hostile=True, nan_albedo=False)
    single_bits(sums, feat, prm, what=name)


@pytest.mark.parametrize("name", list(RD.SWITCHES))
def test_restate_dual_is_the_plain_loop_under_every_switch(name):
    """The buffers of tests/test_denoise_dual.py's test_switches."""
    prm = dict(DC.DUAL, **RD.SWITCHES[name])
    h = RD.halves(70, 9, spp=prm["spp"], seed=5, hostile=True, nan_albedo=False)
    dual_bits(h, prm, what=name)


@pytest.mark.parametrize("W, H", [(12, 9), (9, 67)])
def test_a_shuffled_row_list(W, H):
    """Buffer row i is image row rows[i]: both filters, against the loop and against the image-order result permuted."""
    rows = np.random.default_rng(H).permutation(H).astype(np.uint32)
    assert rows.tolist() != list(range(H))
    sums, feat = RS.buffers(W, H, seed=9, hostile=True, nan_albedo=False)
    single_bits(sums[rows], feat[rows], DC.SINGLE, rows, "rows")
    g = DC.unpack(feat[rows])
    assert_same_bits(LOOP.single(sums[rows], g, DC.SINGLE, rows), LOOP.single(sums, DC.unpack(feat), DC.SINGLE)[rows], "the loop's own rows")
    h = RD.halves(W, H, seed=9, hostile=True, nan_albedo=False)
    dual_bits(tuple(b[rows] for b in h), DC.DUAL, rows, "rows")
    ga, gb = DC.unpack(h[2]), DC.unpack(h[3])
    shuffled = LOOP.dual(h[0][rows], h[1][rows], DC.unpack(h[2][rows]), DC.unpack(h[3][rows]), DC.DUAL, rows)
    for got, ref in zip(shuffled, LOOP.dual(h[0], h[1], ga, gb, DC.DUAL)):
        assert_same_bits(got, ref[rows], "the loop's own rows, dual")


# ---- the restatements inside the enclosure ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.CASES))
def test_restatement_inside_the_enclosure(name):
    """Every value of every output inside its interval; every interval at most 1e-12 wide relative to its end point nearer
    zero; an exact 0 as [0, 0] and +0 (denoise_exact.rel_width / inside). The widths measured: 7e-15 to 3.6e-13."""
    for what, width, off, outside in DC.against_enclosure(name, RESTATED):
        print("%s %s: relative width %.3g, off the middle by %.3g half-widths" % (name, what, width, off))
        assert width <= DC.WIDTH_CAP, (name, what, width)
        assert outside == 0, (name, what, outside, off)


def test_the_cases_cover_what_they_are_meant_to():
    shapes = {DC.CASES[c][1:3] for c in DC.CASES}
    assert shapes >= set(SHAPES)
    for which, key, values in (("single", "n_iter", {1, 3, 5}), ("dual", "n_iter", {1, 3, 5}), ("dual", "var_iter", {0, 1, 3})):
        assert {DC.CASES[c][4][key] for c in DC.CASES if DC.CASES[c][0] == which} >= values
    assert {DC.CASES[c][6] for c in DC.CASES if DC.CASES[c][0] == "dual"} >= {0.0, 0.01, 0.1}
    assert all(any(DC.CASES[c][0] == w and DC.CASES[c][5] for c in DC.CASES) for w in ("single", "dual"))
    _, (_, (albedo, _, _), prm, _) = DC.case_inputs("single 12x9 n5 tight")
    under = (albedo / prm["spp"] < prm["albedo_floor"]).mean()
    assert 0.1 < under < 0.6                               # the floor is at work in the tight cases


# ---- the closed forms -------------------------------------------------------------------------------------------------------
FORMS = {"%s, %s" % (w, n): f for n, w, f in DC.closed_forms()}
FORMS_200 = {"%s, %s" % (w, n): f for n, w, f in DC.closed_forms(big=False)}


@pytest.mark.parametrize("name", list(FORMS_200))
def test_closed_form_holds_for_the_definition_at_200_bits(name):
    FORMS_200[name](DC.Loop(X.Mpf(200)))


@pytest.mark.parametrize("name", list(FORMS))
def test_closed_form_holds_for_the_plain_loop(name):
    FORMS[name](LOOP)


@pytest.mark.parametrize("name", list(FORMS))
def test_closed_form_holds_for_the_restatement(name):
    FORMS[name](RESTATED)


# ---- the enclosure pinned by the 200-bit loop -------------------------------------------------------------------------------
def outside_at_200_bits(res, enc):
    """How many 200-bit values lie outside their intervals, compared as rationals."""
    n = 0
    for r, (lo, hi) in zip(res, enc):
        for v, l, h in zip(r.reshape(-1), lo.reshape(-1), hi.reshape(-1)):
            n += not DC.Fr(float(l)) <= DC.frac(v) <= DC.Fr(float(h))
    return n


def at_200_bits(which, args):
    res = getattr(DC.Loop(X.Mpf(200)), which)(*args)
    return (res,) if which == "single" else res


def moved(a, idx, ulps=2):
    a = np.array(a, dtype=np.float64)
    for _ in range(ulps):
        a[idx] = np.nextafter(a[idx], np.inf)
    return a


@pytest.mark.parametrize("name", [c for c in DC.CASES if DC.CASES[c][1] * DC.CASES[c][2] <= 108])
def test_the_exact_value_lies_inside_every_interval(name):
    which, args = DC.case_inputs(name)
    assert outside_at_200_bits(at_200_bits(which, args), DC.enclosure(name)) == 0


def test_an_input_moved_by_two_ulp_leaves_the_interval():
    """The enclosure is no wider than the arithmetic makes it. Where the definition rounds little, two ulp on ONE input put
    the exact result of the moved input outside the ORIGINAL interval: with n_iter = 0 and no demodulation (S / 4 * 1 * 4:
    every interval a point) for each of the 45 sums in turn; with n_iter = 0 and demodulation ((c / m) * m: intervals of
    about 2 ulp) for at least one; and on identical halves through five iterations, where the variance's intervals are
    [0, 0]. After iterations the intervals are some tens of ulp wide and hold such a move: there the width cap speaks."""
    W, H = 5, 3
    sums, feat = RS.buffers(W, H, seed=3, hostile=False)
    g = DC.unpack(feat)
    interval = DC.Loop(X.Interval53())
    for demodulate, least in ((False, 45), (True, 1)):
        prm = dict(DC.SINGLE, n_iter=0, demodulate=demodulate)
        enc = [X.bounds(interval.single(sums, g, prm))]
        assert outside_at_200_bits(at_200_bits("single", (sums, g, prm)), enc) == 0
        left = sum(outside_at_200_bits(at_200_bits("single", (moved(sums, idx), g, prm)), enc) > 0 for idx in np.ndindex(H, W, 3))
        assert left >= least, (demodulate, left)
    name = "dual 12x9 n5 v1 same halves"
    which, args = DC.case_inputs(name)
    args = (moved(args[0], (4, 6, 1)),) + tuple(args[1:])
    assert outside_at_200_bits(at_200_bits(which, args), DC.enclosure(name)) > 0
