"""rt_math.h on the host against a multiprecision reference (tests/math_ref.py) on the arguments of tests/math_cases.py.

The HIP path and the oracle compile the same header, so parity cannot see a wrong sin_; this file can. First the measure
itself is pinned (constructed errors of exactly 1/2, 1 and 2 ulp, two precisions, two results that must fail), then the
families are shown to reach every branch of rem_pio2, then every family of every function is held to its bound:
sin / cos / acos / log under 1 ulp of the exact value, atan2 under 2 (math_ref.BOUNDS says why), sqrt and '/' equal to IEEE.
Figures measured with tools/math_report.py are in profiles/math_edges.log."""
import math

import mpmath
import numpy as np
import pytest

import math_cases as MC
import math_ref as MR
from math_ref import SIN, COS, ACOS, ATAN2, LOG, SQRT, DIV


def mpf2(e):
    return mpmath.ldexp(mpmath.mpf(1), e)


# ------------------------------------------------------------------------------------------------ the measure ---
@pytest.mark.parametrize("what,exact,got,want", [
    # inside a binade: the ulp of 1.5 is 2^-52
    ("inside, 1/2", lambda: mpmath.mpf(1.5) + mpf2(-53), 1.5, 0.5),
    ("inside, 1", lambda: mpmath.mpf(1.5), 1.5 + 2.0 ** -52, 1.0),
    ("inside, 2", lambda: mpmath.mpf(1.5), 1.5 - 2.0 ** -51, 2.0),
    # exact value 1: its ulp is 2^-52 on both sides, although the doubles below 1 are 2^-53 apart
    ("at 1 from below, 1/2", lambda: mpmath.mpf(1), 1.0 - 2.0 ** -53, 0.5),
    ("at 1 from below, 1", lambda: mpmath.mpf(1), 1.0 - 2.0 ** -52, 1.0),
    ("at 1 from below, 2", lambda: mpmath.mpf(1), 1.0 - 2.0 ** -51, 2.0),
    ("at 1 from above, 1", lambda: mpmath.mpf(1), 1.0 + 2.0 ** -52, 1.0),
    ("at 1 from above, 2", lambda: mpmath.mpf(1), 1.0 + 2.0 ** -51, 2.0),
    # exact value just under 1: its ulp is 2^-53, so the double 1.0 is 1/2 away and 1 + 2^-52 is 2 1/2 away
    ("under 1, 1/2", lambda: mpmath.mpf(1) - mpf2(-54), 1.0, 0.5),
    ("under 1, 1", lambda: mpmath.mpf(1) - mpf2(-53), 1.0, 1.0),
    ("under 1, 2", lambda: mpmath.mpf(1) - mpf2(-53), 1.0 - 3 * 2.0 ** -53, 2.0),
    ("under 1, 2 1/2 across the edge", lambda: mpmath.mpf(1) - mpf2(-54), 1.0 + 2.0 ** -52, 2.5),
    # exact value just over 1: its ulp is 2^-52, so the double 1 - 2^-53 is 1 away, not 2
    ("over 1, 1/2", lambda: mpmath.mpf(1) + mpf2(-53), 1.0, 0.5),
    ("over 1, 1 across the edge", lambda: mpmath.mpf(1) + mpf2(-53), 1.0 - 2.0 ** -53, 1.0),
    ("over 1, 2", lambda: mpmath.mpf(1) + mpf2(-52), 1.0 + 3 * 2.0 ** -52, 2.0),
    # subnormal range: the ulp stays 2^-1074 however small the exact value
    ("subnormal, 1/2", lambda: 5.5 * mpf2(-1074), 5 * 2.0 ** -1074, 0.5),
    ("subnormal, 1", lambda: 5 * mpf2(-1074), 6 * 2.0 ** -1074, 1.0),
    ("subnormal, 2", lambda: 5 * mpf2(-1074), 3 * 2.0 ** -1074, 2.0),
    ("subnormal, to zero", lambda: 2 * mpf2(-1074), 0.0, 2.0),
    ("below the subnormals, 1/2", lambda: mpf2(-1075), 0.0, 0.5),
    ("largest subnormal to smallest normal, 1", lambda: mpf2(-1022) - mpf2(-1074), 2.0 ** -1022, 1.0),
    ("smallest normal, 2", lambda: mpf2(-1022), 2.0 ** -1022 + 2.0 ** -1073, 2.0),
])
def test_ulp_error_on_constructed_values(what, exact, got, want):
    with mpmath.workprec(MR.PREC):
        e = exact()
        assert MR.ulp_error(got, e) == want, what
        assert MR.ulp_error(-got, -e) == want, what


def test_classes_nan_infinities_and_signed_zeros():
    assert MR.ulp_error(math.nan, math.nan) == 0.0 and MR.ulp_error(-math.nan, math.nan) == 0.0     # NaN as a class
    assert MR.ulp_error(0.0, math.nan) == math.inf and MR.ulp_error(math.nan, 0.0) == math.inf
    assert MR.ulp_error(math.inf, math.inf) == 0.0 and MR.ulp_error(-math.inf, math.inf) == math.inf
    assert MR.ulp_error(0.0, 0.0) == 0.0 and MR.ulp_error(-0.0, -0.0) == 0.0
    assert MR.ulp_error(-0.0, 0.0) == math.inf and MR.ulp_error(0.0, -0.0) == math.inf               # a zero with its sign
    assert MR.ulp_error(5e-324, 0.0) == math.inf
    with mpmath.workprec(MR.PREC):
        assert MR.ulp_error(math.nan, mpmath.mpf(1)) == math.inf and MR.ulp_error(math.inf, mpmath.mpf(1)) == math.inf
    # the exact zeros of the functions, and Annex F's
    assert [MR.exact(SIN, [0.0, -0.0])[i] for i in (0, 1)] == [0.0, -0.0] and math.copysign(1, MR.exact(SIN, [-0.0])[0]) == -1
    assert MR.exact(LOG, [1.0])[0] == 0.0 and MR.exact(ACOS, [1.0])[0] == 0.0 and MR.exact(COS, [0.0])[0] == 1
    assert MR.exact(LOG, [0.0, -0.0, math.inf]) == [-math.inf, -math.inf, math.inf] and math.isnan(MR.exact(LOG, [-1.0])[0])
    z = MR.exact(ATAN2, [0.0, -0.0, -0.0, 2.0, -2.0], [1.0, 0.0, 3.0, math.inf, math.inf])
    assert [math.copysign(1, v) for v in z] == [1, -1, -1, 1, -1] and all(v == 0 for v in z)
    assert math.isnan(MR.exact(SIN, [math.inf])[0]) and math.isnan(MR.exact(ACOS, [np.nextafter(1.0, 2.0)])[0])


def test_pio2_constant_of_the_cases():
    with mpmath.workprec(600):
        assert MC.PIO2_INT == int(mpmath.floor(mpmath.pi() / 2 * mpmath.mpf(2) ** MC.PIO2_BITS))


def near_multiples():
    fam = MC.families(SIN)
    return np.concatenate([fam[k][0] for k in fam if k.startswith("nearest k*pi/2")])


def test_400_and_800_bits_classify_alike(O):
    """Next to k * pi/2 with k near 2^50 the result's first bit lies more than 100 bits under the argument's; 400 bits are enough
    if doubling them changes nothing."""
    x = near_multiples()
    for op in (SIN, COS):
        got = O.math_array(op, x)
        e400 = MR.ulp_errors(got, MR.exact(op, x, prec=400), prec=400)
        e800 = MR.ulp_errors(got, MR.exact(op, x, prec=800), prec=800)
        assert np.array_equal(e400 < 1.0, e800 < 1.0)
        assert np.array_equal(e400 < 0.5, e800 < 0.5)
        assert np.allclose(e400, e800, rtol=1e-9, atol=0)


def test_checker_names_the_one_entry_moved_two_doubles_away():
    x = near_multiples()
    for op in (SIN, COS):
        ref = MR.exact(op, x)
        got = MR.nearest(ref)
        assert len(MR.failures(got, ref, 1.0)) == 0 and MR.ulp_errors(got, ref).max() <= 0.5
        for i in (0, len(x) // 3, len(x) - 1):
            bad = got.copy()
            away = math.copysign(math.inf, bad[i])                       # (away from zero: the spacing cannot shrink)
            bad[i] = np.nextafter(np.nextafter(bad[i], away), away)
            assert MR.failures(bad, ref, 1.0).tolist() == [i]
            assert 1.5 <= MR.ulp_errors(bad, ref)[i] <= 4.5                 # (2 +- 1/2; twice that where the two steps cross into the next binade)


def test_checker_flags_single_precision_arguments():
    x = MC.families(SIN)["uniform 1e5..1.6e6"][0]
    ref = MR.exact(SIN, x)
    assert len(MR.failures(np.sin(x), ref, 1.0)) == 0                                   # the platform's sin passes
    assert len(MR.failures(np.sin(x.astype(np.float32)).astype(np.float64), ref, 1.0)) > 0.9 * len(x)


# --------------------------------------------------------------------------------------------- branch coverage ---
def test_families_reach_every_branch_of_rem_pio2():
    """Predicates from the arguments and the exact reduction alone, never from the code under test: the high-word ranges of
    rem_pio2, the exponent drop from x to its exact remainder against 16 and 49 (second and third Cody-Waite round), and —
    for the large branch — whether a quotient rounded in double precision names the wrong multiple."""
    x, _, _ = MC.concatenated(SIN)
    ix = (MC.to_bits(x) >> np.uint64(32)).astype(np.int64) & 0x7FFFFFFF
    finite = ix < 0x7FF00000
    assert (~finite).sum() == 3 and np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()   # (one branch, no arithmetic: x - x)
    count = {"|x| <= pi/4": int((ix <= 0x3FE921FB).sum()), "|x| >= 2^52": len(MC.sincos_at_or_above_2p52())}
    medium = np.flatnonzero((ix > 0x3FE921FB) & (ix < 0x413921FB))
    large = np.flatnonzero((ix >= 0x413921FB) & (ix < 0x43300000))
    drop = np.array([MR.exponent_drop(float(v), MR.pio2_quotient(float(v))[1]) for v in x[medium]])
    count["medium, first round only"] = int((drop <= 16).sum())
    count["medium, second round"] = int(((drop > 16) & (drop <= 49)).sum())
    count["medium, third round"] = int((drop > 49).sum())
    count["large"] = len(large)
    ax = np.abs(x[large])
    reduced = [MR.pio2_quotient(float(v)) for v in ax]
    n_double = np.floor(ax * (2.0 / np.pi) + 0.5)
    n_exact = np.array([n for n, _ in reduced], dtype=np.float64)
    count["large, double-precision quotient one too high"] = int((n_double > n_exact).sum())
    # never one too low: the double nearest 2/pi lies above it, and k + 1/2 is on the quotient's grid wherever its ulp is
    # <= 1/2, so a product above k + 1/2 never rounds below it (the header's step up by one is a guard no argument takes)
    assert int((n_double < n_exact).sum()) == 0 and np.all(np.abs(n_double - n_exact) <= 1)
    ldrop = np.array([MR.exponent_drop(float(v), y) for v, (_, y) in zip(ax, reduced)])
    count["large, remainder cancels more than 53 bits"] = int((ldrop > 53).sum())
    for lo, hi in ((0x413921FB, 0x41F00000), (0x41F00000, 0x42900000), (0x42900000, 0x43300000)):
        count["large, high word %#x..%#x" % (lo, hi)] = int(((ix >= lo) & (ix < hi)).sum())
    assert all(v >= 20 for v in count.values()), count


def test_families_reach_the_branches_of_acos_atan2_and_log():
    count = {}
    x = MC.concatenated(ACOS)[0]
    ix = (MC.to_bits(x) >> np.uint64(32)).astype(np.int64) & 0x7FFFFFFF
    count["acos |x| <= 2^-57"] = int((ix <= 0x3C600000).sum())
    count["acos |x| < 0.5"] = int(((ix > 0x3C600000) & (ix < 0x3FE00000)).sum())
    count["acos x <= -0.5"] = int(((ix >= 0x3FE00000) & (ix < 0x3FF00000) & (x < 0)).sum())
    count["acos x >= 0.5"] = int(((ix >= 0x3FE00000) & (ix < 0x3FF00000) & (x > 0)).sum())
    y, x, _ = MC.concatenated(ATAN2)
    ok = np.isfinite(x) & np.isfinite(y) & (x != 0) & (y != 0)
    y, x = y[ok], x[ok]
    k = ((MC.to_bits(y) >> np.uint64(52)).astype(np.int64) & 0x7FF) - ((MC.to_bits(x) >> np.uint64(52)).astype(np.int64) & 0x7FF)
    count["atan2 exponents more than 60 apart, y the larger"] = int((k > 60).sum())
    count["atan2 exponents more than 60 apart, x the larger and negative"] = int(((k < -60) & (x < 0)).sum())
    with np.errstate(over="ignore", under="ignore"):
        q = np.abs(y / x)
    through_atan = (x == 1) | ~((k > 60) | ((k < -60) & (x < 0)))          # (the quotients atan2_ hands on to atan_)
    for name, lo, hi in (("< 2^-27", 0, 2.0 ** -27), ("< 7/16", 2.0 ** -27, 7 / 16), ("< 11/16", 7 / 16, 11 / 16), ("< 19/16", 11 / 16, 19 / 16),
                         ("< 39/16", 19 / 16, 39 / 16), ("< 2^66", 39 / 16, 2.0 ** 66), (">= 2^66", 2.0 ** 66, np.inf)):
        count["atan2 |y/x| " + name] = int(((q >= lo) & (q < hi) & through_atan).sum())
    for m in range(4):
        count["atan2 quadrant %d" % m] = int((((y < 0) + 2 * (x < 0)) == m).sum())
    x = MC.concatenated(LOG)[0]
    x = x[(x > 0) & np.isfinite(x)]
    m, e = np.frexp(x)
    count["log subnormal"] = int((x < 2.0 ** -1022).sum())
    f = np.where(m < np.sqrt(0.5), 2 * m, m) - 1.0
    count["log |f| < 2^-20"] = int((np.abs(f) < 2.0 ** -20).sum())
    count["log f == 0, k != 0"] = int(((f == 0) & (x != 1)).sum())
    count["log k == 0"] = int(((x > np.sqrt(0.5)) & (x < np.sqrt(2.0)) & (np.abs(f) >= 2.0 ** -20)).sum())
    count["log k != 0"] = int((((x < 0.7) | (x > 1.5)) & (np.abs(f) >= 2.0 ** -20)).sum())
    assert all(v >= 20 for v in count.values()), count


# ------------------------------------------------------------------------------------- the functions themselves ---
def family_ids():
    return [(op, name) for op in (SIN, COS, ACOS, ATAN2, LOG) for name in MC.families(op)]


@pytest.fixture(scope="module")
def host_errors(O):
    """op -> {family: (count, worst error, worst argument)}: one oracle call and one reference per op, shared by all cases."""
    cache = {}

    def get(op):
        if op not in cache:
            a, b, _ = MC.concatenated(op)
            cache[op] = {name: (n, w, arg) for name, n, w, arg in MR.family_errors(op, O.math_array(op, a, b))}
        return cache[op]
    return get


@pytest.mark.parametrize("op,family", family_ids(), ids=["%s-%s" % (MR.NAMES[op], name) for op, name in family_ids()])
def test_host_math_within_its_bound_of_the_exact_value(host_errors, op, family):
    n, w, arg = host_errors(op)[family]
    print("%s, %s: %d arguments, worst %.3f ulp at %s" % (MR.NAMES[op], family, n, w, arg))
    assert w < MR.BOUNDS[op], "%s, %s: %.3f ulp at %s (bound: under %g)" % (MR.NAMES[op], family, w, arg, MR.BOUNDS[op])


def test_sin_is_zero_and_cos_is_one_from_2p52_on(O):
    """A deliberate deviation from the reference's libm: a finite |x| >= 2^52 is an integer with no fraction left
    worth having, and the header reduces it to the remainder +0 in quadrant 0: sin_(x) = +0 — for a negative x too, the sign
    is not carried — and cos_(x) = 1. Pinned as the header has it; this file changes nothing there."""
    x = MC.sincos_at_or_above_2p52()
    assert np.all(np.abs(x) >= 2.0 ** 52) and np.all(np.isfinite(x)) and (np.abs(x) == 2.0 ** 52).sum() == 2 and (x < 0).sum() == len(x) // 2
    s, c = O.math_array(SIN, x), O.math_array(COS, x)
    assert np.all(s == 0.0) and not np.signbit(s).any()
    assert np.all(c == 1.0)
    below = np.nextafter(2.0 ** 52, 0.0)                                   # and not one double sooner
    assert MR.ulp_errors(O.math_array(SIN, [below, -below]), MR.exact(SIN, [below, -below])).max() < 1.0


@pytest.mark.parametrize("op", [SQRT, DIV])
def test_host_sqrt_and_division_are_ieee(O, op):
    for name, (a, b) in MC.families(op).items():
        with np.errstate(all="ignore"):
            want = np.sqrt(a) if op == SQRT else a / b
        got = O.math_array(op, a, b)
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = ~np.isnan(want)
        bad = np.flatnonzero(MC.to_bits(got[ok]) != MC.to_bits(want[ok]))
        assert len(bad) == 0, (name, a[ok][bad[0]].hex(), None if b is None else b[ok][bad[0]].hex())
