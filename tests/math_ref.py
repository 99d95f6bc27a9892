"""A multiprecision reference for rt_math.h's sin / cos / acos / atan2 / log, and the error measure the tests hold them to.

Every GPU test compares the HIP path with the CPU oracle, and both compile the same rt_math.h: a wrong sin_ is wrong on both
sides. This module shares no code with either (it imports nothing from oracle/, raytracer_2022_amd/ or _ffi): the reference
is mpmath at PREC bits — 400, because a double next to k * pi/2 with k near 2^50 cancels more than 100 bits before the first
bit of the result appears — and tests/test_math_ref.py pins the measure itself before anything is measured with it.

`exact(op, a, b)` gives one entry per argument: an mpf where the true result is finite and not zero, else a Python float that
stands for a class — nan, +-inf, or a zero with its sign (sin(+-0), log(1), acos(1), the zeros of C99 Annex F.9.1.4).
`ulp_errors(got, ref)` is |got - exact| / 2^(max(floor(log2 |exact|), -1022) - 52): the ulp of the EXACT value, not the
spacing of a rounded double (the two differ at binade edges and in the subnormals). A class entry costs 0 when `got` is that
class (NaN as a class, infinities and zeros by sign) and inf when it is not."""
import functools
import math

import mpmath
import numpy as np

import math_cases

PREC = 400
SIN, COS, ACOS, ATAN2, LOG, SQRT, DIV = range(7)
NAMES = {SIN: "sin", COS: "cos", ACOS: "acos", ATAN2: "atan2", LOG: "log", SQRT: "sqrt", DIV: "div"}


def _mp(x):
    return mpmath.mpf(float(x))


def _signed(v, negative):
    return -v if negative else v


def _neg(x):
    return math.copysign(1.0, x) < 0


def _sin(x):
    if math.isnan(x) or math.isinf(x):
        return math.nan
    return x if x == 0 else mpmath.sin(_mp(x))


def _cos(x):
    if math.isnan(x) or math.isinf(x):
        return math.nan
    return mpmath.cos(_mp(x))


def _acos(x):
    if math.isnan(x) or abs(x) > 1:
        return math.nan
    return 0.0 if x == 1 else mpmath.acos(_mp(x))


def _log(x):
    if math.isnan(x) or x < 0:
        return math.nan
    if x == 0:
        return -math.inf
    if math.isinf(x):
        return math.inf
    return 0.0 if x == 1 else mpmath.log(_mp(x))


def _atan2(y, x):
    """C99 Annex F.9.1.4, case by case; mpmath only where both arguments are finite and not zero."""
    if math.isnan(x) or math.isnan(y):
        return math.nan
    s = _neg(y)
    pi = mpmath.pi()
    if y == 0:
        return _signed(pi, s) if _neg(x) else _signed(0.0, s)
    if x == 0:
        return _signed(pi / 2, s)
    if math.isinf(y):
        if math.isinf(x):
            return _signed(3 * pi / 4 if x < 0 else pi / 4, s)
        return _signed(pi / 2, s)
    if math.isinf(x):
        return _signed(pi, s) if x < 0 else _signed(0.0, s)
    return mpmath.atan2(_mp(y), _mp(x))


_UNARY = {SIN: _sin, COS: _cos, ACOS: _acos, LOG: _log}


def exact(op, a, b=None, prec=PREC):
    """The true results of `op` on the doubles a (and b): a list of mpf / class floats (see the module's docstring)."""
    a = np.asarray(a, dtype=np.float64).ravel()
    with mpmath.workprec(prec):
        if op == ATAN2:
            b = np.asarray(b, dtype=np.float64).ravel()
            return [+_atan2(float(y), float(x)) for y, x in zip(a, b)]
        f = _UNARY[op]
        return [+f(float(x)) for x in a]


def ulp_of(e):
    """The ulp of a double format stretched over the exact value e (an mpf, not zero): 2^(max(floor(log2 |e|), -1022) - 52)."""
    exponent = mpmath.frexp(e)[1] - 1                       # |e| = m * 2^exp with 0.5 <= m < 1
    return mpmath.ldexp(mpmath.mpf(1), max(exponent, -1022) - 52)


def ulp_error(got, e, prec=PREC):
    """The error of the double `got` against one entry of exact(), in ulps of the exact value, as a float (inf: wrong class)."""
    got = float(got)
    if isinstance(e, float):
        if math.isnan(e):
            return 0.0 if math.isnan(got) else math.inf
        return 0.0 if (got == e and _neg(got) == _neg(e)) else math.inf
    if math.isnan(got) or math.isinf(got):
        return math.inf
    with mpmath.workprec(prec):
        return float(abs(mpmath.mpf(got) - e) / ulp_of(e))


def ulp_errors(got, ref, prec=PREC):
    got = np.asarray(got, dtype=np.float64).ravel()
    assert len(got) == len(ref)
    return np.array([ulp_error(g, e, prec) for g, e in zip(got, ref)], dtype=np.float64)


def failures(got, ref, bound, prec=PREC):
    """Indices whose error is not under `bound` ulps (a wrong class never is)."""
    return np.flatnonzero(~(ulp_errors(got, ref, prec) < bound))


BOUNDS = {SIN: 1.0, COS: 1.0, ACOS: 1.0, LOG: 1.0, ATAN2: 2.0}
"""Ulps, strictly under. sin / cos / acos / log: fdlibm's stated bound for these algorithms. atan2: atan is under 1 ulp; the
quotient's half ulp enters atan with a condition number of at most 1; the quadrant step pi - (z - pi_lo) rounds once more."""


@functools.lru_cache(maxsize=None)
def family_reference(op):
    """exact() over math_cases.concatenated(op), computed once per process and shared: (a, b, parts, ref)."""
    a, b, parts = math_cases.concatenated(op)
    return a, b, parts, exact(op, a, b)


def family_errors(op, got):
    """[(family, count, worst error, worst argument in hex)] of one result vector over concatenated(op)."""
    a, b, parts, ref = family_reference(op)
    err = ulp_errors(got, ref)
    rows = []
    for name, lo, hi in parts:
        w, arg = worst(err[lo:hi], a[lo:hi], None if b is None else b[lo:hi])
        rows.append((name, hi - lo, w, arg))
    return rows


def nearest(ref):
    """Each entry of exact() rounded to the nearest double."""
    return np.array([float(e) for e in ref], dtype=np.float64)


def hexd(x):
    return float(x).hex()


def worst(err, a, b=None):
    """(worst error, its argument in hex) of an error vector — what a failure and tools/math_report.py print."""
    if len(err) == 0:
        return 0.0, "-"
    i = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
    arg = hexd(a[i]) if b is None else "%s, %s" % (hexd(a[i]), hexd(b[i]))
    return float(err[i]), arg


def pio2_quotient(x, prec=PREC):
    """(n, y) with x = n * pi/2 + y exactly (to prec bits), n the nearest integer: the reduction rem_pio2 approximates."""
    with mpmath.workprec(prec):
        h = mpmath.pi() / 2
        n = mpmath.nint(_mp(x) / h)
        return int(n), _mp(x) - n * h


def exponent_drop(x, y):
    """Binary exponent of the double x minus that of its exact remainder y (an mpf): what rem_pio2 holds against 16 and 49."""
    if y == 0:
        return 10 ** 6
    return (math.frexp(x)[1] - 1) - (mpmath.frexp(y)[1] - 1)
