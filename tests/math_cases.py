"""The arguments tests/test_math_ref.py, tests/test_math_edges_gpu.py and tools/math_report.py put rt_math.h through.

numpy and Python integers only, deterministic: `families(op)` is an ordered dict  name -> (a, b)  (b is None for the unary
functions) of the places where these algorithms switch branch, cancel or leave the normal range, so that a failure can name
the family and its worst argument. Ops are numbered as the oracle's rto_math_op and the device probe number them:
0 sin, 1 cos, 2 acos, 3 atan2 (a = y, b = x), 4 log, 5 sqrt, 6 '/' (a / b)."""
import collections
import functools

import numpy as np

SIN, COS, ACOS, ATAN2, LOG, SQRT, DIV = range(7)
OPS = (SIN, COS, ACOS, ATAN2, LOG, SQRT, DIV)

# floor(pi/2 * 2^256): enough bits to round k * pi/2 to the nearest double for every k < 2^52 (tests/test_math_ref.py holds
# the constant itself to mpmath).
PIO2_BITS = 256
PIO2_INT = 0x1921FB54442D18469898CC51701B839A252049C1114CF98E804177D4C76273644

INF, NAN = np.inf, np.nan
TINY = 2.0 ** -1074                                  # the smallest subnormal
SUB_MAX = 2.0 ** -1022 - 2.0 ** -1074                # the largest


def _f(values):
    return np.array(values, dtype=np.float64)


def from_bits(u):
    return np.array(u, dtype=np.uint64).view(np.float64)


def to_bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def neighbours(x, n):
    """x and its n nearest doubles on either side (x finite, and not within n doubles of zero or infinity)."""
    u = to_bits(np.atleast_1d(_f(x))).astype(np.int64)
    return (u[:, None] + np.arange(-n, n + 1, dtype=np.int64)[None, :]).ravel().astype(np.uint64).view(np.float64)


def both_signs(x):
    x = _f(x)
    return np.concatenate([x, -x])


def random_signs(rng, x):
    return np.where(rng.integers(0, 2, len(x)) == 1, -x, x)


def binade_draws(rng, e_lo, e_hi, per):
    """`per` doubles with random sign in each binade [2^e, 2^(e+1)), e_lo <= e <= e_hi, subnormal binades included."""
    out = []
    for e in range(e_lo, e_hi + 1):
        frac = rng.integers(0, 1 << 52, per, dtype=np.uint64)
        if e >= -1022:
            u = (np.uint64(e + 1023) << np.uint64(52)) | frac
        else:
            top = e + 1074                                   # the subnormal's leading bit
            u = (np.uint64(1) << np.uint64(top)) | (frac & np.uint64((1 << top) - 1))
        out.append(u)
    return random_signs(rng, from_bits(np.concatenate(out)))


def log_uniform_ints(rng, lo, hi, n):
    """n integers spread log-uniformly over [lo, hi)."""
    k = np.exp2(rng.uniform(np.log2(lo), np.log2(hi), n)).astype(np.int64)
    return np.clip(k, lo, hi - 1)


def nearest_multiple_of_pio2(k, num=1, den=1):
    """The double nearest k * (num / den) * pi/2, by integer arithmetic (Python's int / int is correctly rounded)."""
    return _f([(int(v) * num * PIO2_INT) / (den << PIO2_BITS) for v in k])


K_RANGES = (("k<2^20", 1, 1 << 20), ("k=2^20..2^30", 1 << 20, 1 << 30), ("k=2^30..2^40", 1 << 30, 1 << 40), ("k=2^40..2^51", 1 << 40, 1 << 51))


def _sincos_families():
    rng = np.random.default_rng(20221)
    fam = collections.OrderedDict()
    fam["zeros and subnormals"] = both_signs([0.0, TINY, 3 * TINY, 2.0 ** -1050, SUB_MAX])
    fam["every binade 2^-1074..2^52"] = binade_draws(rng, -1074, 51, 3)
    # rem_pio2's branch edges: high words 0x3fe921fb (pi/4) and 0x413921fb (2^20 * pi/2), and 2^52
    fam["edge pi/4"] = both_signs(neighbours(from_bits([0x3FE921FB00000000, 0x3FE921FB54442D18, 0x3FE921FC00000000]), 8))
    fam["edge 2^20*pi/2"] = both_signs(neighbours(from_bits([0x413921FB00000000, 0x413921FB54442D18, 0x413921FC00000000]), 8))
    below_2p52 = neighbours(from_bits([0x4330000000000000]), 8)
    fam["edge 2^52, below"] = both_signs(below_2p52[below_2p52 < 2.0 ** 52])
    for name, lo, hi in K_RANGES:
        k = log_uniform_ints(rng, lo, hi, 1200)
        x = nearest_multiple_of_pio2(k)
        fam["nearest k*pi/2, " + name] = random_signs(rng, neighbours(x, 1))
        # the same k * pi/2, moved off by 2^-17 .. 2^-48 of itself: the remainder loses 17 .. 48 bits, not all 53
        k = log_uniform_ints(rng, max(lo, 4), hi, 64 * 32)
        x = nearest_multiple_of_pio2(k)
        off = np.exp2(-np.tile(np.arange(17, 49), 64).astype(np.float64))
        fam["k*pi/2 * (1 +- 2^-17..-48), " + name] = random_signs(rng, x * (1.0 + random_signs(rng, off)))
        # half way between two multiples: where a quotient rounded in double precision picks the wrong neighbour
        k = log_uniform_ints(rng, lo, hi, 300)
        x = nearest_multiple_of_pio2(2 * k + 1, 1, 2)
        fam["nearest (k+1/2)*pi/2, " + name] = random_signs(rng, neighbours(x, 1))
    # the top binade, where the quotient's ulp is 1/2: the only place where its rounding can outweigh 2/pi's own (upward)
    # rounding and name the multiple below
    k = log_uniform_ints(rng, 1 << 51, 2866000000000000, 600)
    fam["(k+1/2)*pi/2 and 2 neighbours, k=2^51..2^52*2/pi"] = random_signs(rng, neighbours(nearest_multiple_of_pio2(2 * k + 1, 1, 2), 2))
    for name, lo, hi in (("1e5..1.6e6", 1e5, 1.6e6), ("1.7e6..1e9", 1.7e6, 1e9), ("1e9..1e15", 1e9, 1e15), ("1e15..2^52", 1e15, 2.0 ** 52)):
        x = rng.uniform(lo, hi, 2000)
        fam["uniform " + name] = random_signs(rng, x[x < 2.0 ** 52])
    fam["inf and nan"] = _f([INF, -INF, NAN])
    return fam


def _sincos_at_or_above_2p52():
    """Finite |x| >= 2^52, where the header defines sin_ = 0 (signed like x) and cos_ = 1: pinned by a test of its own."""
    rng = np.random.default_rng(20222)
    up = neighbours(from_bits([0x4330000000000000]), 8)
    return both_signs(np.concatenate([up[up >= 2.0 ** 52], binade_draws(rng, 52, 1023, 1), _f([2.0 ** 53, 1e300, np.finfo(np.float64).max])]))


def _acos_families():
    rng = np.random.default_rng(20223)
    fam = collections.OrderedDict()
    k = np.arange(1, 54).astype(np.float64)
    fam["+-1"] = _f([1.0, -1.0])
    fam["+-(1 - 2^-k), k = 1..53"] = both_signs(1.0 - np.exp2(-k))
    fam["16 doubles either side of +-0.5"] = both_signs(neighbours([0.5], 16))
    fam["zeros, subnormals, 2^-k down to 2^-60"] = both_signs(np.concatenate([_f([0.0, TINY, SUB_MAX, 2.0 ** -1022]), np.exp2(-np.arange(1, 61).astype(np.float64)),
                                                                              neighbours(from_bits([0x3C60000000000000 + (1 << 32)]), 4)]))
    fam["uniform (-1, 1)"] = rng.uniform(-1.0, 1.0, 20000)
    fam["uniform in 1 - |x| down to 2^-40"] = random_signs(rng, 1.0 - np.exp2(rng.uniform(-40, -1, 4000)))
    fam["outside [-1, 1], inf, nan"] = _f([np.nextafter(1.0, 2.0), -np.nextafter(1.0, 2.0), 1.5, -1.5, 1e300, INF, -INF, NAN])
    return fam


def _atan2_families():
    rng = np.random.default_rng(20224)
    fam = collections.OrderedDict()
    v = _f([0.0, -0.0, 1.5, -1.5, TINY, -TINY, 1e300, -1e300, 1.0, -1.0, INF, -INF, NAN])
    fam["Annex F.9.1.4 table"] = (np.repeat(v, len(v)), np.tile(v, len(v)))
    # |y / x| at atan's breakpoints and at atan2's exponent-difference cuts, with the quotient's neighbours
    ratios = [7 / 16, 11 / 16, 19 / 16, 39 / 16] + [2.0 ** e for e in (-67, -66, -65, -62, -61, -60, -59, -28, -27, -26, 59, 60, 61, 62, 65, 66, 67)]
    ys, xs = [], []
    for x0 in (1.0, 3.0, 0.7, 1.0e10, 2.0 ** -500):
        for r in ratios:
            y = neighbours([r * x0], 4)
            for sy in (1.0, -1.0):
                for sx in (1.0, -1.0):
                    ys.append(sy * y)
                    xs.append(np.full(len(y), sx * x0))
    fam["breakpoints 7/16 11/16 19/16 39/16, 2^+-27, 2^+-60, 2^+-66"] = (np.concatenate(ys), np.concatenate(xs))
    sub = np.abs(binade_draws(rng, -1074, -1023, 8))
    nrm = np.exp2(rng.uniform(-1000, 1000, len(sub)))
    fam["subnormal y, normal x"] = (random_signs(rng, sub), random_signs(rng, nrm))
    fam["normal y, subnormal x"] = (random_signs(rng, nrm), random_signs(rng, sub))
    fam["subnormal y and x"] = (random_signs(rng, sub), random_signs(rng, rng.permutation(sub)))
    big, small = 1e300 * rng.uniform(0.5, 1.5, 200), 1e-300 * rng.uniform(0.5, 1.5, 200)
    fam["quotient overflows"] = (random_signs(rng, big), random_signs(rng, small))
    fam["quotient underflows"] = (random_signs(rng, small), random_signs(rng, big))
    ang = rng.uniform(-np.pi, np.pi, 8000)
    rad = np.exp2(rng.uniform(-300, 300, len(ang)))
    fam["every quadrant, radii 2^-300..2^300"] = (rad * np.sin(ang), rad * np.cos(ang))
    fam["near the axes"] = (random_signs(rng, np.exp2(rng.uniform(-70, 0, 4000))), random_signs(rng, np.exp2(rng.uniform(-70, 0, 4000))))
    fam["uniform (-3, 3)^2"] = (rng.uniform(-3, 3, 20000), rng.uniform(-3, 3, 20000))
    return fam


def _log_families():
    rng = np.random.default_rng(20225)
    fam = collections.OrderedDict()
    k = np.arange(1, 4097).astype(np.float64)
    fam["RNG grid k*2^-53, k = 1..4096"] = k * 2.0 ** -53
    fam["RNG grid k*2^-53, k = 2^53-4096..2^53-1"] = (2.0 ** 53 - k[::-1]) * 2.0 ** -53
    fam["powers of two"] = np.exp2(np.arange(-1074, 1024).astype(np.float64))
    e = np.arange(1, 54).astype(np.float64)
    fam["1 +- 2^-k"] = np.concatenate([1.0 + np.exp2(-e[:52]), 1.0 - np.exp2(-e)])
    fam["neighbours of sqrt(2)/2, sqrt(2), 1 +- 2^-20, e"] = neighbours([np.sqrt(0.5), np.sqrt(2.0), 1.0 + 2.0 ** -20, 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -21, 2.718281828459045,
                                                                          from_bits([0x3FF6A09E00000000])[0], from_bits([0x3FE6A09E00000000])[0]], 16)
    fam["subnormals"] = np.concatenate([_f([TINY, 2 * TINY, 3 * TINY, SUB_MAX, 2.0 ** -1022]), np.abs(binade_draws(rng, -1074, -1023, 8))])
    fam["every binade"] = np.abs(binade_draws(rng, -1022, 1023, 4))
    fam["uniform (0.5, 2)"] = rng.uniform(0.5, 2.0, 8000)
    fam["zeros, negatives, inf, nan"] = _f([0.0, -0.0, -TINY, -1.0, -1e300, -INF, INF, NAN])
    return fam


def _sqrt_families():
    rng = np.random.default_rng(20226)
    fam = collections.OrderedDict()
    fam["subnormal operands"] = np.concatenate([_f([TINY, 2 * TINY, SUB_MAX]), np.abs(binade_draws(rng, -1074, -1023, 20))])
    fam["every binade"] = np.abs(binade_draws(rng, -1022, 1023, 4))
    n = rng.integers(1, 1 << 26, 3000).astype(np.float64)
    fam["exact squares and their neighbours"] = neighbours(n * n, 2)
    p = np.exp2(np.arange(-500, 501, 3).astype(np.float64))
    fam["results that round up to a power of two"] = neighbours(p * p, 3)
    fam["uniform (0, 4)"] = rng.uniform(0.0, 4.0, 8000)
    fam["zeros, negatives, inf, nan, max"] = _f([0.0, -0.0, -TINY, -1.0, -INF, INF, NAN, np.finfo(np.float64).max])
    return {k: (v, None) for k, v in fam.items()}


def _div_families():
    rng = np.random.default_rng(20227)
    fam = collections.OrderedDict()
    sub = np.abs(binade_draws(rng, -1074, -1023, 20))
    nrm = rng.uniform(0.5, 2.0, len(sub))
    fam["subnormal operands"] = (random_signs(rng, sub), random_signs(rng, rng.permutation(sub)))
    fam["subnormal over normal, normal over subnormal"] = (np.concatenate([sub, nrm]), np.concatenate([random_signs(rng, nrm), sub]))
    a = rng.uniform(1.0, 2.0, 4000)
    b = rng.uniform(1.0, 2.0, 4000)
    fam["subnormal results"] = (a * 2.0 ** -600, random_signs(rng, b * np.exp2(rng.integers(420, 476, 4000).astype(np.float64))))
    fam["results that overflow or just do not"] = (random_signs(rng, a * 2.0 ** 600), b * np.exp2(-rng.integers(420, 426, 4000).astype(np.float64)))
    q = np.exp2(rng.integers(-1000, 1000, 2000).astype(np.float64))
    d = rng.uniform(1.0, 2.0, 2000)
    fam["results that round up to a power of two"] = (neighbours(q * d, 3), np.repeat(d, 7))
    fam["uniform (-3, 3)^2"] = (rng.uniform(-3, 3, 8000), rng.uniform(-3, 3, 8000))
    v = _f([0.0, -0.0, 1.0, -2.0, TINY, INF, -INF, NAN, np.finfo(np.float64).max])
    fam["zeros, inf, nan"] = (np.repeat(v, len(v)), np.tile(v, len(v)))
    return fam


@functools.lru_cache(maxsize=None)
def families(op):
    """name -> (a, b) for one op; arrays are built once and set read-only, so every user sees the same arguments."""
    if op in (SIN, COS):
        fam = {k: (v, None) for k, v in _sincos_families().items()}
    elif op == ACOS:
        fam = {k: (v, None) for k, v in _acos_families().items()}
    elif op == ATAN2:
        fam = _atan2_families()
    elif op == LOG:
        fam = {k: (v, None) for k, v in _log_families().items()}
    elif op == SQRT:
        fam = _sqrt_families()
    elif op == DIV:
        fam = _div_families()
    else:
        raise ValueError(op)
    out = collections.OrderedDict()
    for name, (a, b) in fam.items():
        a = np.ascontiguousarray(a, dtype=np.float64)
        a.setflags(write=False)
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.float64)
            assert a.shape == b.shape, name
            b.setflags(write=False)
        out[name] = (a, b)
    return out


@functools.lru_cache(maxsize=None)
def sincos_at_or_above_2p52():
    x = _sincos_at_or_above_2p52()
    x.setflags(write=False)
    return x


def concatenated(op):
    """All families of one op end to end: (a, b, [(name, start, stop), ...]) — one device call's worth."""
    parts, a, b, at = [], [], [], 0
    for name, (x, y) in families(op).items():
        parts.append((name, at, at + len(x)))
        at += len(x)
        a.append(x)
        if y is not None:
            b.append(y)
    return np.concatenate(a), (np.concatenate(b) if b else None), parts
