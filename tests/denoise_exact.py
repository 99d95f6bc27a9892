"""A third statement of the two denoisers (rt_denoise*, rt_denoise_dual*), written from the prose of include/rt2022.h alone:
one plain loop over the pixels and their taps, the same code for three kinds of number. It shares nothing with the kernels
or with the numpy restatements (tests/denoise_ref.py, tests/denoise_dual_ref.py): it imports neither them, nor the package,
nor the oracle, and takes plain arrays and plain numbers — the caller unpacks the feature records. No GPU is needed.

The kinds of number:

  Float64()      IEEE doubles, one operation after the other in the header's order: the definition itself. The numpy
                 restatements must give these bits (tests/test_denoise_ref.py).
  Interval53()   mpmath.iv at 53 bits: every + - * / returns an interval, rounded outwards to doubles, that holds the result
                 for every choice of operands from the operand intervals. The inputs enter as points. By induction over the
                 operations the result interval of an output value holds the exact real value of the definition AND every
                 round-to-nearest double evaluation of it, in any order of the taps (a sum's interval does not depend on what
                 a correctly rounded addition does inside it; reordering the additions changes which intermediate intervals
                 occur, not that each holds its double). The definition divides only by sp, by m >= albedo_floor > 0, by a
                 product of factors >= 1, by (u_p + u_q) + var_floor > 0 and by sw >= 9/64: no interval ever straddles a
                 zero denominator. The one comparison, a_j > albedo_floor, must be decided by the interval; a buffer where
                 it is not is refused (Undecided), never guessed. Finite inputs only.
  Mpf(200)       mpmath.mpf at 200 bits: the exact value to 1e-60, which pins the enclosure (it must lie inside every
                 interval, and must leave it when an input moves).

A result is a numpy object array of such numbers in buffer order; `floats`, `bounds` and `rel_width` read it."""
import math

import mpmath
import numpy as np

H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)     # the B3 spline; every product of two is exact


class Undecided(Exception):
    """An interval that does not decide a_j > albedo_floor."""


class Float64:
    name = "float64"

    def num(self, x):
        return np.float64(x)

    def is_nan(self, x):
        return bool(x != x)

    def above(self, a, b):
        return bool(a > b)


class Interval53:
    name = "interval, 53 bits"

    def __init__(self):
        self.ctx = mpmath.iv
        self.ctx.prec = 53

    def num(self, x):
        if not math.isfinite(x):
            raise ValueError("the enclosure is for finite inputs")
        return self.ctx.mpf(float(x))                      # a double is a point: no rounding

    def is_nan(self, x):
        return False

    def above(self, a, b):
        if a.a > b.b:
            return True
        if a.b <= b.a:
            return False
        raise Undecided("albedo %s against floor %s" % (a, b))


class Mpf:
    def __init__(self, bits=200):
        self.ctx = mpmath.mp.clone()
        self.ctx.prec = bits
        self.name = "mpf, %d bits" % bits

    def num(self, x):
        if not math.isfinite(x):
            raise ValueError("the multiprecision loop is for finite inputs")
        return self.ctx.mpf(float(x))

    def is_nan(self, x):
        return False

    def above(self, a, b):
        return bool(a > b)


# ---- the pieces both filters share ------------------------------------------------------------------------------------------
def _inv(K, sigma, scale=1.0):
    """1.0 / (s * s) with s = sigma * scale; a sigma of +inf switches its term off: 0."""
    if sigma == math.inf:
        return K.num(0.0)
    s = K.num(sigma) * K.num(scale)
    return K.num(1.0) / (s * s)


def _dist(p, q):
    d0, d1, d2 = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return (d0 * d0 + d1 * d1) + d2 * d2


def _buffer_row_of(height, rows):
    """at[y] = the buffer row that holds image row y: buffer row i is image row rows[i]."""
    if rows is None:
        return list(range(height))
    at = [None] * height
    for i, r in enumerate(rows):
        assert 0 <= int(r) < height and at[int(r)] is None, "not a permutation of the image's rows"
        at[int(r)] = i
    assert len(rows) == height
    return at


def _taps(K, width, height, x, y, step):
    """The taps of pixel (x, y) that fall inside the image, rows first (j), then columns (i): (h_j * h_i, qx, qy)."""
    for j in range(-2, 3):
        qy = y + j * step
        if qy < 0 or qy >= height:
            continue
        for i in range(-2, 3):
            qx = x + i * step
            if qx < 0 or qx >= width:
                continue
            yield K.hh[j + 2][i + 2], qx, qy


def _prepare_kind(K):
    K.hh = [[K.num(H5[j] * H5[i]) for i in range(5)] for j in range(5)]
    K.one, K.zero, K.half = K.num(1.0), K.num(0.0), K.num(0.5)


def _mean(K, s, sp):
    return (K.zero if K.is_nan(s) else s) / sp


def _modulation(K, a, floor, demodulate):
    if not demodulate:
        return [K.one, K.one, K.one]
    return [aj if K.above(aj, floor) else floor for aj in a]     # a NaN albedo is not above anything: the floor


def _guide_factors(K, G, p, q, inv_n, inv_z, inv_a):
    """(1 + dn*inv_n, 1 + (dz*dz)*inv_z, 1 + da*inv_a) between the pixels p and q = (x, y) of the guide grids G."""
    A, N, Z = G
    (px, py), (qx, qy) = p, q
    dz = Z[py][px] - Z[qy][qx]
    return (K.one + _dist(N[py][px], N[qy][qx]) * inv_n, K.one + (dz * dz) * inv_z, K.one + _dist(A[py][px], A[qy][qx]) * inv_a)


def _grid(height, width):
    return [[None] * width for _ in range(height)]


def _quiet(f):
    """Doubles overflow to inf and turn 0 * inf into NaN as IEEE says, without numpy's warnings."""
    def g(*a, **kw):
        with np.errstate(all="ignore"):
            return f(*a, **kw)
    g.__doc__, g.__name__ = f.__doc__, f.__name__
    return g


# ---- rt_denoise -------------------------------------------------------------------------------------------------------------
@_quiet
def denoise(K, sums, albedo, normal, depth, *, spp, n_iter, sigma_color, sigma_normal, sigma_depth, sigma_albedo, albedo_floor,
            demodulate=True, rows=None):
    """rt_denoise on plain arrays in buffer order: sums, albedo, normal (H, W, 3) and depth (H, W), all sums of `spp` samples
    -> the filtered sums, an object array (H, W, 3) of K's numbers in buffer order."""
    _prepare_kind(K)
    height, width = len(sums), len(sums[0])
    at = _buffer_row_of(height, rows)
    sp, floor = K.num(float(spp)), K.num(albedo_floor)
    E, A, N, Z, M = (_grid(height, width) for _ in range(5))
    for y in range(height):
        for x in range(width):
            b = at[y]
            c = [_mean(K, K.num(sums[b][x][j]), sp) for j in range(3)]
            A[y][x] = [K.num(albedo[b][x][j]) / sp for j in range(3)]
            N[y][x] = [K.num(normal[b][x][j]) / sp for j in range(3)]
            Z[y][x] = K.num(depth[b][x]) / sp
            M[y][x] = _modulation(K, A[y][x], floor, demodulate)
            E[y][x] = [c[j] / M[y][x][j] for j in range(3)]
    inv_n, inv_z, inv_a = _inv(K, sigma_normal), _inv(K, sigma_depth), _inv(K, sigma_albedo)
    for k in range(n_iter):
        step = 2 ** k
        inv_c = _inv(K, sigma_color, 2.0 ** -k)            # sigma_k = sigma_color * 2^-k, an exact scaling
        nxt = _grid(height, width)
        for y in range(height):
            for x in range(width):
                sw, sv = K.zero, [K.zero, K.zero, K.zero]
                for hh, qx, qy in _taps(K, width, height, x, y, step):
                    eq = E[qy][qx]
                    fn, fz, fa = _guide_factors(K, (A, N, Z), (x, y), (qx, qy), inv_n, inv_z, inv_a)
                    den = (((K.one + _dist(E[y][x], eq) * inv_c) * fn) * fz) * fa
                    w = hh / den
                    sw = sw + w
                    sv = [sv[j] + w * eq[j] for j in range(3)]
                nxt[y][x] = [sv[j] / sw for j in range(3)]
        E = nxt
    out = np.empty((height, width, 3), dtype=object)
    for y in range(height):
        for x in range(width):
            for j in range(3):
                out[at[y], x, j] = (E[y][x][j] * M[y][x][j]) * sp
    return out


# ---- rt_denoise_dual --------------------------------------------------------------------------------------------------------
@_quiet
def denoise_dual(K, sum_a, sum_b, albedo_a, albedo_b, normal_a, normal_b, depth_a, depth_b, *, spp, n_iter, sigma_color,
                 sigma_normal, sigma_depth, sigma_albedo, albedo_floor, var_iter, var_floor, demodulate=True, rows=None):
    """rt_denoise_dual on plain arrays in buffer order, each half's sums of `spp` samples -> (the filtered sums of 2 * spp
    samples (H, W, 3), the residual variance (H, W)), object arrays of K's numbers in buffer order."""
    _prepare_kind(K)
    height, width = len(sum_a), len(sum_a[0])
    at = _buffer_row_of(height, rows)
    sp, floor, vfloor = K.num(float(spp)), K.num(albedo_floor), K.num(var_floor)
    sp2 = sp + sp
    E, U, A, N, Z, M = (_grid(height, width) for _ in range(6))
    for y in range(height):
        for x in range(width):
            b = at[y]
            ca = [_mean(K, K.num(sum_a[b][x][j]), sp) for j in range(3)]
            cb = [_mean(K, K.num(sum_b[b][x][j]), sp) for j in range(3)]
            A[y][x] = [(K.num(albedo_a[b][x][j]) + K.num(albedo_b[b][x][j])) / sp2 for j in range(3)]
            N[y][x] = [(K.num(normal_a[b][x][j]) + K.num(normal_b[b][x][j])) / sp2 for j in range(3)]
            Z[y][x] = (K.num(depth_a[b][x]) + K.num(depth_b[b][x])) / sp2
            m = M[y][x] = _modulation(K, A[y][x], floor, demodulate)
            E[y][x] = [((ca[j] + cb[j]) * K.half) / m[j] for j in range(3)]
            h = [((ca[j] - cb[j]) * K.half) / m[j] for j in range(3)]
            U[y][x] = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]
    inv_n, inv_z, inv_a = _inv(K, sigma_normal), _inv(K, sigma_depth), _inv(K, sigma_albedo)
    inv_c = _inv(K, sigma_color)                           # not halved: the propagated variance shrinks instead
    for t in range(var_iter):                              # the variance prefilter: guides only
        nxt = _grid(height, width)
        for y in range(height):
            for x in range(width):
                sw, sx = K.zero, K.zero
                for hh, qx, qy in _taps(K, width, height, x, y, 2 ** t):
                    fn, fz, fa = _guide_factors(K, (A, N, Z), (x, y), (qx, qy), inv_n, inv_z, inv_a)
                    w = hh / ((fn * fz) * fa)
                    sw = sw + w
                    sx = sx + w * U[qy][qx]
                nxt[y][x] = sx / sw
        U = nxt
    for k in range(n_iter):
        nxt_e, nxt_u = _grid(height, width), _grid(height, width)
        for y in range(height):
            for x in range(width):
                sw, su, sv = K.zero, K.zero, [K.zero, K.zero, K.zero]
                for hh, qx, qy in _taps(K, width, height, x, y, 2 ** k):
                    eq, uq = E[qy][qx], U[qy][qx]
                    fn, fz, fa = _guide_factors(K, (A, N, Z), (x, y), (qx, qy), inv_n, inv_z, inv_a)
                    r = (_dist(E[y][x], eq) * inv_c) / ((U[y][x] + uq) + vfloor)
                    den = (((K.one + r) * fn) * fz) * fa
                    w = hh / den
                    sw = sw + w
                    sv = [sv[j] + w * eq[j] for j in range(3)]
                    su = su + (w * w) * uq
                nxt_e[y][x] = [sv[j] / sw for j in range(3)]
                nxt_u[y][x] = su / (sw * sw)
        E, U = nxt_e, nxt_u
    out = np.empty((height, width, 3), dtype=object)
    var = np.empty((height, width), dtype=object)
    for y in range(height):
        for x in range(width):
            var[at[y], x] = U[y][x]
            for j in range(3):
                out[at[y], x, j] = (E[y][x][j] * M[y][x][j]) * sp2
    return out, var


# ---- reading a result -------------------------------------------------------------------------------------------------------
def floats(res):
    """A Float64 result as a float64 array."""
    return np.array(res.tolist(), dtype=np.float64).reshape(res.shape)


def bounds(res):
    """An Interval53 result as (lo, hi), float64 arrays: the end points are doubles already."""
    flat = res.reshape(-1)
    lo = np.array([float(v.a) for v in flat], dtype=np.float64).reshape(res.shape)
    hi = np.array([float(v.b) for v in flat], dtype=np.float64).reshape(res.shape)
    for v, l, h in zip(flat, lo.reshape(-1), hi.reshape(-1)):
        assert v.a == l and v.b == h, "an end point that is no double"
    return lo, hi


def rel_width(lo, hi):
    """(hi - lo) / the end point nearer zero; 0 for the interval [0, 0]; inf for any other interval that holds 0."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    small = np.minimum(np.abs(lo), np.abs(hi))
    with np.errstate(all="ignore"):
        w = np.where((lo == 0) & (hi == 0), 0.0, np.where((lo > 0) | (hi < 0), (hi - lo) / small, np.inf))
    return w


def inside(value, lo, hi):
    """Per element: lo <= value <= hi; where the interval is [0, 0] the value must be +0."""
    value = np.asarray(value, dtype=np.float64)
    ok = (lo <= value) & (value <= hi)
    zero = (lo == 0) & (hi == 0)
    return ok & (~zero | ~np.signbit(value))
