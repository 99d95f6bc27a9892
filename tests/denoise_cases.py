"""What the denoiser tests on the CPU (tests/test_denoise_ref.py), on the device (tests/test_denoise_exact_gpu.py) and
tools/denoise_report.py share: the ways to run a filter on plain arrays, the cases whose every value is held to the
enclosure of tests/denoise_exact.py, and closed forms of include/rt2022.h's definition. No GPU is needed here.

A *filter* is an object with
    single(sums, guides, prm, rows=None) -> out (H, W, 3)
    dual(sum_a, sum_b, guides_a, guides_b, prm, rows=None) -> (out (H, W, 3), variance (H, W))
where guides = (albedo (H, W, 3), normal (H, W, 3), depth (H, W)), all sums of prm["spp"] samples in buffer order, and prm
holds denoise_exact's keywords. Loop(kind) is denoise_exact's loop, Restated the numpy restatements, Library the host form
of the library, Device its device form on torch buffers.

Every closed form below is a function check_*(filt) that raises AssertionError. It is derived in its docstring from
h = (1, 4, 6, 4, 1) / 16 and the header's formulas, compares in exact rational arithmetic (a double and a 200-bit number
are both rationals), and is run on Loop(Mpf(200)) first: a closed form that the definition itself does not satisfy is a
mistake in the closed form. Tolerances are counted in ulps of the expected value (2^-52 of it) and come from the number of
roundings the definition makes, stated where they are used."""
import math
from fractions import Fraction as Fr

import numpy as np

import raytracer_2022_amd as rt
from raytracer_2022_amd import _ffi as F

import denoise_exact as X
from denoise_dual_ref import halves, restate_dual
from denoise_ref import buffers, restate

INF = math.inf
# The package's defaults (denoise_params, DUAL_DEFAULTS), written out: test_denoise_ref.py holds them to the package.
SINGLE = dict(spp=4, n_iter=5, sigma_color=1.0, sigma_normal=0.3, sigma_depth=INF, sigma_albedo=0.3, albedo_floor=1e-3, demodulate=True)
DUAL = dict(SINGLE, sigma_color=2.0, var_iter=1, var_floor=1e-6)
TIGHT = dict(sigma_color=0.3, sigma_normal=0.05, sigma_depth=0.1, sigma_albedo=0.01, albedo_floor=0.3)
TIGHT_DUAL = dict(TIGHT, sigma_color=0.5, var_floor=1e-12)
OFF = dict(sigma_color=INF, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)
PLAIN = dict(SINGLE, demodulate=False, **OFF)              # the plain spline on the radiance itself
PLAIN_DUAL = dict(DUAL, demodulate=False, var_iter=0, **OFF)


# ---- filters ----------------------------------------------------------------------------------------------------------------
def unpack(feat):
    f = np.asarray(feat)
    return f["albedo"], f["normal"], f["depth"]


def pack(guides):
    albedo, normal, depth = guides
    feat = np.zeros(np.asarray(depth).shape, dtype=F.FEATURE_DTYPE)
    feat["albedo"], feat["normal"], feat["depth"] = albedo, normal, depth
    return feat


def blocks(shape, prm):
    """(rt_denoise_params, rt_denoise_dual_params or None) of an (H, W, 3) image for prm."""
    kw = {k: prm[k] for k in ("n_iter", "sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo", "albedo_floor", "demodulate")}
    p = rt.denoise_params(shape[1], shape[0], prm["spp"], **kw)
    return p, (rt.denoise_dual_params(prm["var_iter"], prm["var_floor"]) if "var_iter" in prm else None)


class Loop:
    def __init__(self, kind):
        self.kind, self.name = kind, "loop, " + kind.name
        self.read = X.floats if isinstance(kind, X.Float64) else (lambda r: r)

    def single(self, sums, guides, prm, rows=None):
        return self.read(X.denoise(self.kind, sums, *guides, rows=rows, **prm))

    def dual(self, sum_a, sum_b, ga, gb, prm, rows=None):
        out, var = X.denoise_dual(self.kind, sum_a, sum_b, ga[0], gb[0], ga[1], gb[1], ga[2], gb[2], rows=rows, **prm)
        return self.read(out), self.read(var)


class Restated:
    name = "restatement"

    def single(self, sums, guides, prm, rows=None):
        return restate(sums, pack(guides), blocks(np.shape(sums), prm)[0], rows)

    def dual(self, sum_a, sum_b, ga, gb, prm, rows=None):
        return restate_dual(sum_a, sum_b, pack(ga), pack(gb), *blocks(np.shape(sum_a), prm), rows)


class Library:
    name = "library, host form"

    def single(self, sums, guides, prm, rows=None):
        return rt.denoise(sums, pack(guides), blocks(np.shape(sums), prm)[0], row_ids=rows)

    def dual(self, sum_a, sum_b, ga, gb, prm, rows=None):
        return rt.denoise_dual(sum_a, sum_b, pack(ga), pack(gb), *blocks(np.shape(sum_a), prm), row_ids=rows, want_variance=True)


class Device:
    """rt_denoise_device / rt_denoise_dual_device on torch buffers and the default stream; the workspace starts as 0xFF bytes."""
    name = "library, device form"

    def _up(self, *arrays):
        import torch
        self.torch = torch
        return [torch.from_numpy(np.ascontiguousarray(a).view(np.float64 if a.dtype == F.FEATURE_DTYPE else a.dtype).reshape(-1)).cuda()
                for a in arrays]

    def single(self, sums, guides, prm, rows=None):
        p = blocks(np.shape(sums), prm)[0]
        d_sums, d_feat = self._up(np.asarray(sums, dtype=np.float64), pack(guides))
        torch_ = self.torch
        d_out = torch_.full(np.shape(sums), 7.0, dtype=torch_.float64, device="cuda")
        d_ws = torch_.full((rt.denoise_workspace_bytes(p),), 0xFF, dtype=torch_.uint8, device="cuda")
        d_rows = None if rows is None else self._up(np.asarray(rows, dtype=np.uint32).view(np.int32))[0]
        torch_.cuda.synchronize()
        rt.denoise_device(d_sums.data_ptr(), d_feat.data_ptr(), p, d_out.data_ptr(), d_ws.data_ptr(),
                          d_row_ids_ptr=None if rows is None else d_rows.data_ptr())
        torch_.cuda.synchronize()
        return d_out.cpu().numpy()

    def dual(self, sum_a, sum_b, ga, gb, prm, rows=None):
        p, q = blocks(np.shape(sum_a), prm)
        d_sa, d_sb, d_fa, d_fb = self._up(np.asarray(sum_a, dtype=np.float64), np.asarray(sum_b, dtype=np.float64), pack(ga), pack(gb))
        torch_ = self.torch
        d_out = torch_.full(np.shape(sum_a), 7.0, dtype=torch_.float64, device="cuda")
        d_var = torch_.full(np.shape(sum_a)[:2], 7.0, dtype=torch_.float64, device="cuda")
        d_ws = torch_.full((rt.denoise_dual_workspace_bytes(p),), 0xFF, dtype=torch_.uint8, device="cuda")
        d_rows = None if rows is None else self._up(np.asarray(rows, dtype=np.uint32).view(np.int32))[0]
        torch_.cuda.synchronize()
        rt.denoise_dual_device(d_sa.data_ptr(), d_sb.data_ptr(), d_fa.data_ptr(), d_fb.data_ptr(), p, q, d_out.data_ptr(), d_ws.data_ptr(),
                               d_out_variance_ptr=d_var.data_ptr(), d_row_ids_ptr=None if rows is None else d_rows.data_ptr())
        torch_.cuda.synchronize()
        return d_out.cpu().numpy(), d_var.cpu().numpy()


# ---- the cases held to the enclosure ----------------------------------------------------------------------------------------
# name -> (filter, W, H, seed, parameters over the defaults, shuffled rows, B's noise relative to A or None: independent halves,
# run on the device too). The shapes: images smaller than the footprint; 12 x 9; 67 x 9 and 9 x 67 for a lane strip boundary
# in x and row groups of 4 in y. TIGHT's floor of 0.3 puts a third of the albedos under the floor.
def _cases():
    c = {}
    for W, H in ((1, 1), (1, 9), (9, 1), (5, 3)):
        c["single %dx%d" % (W, H)] = ("single", W, H, W * 16 + H, dict(n_iter=5), False, None, False)
        c["dual %dx%d" % (W, H)] = ("dual", W, H, W * 16 + H, dict(n_iter=5, var_iter=3), False, None, False)
    c["single 12x9 n1"] = ("single", 12, 9, 2, dict(n_iter=1), False, None, True)
    c["single 12x9 n3"] = ("single", 12, 9, 3, dict(n_iter=3), True, None, False)
    c["single 12x9 n5 tight"] = ("single", 12, 9, 4, dict(TIGHT, n_iter=5), False, None, True)
    c["single 12x9 n1 tight"] = ("single", 12, 9, 5, dict(TIGHT, n_iter=1), False, None, False)
    c["single 67x9 n5"] = ("single", 67, 9, 6, dict(n_iter=5), False, None, True)
    c["single 9x67 n5 tight rows"] = ("single", 9, 67, 7, dict(TIGHT, n_iter=5), True, None, True)
    c["dual 12x9 n1 v0"] = ("dual", 12, 9, 2, dict(n_iter=1, var_iter=0), False, 0.01, True)
    c["dual 12x9 n3 v1"] = ("dual", 12, 9, 3, dict(n_iter=3, var_iter=1), True, 0.1, False)
    c["dual 12x9 n5 v3 tight"] = ("dual", 12, 9, 4, dict(TIGHT_DUAL, n_iter=5, var_iter=3), False, 0.1, False)
    c["dual 12x9 n5 v1 tight"] = ("dual", 12, 9, 8, dict(TIGHT_DUAL, n_iter=5, var_iter=1), False, None, True)
    c["dual 12x9 n5 v1 same halves"] = ("dual", 12, 9, 5, dict(n_iter=5, var_iter=1), False, 0.0, False)
    c["dual 67x9 n5 v1"] = ("dual", 67, 9, 6, dict(n_iter=5, var_iter=1), False, 0.01, True)
    c["dual 9x67 n5 v0 tight rows"] = ("dual", 9, 67, 7, dict(TIGHT_DUAL, n_iter=5, var_iter=0), True, 0.01, True)
    return c


CASES = _cases()
GPU_CASES = [k for k, v in CASES.items() if v[7]]
WIDTH_CAP = 1e-12                                          # every compared value's relative interval width


def case_inputs(name):
    """-> (filter, args for the filter's method: arrays, parameters, rows)."""
    which, W, H, seed, over, shuffled, noise, _ = CASES[name]
    rows = np.random.default_rng(seed).permutation(H).astype(np.uint32) if shuffled else None
    if which == "single":
        sums, feat = buffers(W, H, seed=seed, hostile=False)
        return which, (sums, unpack(feat), dict(SINGLE, **over), rows)
    sa, sb, fa, fb = halves(W, H, seed=seed, hostile=False)
    if noise is not None:                                  # B is A with relative Gaussian noise on the sums, the guides shared
        sb, fb = sa * (1.0 + noise * np.random.default_rng(seed + 1).normal(size=sa.shape)), fa.copy()
    return which, (sa, sb, unpack(fa), unpack(fb), dict(DUAL, **over), rows)


_enclosures = {}


def enclosure(name):
    """The case's intervals, computed once per process: a list of (lo, hi), the colour's and for the dual the variance's."""
    if name not in _enclosures:
        which, args = case_inputs(name)
        res = getattr(Loop(X.Interval53()), which)(*args)
        _enclosures[name] = [X.bounds(r) for r in ((res,) if which == "single" else res)]
    return _enclosures[name]


def against_enclosure(name, filt):
    """Run the case through `filt` -> per output (what, largest relative width, worst |got - mid| / half-width, number of
    values outside). The caller asserts; tools/denoise_report.py prints."""
    which, args = case_inputs(name)
    got = getattr(filt, which)(*args)
    rows = []
    for what, g, (lo, hi) in zip(("colour", "variance"), (got,) if which == "single" else got, enclosure(name)):
        g = np.asarray(g, dtype=np.float64)
        assert g.shape == lo.shape
        half = (hi - lo) / 2
        with np.errstate(all="ignore"):
            off = np.where(half > 0, np.abs(g - (lo + half)) / half, np.where(g == lo, 0.0, np.inf))
            off = np.where(np.isnan(g), np.inf, off)
        rows.append((what, float(X.rel_width(lo, hi).max()), float(off.max()), int((~X.inside(g, lo, hi)).sum())))
    return rows


# ---- exact comparison -------------------------------------------------------------------------------------------------------
def frac(v):
    """A double or an mpmath number as the rational it is."""
    if hasattr(v, "_mpf_"):
        sign, man, exp, _ = v._mpf_
        assert man != 0 or exp == 0, "not finite"
        return (-1) ** sign * Fr(int(man)) * Fr(2) ** int(exp)
    assert math.isfinite(float(v)), "not finite"
    return Fr(float(v))


worst_ulps = {}                                            # what[0] -> the largest |got - want| seen, in ulps of want


def close(got, want, ulps, what=""):
    """|got - want| <= ulps * 2^-52 * |want|, in rationals."""
    g, w = frac(got), Fr(want)
    key = what[0] if isinstance(what, tuple) else what
    worst_ulps[key] = max(worst_ulps.get(key, 0.0), float(abs(g - w) / abs(w) * 2 ** 52) if w else 0.0)
    assert abs(g - w) <= ulps * Fr(1, 2 ** 52) * abs(w), (what, float(g), float(w), float(abs(g - w) / abs(w)) * 2 ** 52 if w else None)


def flat_guides(W, H, spp, albedo=(0.5, 0.5, 0.5), normal=(0.0, 0.0, 1.0), depth=3.0):
    a, n, z = np.empty((H, W, 3)), np.empty((H, W, 3)), np.full((H, W), depth * spp)
    a[...], n[...] = np.multiply(albedo, spp), np.multiply(normal, spp)
    return a, n, z


def random_guides(W, H, seed):
    return unpack(buffers(W, H, seed=seed, hostile=False)[1])


def _taken(n, at, step=1):
    """The offsets i in -2 .. 2 whose tap at + i*step lies in [0, n)."""
    return [i for i in range(-2, 3) if 0 <= at + i * step < n]


H16 = (1, 4, 6, 4, 1)                                      # h * 16


def h(i):
    return Fr(H16[i + 2], 16)


# ---- fixed point ------------------------------------------------------------------------------------------------------------
FIXED_ITERS = range(0, 7)


def check_fixed_point(filt, n_iter):
    """Constant colour over constant guides: every difference is 0, so every taken tap has den = 1 and w = hh, and
    e' = sum(hh e) / sum(hh) = e whatever taps the image holds — also at borders and corners, where sum(hh) < 1: the
    normalisation must be over the taps taken. out = ((c / m) * m) * sp returns the sums. The roundings: c / m, one sum of
    products and one quotient per iteration, the remodulation; the issue's bound is 4 ulp for n_iter 0 .. 6. The third
    albedo (0.0005 * spp) lies under the floor: the remodulation must multiply by the floor it divided by."""
    W, H, spp = 7, 5, 4
    sums = np.empty((H, W, 3))
    sums[...] = np.multiply((0.7, 0.3, 0.9), spp)
    guides = flat_guides(W, H, spp, albedo=(0.45, 0.25, 0.0005))
    out = filt.single(sums, guides, dict(SINGLE, n_iter=n_iter))
    for idx in np.ndindex(H, W, 3):
        close(out[idx], sums[idx], 4, ("fixed point", n_iter, idx))


def check_fixed_point_dual(filt, n_iter, var_iter):
    """The same on halves c + d and c - d: the colour comes back as A + B, and the variance estimate v0 = |d / m|^2 is one
    constant, which the prefilter (guides constant: w = hh) must leave constant through every pass: sx / sw = v0."""
    W, H, spp = 7, 5, 4
    c, d = np.multiply((0.7, 0.3, 0.9), spp), np.multiply((0.05, 0.02, 0.001), spp)
    sa, sb = np.empty((H, W, 3)), np.empty((H, W, 3))
    sa[...], sb[...] = c + d, c - d
    guides = flat_guides(W, H, spp, albedo=(0.45, 0.25, 0.0005))
    prm = dict(DUAL, n_iter=n_iter, var_iter=var_iter)
    out, var = filt.dual(sa, sb, guides, guides, prm)
    m = [Fr(0.45 * spp) / spp, Fr(0.25), Fr(prm["albedo_floor"])]
    v0 = sum(((Fr(sa[0, 0, j]) - Fr(sb[0, 0, j])) / spp / 2 / m[j]) ** 2 for j in range(3))
    for idx in np.ndindex(H, W, 3):
        close(out[idx], Fr(sa[idx]) + Fr(sb[idx]), 4, ("dual fixed point", n_iter, idx))
    if n_iter == 0:
        for idx in np.ndindex(H, W):                       # 9 roundings to v0, then sum, product and quotient per pass
            close(var[idx], v0, 8 + 4 * var_iter, ("constant variance", var_iter, idx))


# ---- impulse response -------------------------------------------------------------------------------------------------------
def spline_kernel(n_iter):
    """h (*) h^2 (*) h^4 ...: the 1-D response of n_iter plain iterations, as integers over 16^n_iter (np.convolve on
    integers: exact). Index r + R is offset r, R = 2 * (2^n_iter - 1)."""
    k = np.array([1], dtype=np.int64)
    for it in range(n_iter):
        up = np.zeros(4 * 2 ** it + 1, dtype=np.int64)
        up[:: 2 ** it] = H16
        k = np.convolve(k, up)
    return k, 16 ** n_iter


def check_impulse(filt, W, H, x0, y0, n_iter, dual=False):
    """All four sigmas off and no demodulation: w = hh, whatever the (random) guides hold. One pixel holds c, the others 0.
    Where the footprint of all n_iter iterations, 2 * (2^n - 1) pixels each way, lies inside the image, every sw along
    the way is sum(hh) = 1 and the result is the n-fold convolution: out(x, y) = K[y0 - y] * K[x0 - x] * c, K = h (*) h^2
    (*) h^4. All of it is dyadic with few bits, so doubles are exact: the comparison is for equality. A transposed index, a
    step of k + 1 or a sigma left on gives another pattern. The image is not square and the impulse off centre."""
    spp = 4
    c = (1.0, 2.0, 0.5)
    sums = np.zeros((H, W, 3))
    sums[y0, x0] = np.multiply(c, spp)
    g = random_guides(W, H, 21)
    if dual:
        out, var = filt.dual(sums, sums.copy(), g, g, dict(PLAIN_DUAL, n_iter=n_iter))
        scale = 2 * spp
    else:
        out, scale = filt.single(sums, g, dict(PLAIN, n_iter=n_iter)), spp
    K, den = spline_kernel(n_iter)
    R = 2 * (2 ** n_iter - 1)
    assert 2 * R + 1 <= min(W, H), "no pixel has its whole footprint inside"
    seen = 0
    for y in range(R, H - R):
        for x in range(R, W - R):
            ky = int(K[y0 - y + R]) if abs(y0 - y) <= R else 0
            kx = int(K[x0 - x + R]) if abs(x0 - x) <= R else 0
            seen += ky * kx != 0
            for j in range(3):
                assert frac(out[y, x, j]) == Fr(ky * kx, den * den) * Fr(c[j]) * scale, ("impulse", n_iter, x, y, j)
            if dual:
                assert frac(var[y, x]) == 0
    assert seen > 1


def check_impulse_borders(filt, dual=False):
    """One iteration, the impulse in a corner region, EVERY pixel: out(p) = hh(q0 - p) * c / sw(p) with sw(p) the sum of
    hh over the taps the image holds, (sum of taken h_j) * (sum of taken h_i). Numerator and denominator are exact in
    doubles, so the definition's value is the correctly rounded quotient: 1 ulp. Clamped taps count the corner twice."""
    W, H, spp, x0, y0 = 9, 6, 4, 1, 0
    c = (1.0, 2.0, 0.5)
    sums = np.zeros((H, W, 3))
    sums[y0, x0] = np.multiply(c, spp)
    g = random_guides(W, H, 22)
    if dual:
        out, scale = filt.dual(sums, sums.copy(), g, g, dict(PLAIN_DUAL, n_iter=1))[0], 2 * spp
    else:
        out, scale = filt.single(sums, g, dict(PLAIN, n_iter=1)), spp
    for y in range(H):
        for x in range(W):
            sw = sum(h(j) for j in _taken(H, y)) * sum(h(i) for i in _taken(W, x))
            hh = h(y0 - y) * h(x0 - x) if abs(y0 - y) <= 2 and abs(x0 - x) <= 2 else Fr(0)
            for j in range(3):
                close(out[y, x, j], hh * Fr(c[j]) / sw * scale, 1, ("impulse at the border", x, y, j))


# ---- linear ramp ------------------------------------------------------------------------------------------------------------
def check_ramp(filt, dual=False):
    """Same switches. h is symmetric with sum 1, so a colour linear in x and y is a fixed point wherever the whole footprint
    is inside. The coefficients are dyadic: every product and sum is exact, the comparison is for equality (tighter than the
    enclosure's width, which is 0 here as well)."""
    W, H, spp, n_iter = 19, 15, 4, 2
    R = 2 * (2 ** n_iter - 1)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sums = np.stack([0.25 * xs + 0.5 * ys + 1.0, 2.0 * xs + 0.125 * ys, 8.0 - 0.0625 * xs + 0.25 * ys], axis=-1) * spp
    g = random_guides(W, H, 23)
    if dual:
        out, scale = filt.dual(sums, sums.copy(), g, g, dict(PLAIN_DUAL, n_iter=n_iter))[0], 2
    else:
        out, scale = filt.single(sums, g, dict(PLAIN, n_iter=n_iter)), 1
    for y in range(R, H - R):
        for x in range(R, W - R):
            for j in range(3):
                assert frac(out[y, x, j]) == Fr(sums[y, x, j]) * scale, ("ramp", x, y, j)
    assert frac(out[0, 0, 0]) != Fr(sums[0, 0, 0]) * scale     # the corner sees only one side of the ramp


# ---- edge stop --------------------------------------------------------------------------------------------------------------
SLACK = 1 + Fr(1, 2 ** 40)                                 # the roundings of a double evaluation: at most 1e-12 (WIDTH_CAP)
EDGE_L, EDGE_R = (1.0, 0.5, 0.25), (0.25, 1.0, 2.0)
EDGE_GUIDES = {
    # guide -> (keywords of flat_guides left, right, the sigma's name, the squared guide distance across the edge)
    "normal": (dict(normal=(0.0, 0.0, 1.0)), dict(normal=(1.0, 0.0, 0.0)), "sigma_normal", Fr(2)),
    "depth": (dict(depth=1.0), dict(depth=3.0), "sigma_depth", Fr(4)),
    "albedo": (dict(albedo=(0.5, 0.5, 0.25)), dict(albedo=(0.5, 0.5, 0.75)), "sigma_albedo", Fr(1, 4)),     # the third component alone
}


def _two_sides(W, H, spp, xe, left, right):
    gl, gr = flat_guides(W, H, spp, **left), flat_guides(W, H, spp, **right)
    return tuple(np.concatenate([a[:, :xe], b[:, xe:]], axis=1) for a, b in zip(gl, gr))


def _edge_image(W, H, spp, xe, guides):
    """Sums whose demodulated colour is EDGE_L left of column xe and EDGE_R from it on (albedo 0.5, 0.25, 0.75: exact)."""
    e = np.empty((H, W, 3))
    e[:, :xe], e[:, xe:] = EDGE_L, EDGE_R
    return e * (guides[0] / spp) * spp, e


def check_edge_stop(filt, guide, n_iter=3, dual=False):
    """Two half-images that differ in ONE guide by the squared distance D (normals (0,0,1) | (1,0,0): D = 2; depths 1 | 3:
    D = 4; albedos that differ in the third component alone: D = 1/4), colours L | R, the colour term off, sigma = 0.01.
    A tap across the edge has w = hh * kappa, kappa = 1 / (1 + D / sigma^2); a tap on the own side has w = hh. Let eps_k
    bound |e_k - own side's colour| over the image. For a pixel p left of the edge
        e'(p) - L = [ sum_same w (e(q) - L) + sum_cross w (e(q) - L) ] / sw,  |e(q) - L| <= eps_k  resp.  |R - L| + eps_k
    so  |e'(p) - L| <= eps_k + (sum_cross w / sw) |R - L|. The cross taps of p are columns i >= i0 >= 1 of every taken
    row: sum_cross w <= kappa * (h_1 + h_2) * Hj = kappa * (5/16) * Hj with Hj the sum of h_j over the taken rows, and the own
    side holds at least column i = 0: sw >= (3/8) * Hj. Hence eps_(k+1) <= eps_k + (5/6) kappa |R - L|, and after n
    iterations every pixel is within n * (5/6) * kappa * |R - L| of its own side's colour, per channel. (The issue's cruder
    constant is sum_cross hh <= 1 over sw >= 9/64: 64/9.) With the sigma at +inf the same image must leak by the spline's
    share: one iteration moves the pixel next to the edge by exactly (5/16) (R - L) and its neighbour by (1/16) (R - L), to
    4 ulp — over a hundred times the bound, which is therefore not vacuous.
    dual: the halves are e +- d with d = (1/8, 0, 0) | (1/2, 0, 0), so v0 is 1/64 | 1/4; the colour obeys the same bound
    through n iterations, and n_iter = 0 with n prefilter passes holds the variance within n * (5/6) * kappa * |vR - vL|."""
    W, H, spp, xe, sigma = 20, 6, 4, 9, 0.01
    left, right, name, D = EDGE_GUIDES[guide]
    guides = _two_sides(W, H, spp, xe, left, right)
    sums, e = _edge_image(W, H, spp, xe, guides)
    m = guides[0] / spp
    kappa = 1 / (1 + D / Fr(sigma) ** 2)
    base = dict(DUAL if dual else SINGLE, demodulate=True, **OFF)
    side = lambda x: (EDGE_L, EDGE_R)[x >= xe]
    gap = [abs(Fr(EDGE_R[j]) - Fr(EDGE_L[j])) for j in range(3)]

    def run(prm, what="colour"):
        if not dual:
            return filt.single(sums, guides, {k: v for k, v in prm.items() if k != "var_iter"})
        d = np.zeros((H, W, 3))
        d[:, :xe, 0], d[:, xe:, 0] = 0.125, 0.5
        out, var = filt.dual((e + d) * m * spp, (e - d) * m * spp, guides, guides, prm)
        return out if what == "colour" else var

    scale = 2 * spp if dual else spp
    out = run(dict(base, n_iter=n_iter, var_iter=0, **{name: sigma}))
    for y, x, j in np.ndindex(H, W, 3):
        got = frac(out[y, x, j]) / Fr(m[y, x, j]) / scale
        assert abs(got - Fr(side(x)[j])) <= n_iter * Fr(5, 6) * kappa * gap[j] * SLACK, ("edge stop", guide, x, y, j)
    leak = run(dict(base, n_iter=1, var_iter=0))
    for y, x, j in np.ndindex(H, 2, 3):
        want = Fr(EDGE_L[j]) + (Fr(5, 16), Fr(1, 16))[x] * (Fr(EDGE_R[j]) - Fr(EDGE_L[j]))
        close(frac(leak[y, xe - 1 - x, j]) / Fr(m[y, xe - 1 - x, j]) / scale, want, 4, ("leak with the term off", guide, x, y, j))
        assert abs(want - Fr(EDGE_L[j])) > 100 * Fr(5, 6) * kappa * gap[j] or gap[j] == 0
    if dual:
        var = run(dict(base, n_iter=0, var_iter=n_iter, **{name: sigma}), "variance")
        vl, vr = Fr(1, 64), Fr(1, 4)
        for y, x in np.ndindex(H, W):
            assert abs(frac(var[y, x]) - (vl, vr)[x >= xe]) <= n_iter * Fr(5, 6) * kappa * (vr - vl) * SLACK, ("prefilter edge stop", guide, x, y)


def check_colour_edge(filt, n_iter=5):
    """The colour term alone (guides constant, no demodulation), colours L | R that differ by G = 1 in the first channel,
    sigma_color = 0.1, sigma_k = sigma_color * 2^-k. With eps_k as above and c_k = 4^k / sigma^2, a cross
    tap has dc >= (G - 2 eps_k)^2, so w <= hh * kappa_k, kappa_k = 1 / (1 + (G - 2 eps_k)^2 c_k); an own-side tap has
    dc <= 3 (2 eps_k)^2, so w >= hh / (1 + 12 eps_k^2 c_k), and the centre tap has w = 9/64 exactly. So sw is at least
    (3/8) Hj / (1 + 12 eps_k^2 c_k) and at least 9/64 >= (9/64) Hj, and the argument of check_edge_stop gives
        eps_(k+1) <= eps_k + kappa_k * min((5/6) (1 + 12 eps_k^2 c_k), 20/9) * G,
    evaluated below in rationals. kappa_k falls by 4 per iteration: the bound stays under 1.5 * kappa_0 * G (asserted). It
    shows that the colour term stops an edge; it is loose by a factor of ten (the own side pulls a leaked value back), so
    it does NOT see a sigma that is not halved — check_two_scales does."""
    W, H, spp, xe, sigma = 67, 5, 4, 33, 0.1
    L, R = (0.5, 0.5, 0.5), (1.5, 0.5, 0.5)
    e = np.empty((H, W, 3))
    e[:, :xe], e[:, xe:] = L, R
    prm = dict(SINGLE, n_iter=n_iter, sigma_color=sigma, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF, demodulate=False)
    out = filt.single(e * spp, flat_guides(W, H, spp), prm)
    eps, G = Fr(0), Fr(1)
    for k in range(n_iter):
        ck = 4 ** k / Fr(sigma) ** 2
        eps = eps + min(Fr(5, 6) * (1 + 12 * eps ** 2 * ck), Fr(20, 9)) / (1 + (G - 2 * eps) ** 2 * ck) * G
    assert eps < Fr(3, 2) / (1 + 1 / Fr(sigma) ** 2)
    for y, x, j in np.ndindex(H, W, 3):
        assert abs(frac(out[y, x, j]) / spp - Fr((L, R)[x >= xe][j])) <= eps * SLACK, ("colour edge", x, y, j)


# ---- the dual filter's one step on two regions, exactly ---------------------------------------------------------------------
def check_two_region_step(filt):
    """ONE colour iteration of the dual filter with its colour term ON, everything else off, no prefilter, on two regions:
    e = L | R = (1, 1/2, 1/4) | (5/4, 1/2, 1/4), halves e +- d with d = (1/8, 0, 0) | (1/2, 0, 0), so u0 = 1/64 | 1/4 — all
    exact in doubles. sigma_color = 2: inv_c = 1/4. A tap on the own side has dc = 0, r = 0, w = hh; a tap across has
        r = (1/16 * 1/4) / ((1/64 + 1/4) + var_floor),   w = hh * kappa,   kappa = 1 / (1 + r)
    which holds u_p + u_q, not 2 u_p. With S, T the sums of hh and hh^2 over the taken taps on the own side (index s) and
    across (index c):
        e1(p) = (S_s e_p + kappa S_c e_q) / (S_s + kappa S_c)
        u1(p) = (T_s u_p + kappa^2 T_c u_q) / (S_s + kappa S_c)^2           (su / (sw * sw), not su / sw)
    at EVERY pixel, borders included (taps skipped, not clamped). A double evaluation makes at most 8 roundings per tap and
    25 additions per sum, in three sums and two quotients: under 128 * 2^-53 relative, so 64 ulp."""
    W, H, spp, xe = 12, 7, 4, 5
    vfloor = 2.0 ** -20
    eL, eR, dL, dR = (1.0, 0.5, 0.25), (1.25, 0.5, 0.25), 0.125, 0.5
    e, d = np.empty((H, W, 3)), np.zeros((H, W, 3))
    e[:, :xe], e[:, xe:] = eL, eR
    d[:, :xe, 0], d[:, xe:, 0] = dL, dR
    g = flat_guides(W, H, spp)
    prm = dict(DUAL, n_iter=1, var_iter=0, var_floor=vfloor, demodulate=False, sigma_color=2.0, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)
    out, var = filt.dual((e + d) * spp, (e - d) * spp, g, g, prm)
    u = (Fr(dL) ** 2, Fr(dR) ** 2)
    r = Fr(1, 16) * Fr(1, 4) / ((u[0] + u[1]) + Fr(vfloor))
    kappa = 1 / (1 + r)
    for y in range(H):
        hj = [h(j) for j in _taken(H, y)]
        for x in range(W):
            mine = x >= xe
            own = [h(i) for i in _taken(W, x) if (x + i >= xe) == mine]
            across = [h(i) for i in _taken(W, x) if (x + i >= xe) != mine]
            Ss, Sc = sum(hj) * sum(own), sum(hj) * sum(across)
            Ts, Tc = sum(a * a for a in hj) * sum(a * a for a in own), sum(a * a for a in hj) * sum(a * a for a in across)
            sw = Ss + kappa * Sc
            close(var[y, x], (Ts * u[mine] + kappa ** 2 * Tc * u[not mine]) / sw ** 2, 64, ("two regions, variance", x, y))
            for j in range(3):
                ep, eq = Fr((eL, eR)[mine][j]), Fr((eL, eR)[not mine][j])
                close(out[y, x, j], (Ss * ep + kappa * Sc * eq) / sw * 2 * spp, 64, ("two regions, colour", x, y, j))


# ---- variance propagation ---------------------------------------------------------------------------------------------------
def check_variance_propagation(filt, W, H, n_iter):
    """Guide sigmas off, sigma_color = +inf, no prefilter, no demodulation, halves c +- d with d = (1/16, 1/8, 1/4):
    v0 = 21/256 everywhere and w = hh, so one iteration gives u1 = sum(hh^2) u0 / sum(hh)^2. Inside, sum(hh) = 1 and
    sum(hh^2) = (sum h^2)^2 = (70/256)^2 = (35/128)^2: k iterations give u0 * (35/128)^(2k) wherever the footprint of all
    k lies inside — exact in doubles (35^6 * 21 has 36 bits), compared for equality. After ONE iteration every pixel,
    borders included, holds the closed form over the taps taken, sum(hh^2) / sum(hh)^2 * u0: exact numerator and
    denominator, one correctly rounded quotient, 1 ulp."""
    spp = 4
    c, d = np.empty((H, W, 3)), np.empty((H, W, 3))
    c[...], d[...] = (0.75, 0.5, 1.25), (0.0625, 0.125, 0.25)
    g = random_guides(W, H, 24)
    u0 = Fr(21, 256)
    _, var = filt.dual((c + d) * spp, (c - d) * spp, g, g, dict(PLAIN_DUAL, n_iter=n_iter))
    R = 2 * (2 ** n_iter - 1)
    assert 2 * R + 1 <= min(W, H)
    for y in range(R, H - R):
        for x in range(R, W - R):
            assert frac(var[y, x]) == u0 * Fr(35, 128) ** (2 * n_iter), ("variance inside", n_iter, x, y)
    if n_iter == 1:
        for y in range(H):
            for x in range(W):
                hj, hi = [h(j) for j in _taken(H, y)], [h(i) for i in _taken(W, x)]
                want = sum(a * a for a in hj) * sum(a * a for a in hi) / (sum(hj) * sum(hi)) ** 2 * u0
                close(var[y, x], want, 1, ("variance at the border", x, y))


def check_variance_calibration(filt):
    """What "the residual variance per pixel" means. Halves iid N(c, s^2) per channel around a constant, 64 x 64, seed fixed,
    one iteration, no prefilter, the colour term off, constant guides, no demodulation. Per channel the mean (A + B) / 2 has
    variance s^2 / 2, and v0 = |(A - B) / 2|^2 estimates the three channels' sum without bias. Inside, e1 - c = sum hh
    (e0 - c) has the summed variance (35/128)^2 * 3 s^2 / 2, and out_var = sum hh^2 v0 estimates exactly that.
      (a) mean(out_var) against (35/128)^2 * mean(v0) over the pixels inside: both are weighted means of the same v0
          samples; the standard error of either is at most (35/128)^2 * std(v0) / sqrt(n), and twice that is allowed for.
      (b) mean |e1 - c|^2 against mean(out_var) on a lattice of stride 5 (footprints disjoint: independent pixels), the
          standard error from the sample standard deviations of both, in quadrature.
    Both within 6 standard errors. Inside, sw = 1, so this does not see su / sw for su / (sw * sw) (the border closed forms
    do); it sees the weights' square: su = sum(w u) would report u0 itself, 13 times the variance that is left."""
    W = H = 64
    spp, s = 4, 0.05
    g = np.random.default_rng(31)
    c = np.array((0.75, 0.5, 1.25))
    A, B = c + s * g.normal(size=(H, W, 3)), c + s * g.normal(size=(H, W, 3))
    guides = flat_guides(W, H, spp)
    prm0 = dict(PLAIN_DUAL, n_iter=0)
    v0 = np.asarray(filt.dual(A * spp, B * spp, guides, guides, prm0)[1], dtype=np.float64)
    out, var = (np.asarray(a, dtype=np.float64) for a in filt.dual(A * spp, B * spp, guides, guides, dict(PLAIN_DUAL, n_iter=1)))
    k2 = (35.0 / 128.0) ** 2
    inside = (slice(2, H - 2), slice(2, W - 2))
    n = v0[inside].size
    se = 2 * k2 * v0[inside].std(ddof=1) / math.sqrt(n)
    ratio_a = var[inside].mean() / (k2 * v0[inside].mean())
    assert abs(var[inside].mean() - k2 * v0[inside].mean()) <= 6 * se, ("mean of out_var", ratio_a)
    lattice = (slice(2, H - 2, 5), slice(2, W - 2, 5))
    sq = ((out[lattice] / (2 * spp) - c) ** 2).sum(-1)
    pv = var[lattice]
    se = math.sqrt(sq.var(ddof=1) / sq.size + pv.var(ddof=1) / pv.size)
    assert abs(sq.mean() - pv.mean()) <= 6 * se, ("empirical variance", sq.mean(), pv.mean(), se)
    assert 6 * se < 0.6 * pv.mean()                        # the test has teeth: a factor of 13 is far outside
    return ratio_a, sq.mean() / pv.mean()


# ---- exact invariants, compared on bits -------------------------------------------------------------------------------------
def same(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


def check_invariants(filt):
    """Scalings by powers of two are exact in doubles (no value here comes near the exponent's ends), so:
      (sums * 2^k, sigma_color * 2^k) -> out * 2^k for k = +-3: e scales by 2^k, dc by 4^k, inv_c by 4^-k, every w is the same;
      (sums * 2, features * 2, spp * 2) -> out * 2: every mean is the same double, the last product doubles."""
    W, H = 12, 9
    sums, feat = buffers(W, H, seed=41, hostile=False)
    g = unpack(feat)
    for prm in (dict(SINGLE), dict(SINGLE, **TIGHT)):
        ref = filt.single(sums, g, prm)
        for k in (-3, 3):
            s = 2.0 ** k
            same(filt.single(sums * s, g, dict(prm, sigma_color=prm["sigma_color"] * s)), np.asarray(ref) * s, ("scaled by 2^%d" % k))
        same(filt.single(sums * 2, tuple(a * 2 for a in g), dict(prm, spp=2 * prm["spp"])), np.asarray(ref) * 2, "twice the samples")


def check_two_scales(filt):
    """Iteration k >= 1 of rt_denoise reads the taps p + (i, j) * 2^k with sigma_color * 2^-k. The pixels of one parity class
    (x mod 2, y mod 2) only ever read their own class from then on, at the offsets (i, j) * 2^(k-1) of the decimated image,
    and a tap leaves the image exactly when it leaves the decimated one. So with m = 1 (no demodulation; the sums * 1 / 4 * 4
    are exact)
        denoise(S, n, sigma) = on each parity class: denoise(denoise(S, 1, sigma)[class], n - 1, sigma / 2)
    operation for operation, hence bit for bit, with every guide term on. n = 3: the left side steps 1, 2, 4 under sigma,
    sigma / 2, sigma / 4. A step of k + 1 (1, 2, 3) or a sigma that stays breaks the equality."""
    W, H, n = 13, 10, 3
    sums, feat = buffers(W, H, seed=43, hostile=False)
    g = unpack(feat)
    for over in (dict(), dict(TIGHT)):
        prm = dict(SINGLE, demodulate=False, **over)
        whole = np.asarray(filt.single(sums, g, dict(prm, n_iter=n)), dtype=np.float64)
        first = np.asarray(filt.single(sums, g, dict(prm, n_iter=1)), dtype=np.float64)
        for py in (0, 1):
            for px in (0, 1):
                cls = (slice(py, None, 2), slice(px, None, 2))
                rest = filt.single(np.ascontiguousarray(first[cls]), tuple(np.ascontiguousarray(a[cls]) for a in g),
                                   dict(prm, n_iter=n - 1, sigma_color=prm["sigma_color"] / 2))
                same(rest, whole[cls], ("two scales", py, px))
        assert not np.array_equal(whole, first)


def check_invariants_dual(filt):
    """  the halves exchanged -> the same bits in both outputs: c, the guides and v0 = |+-h|^2 are symmetric in A and B;
      (sums * 2^k, var_floor * 4^k) -> (out * 2^k, variance * 4^k): r is a ratio of two quantities that scale by 4^k;
      identical halves -> the variance is +0 exactly: h = (+0 * 0.5) / m = +0, v0 = +0, every su = +0 and +0 / sw^2 = +0,
      while r = dc * inv_c / var_floor stays finite (var_floor 1e-6, sigma_color 2)."""
    W, H = 12, 9
    sa, sb, fa, fb = halves(W, H, seed=42, hostile=False)
    ga, gb = unpack(fa), unpack(fb)
    for prm in (dict(DUAL), dict(DUAL, **TIGHT_DUAL)):
        out, var = filt.dual(sa, sb, ga, gb, prm)
        o2, v2 = filt.dual(sb, sa, gb, ga, prm)
        same(o2, out, "halves exchanged"), same(v2, var, "halves exchanged, variance")
        for k in (-3, 3):
            s = 2.0 ** k
            o2, v2 = filt.dual(sa * s, sb * s, ga, gb, dict(prm, var_floor=prm["var_floor"] * s * s))
            same(o2, np.asarray(out) * s, "scaled"), same(v2, np.asarray(var) * s * s, "scaled, variance")
    out, var = filt.dual(sa, sa.copy(), ga, ga, dict(DUAL))
    var = np.asarray(var, dtype=np.float64)
    assert np.isfinite(np.asarray(out, dtype=np.float64)).all()
    assert not var.any() and not np.signbit(var).any(), "identical halves: the variance is +0"


# ---- the closed forms as a list -----------------------------------------------------------------------------------------------
def closed_forms(big=True):
    """[(name, "single" | "dual", check(filt))]. big=False: the sizes and counts the 200-bit loop can afford, and without the
    statistics and the bit comparisons, which mean nothing there."""
    W, H, x0, y0 = (67, 35, 40, 13) if big else (19, 15, 11, 6)
    f = [("fixed point, n_iter %d" % n, "single", lambda filt, n=n: check_fixed_point(filt, n)) for n in FIXED_ITERS]
    f += [("fixed point, n_iter %d, var_iter %d" % nv, "dual", lambda filt, nv=nv: check_fixed_point_dual(filt, *nv))
          for nv in ((0, 0), (0, 1), (0, 3), (3, 1), (6, 0))]
    for which in ("single", "dual"):
        d = which == "dual"
        f += [("impulse, n_iter %d" % n, which, lambda filt, n=n, d=d: check_impulse(filt, W, H, x0, y0, n, dual=d))
              for n in ((1, 2, 3) if big else (1, 2))]
        f += [("impulse at the borders", which, lambda filt, d=d: check_impulse_borders(filt, dual=d)),
              ("ramp", which, lambda filt, d=d: check_ramp(filt, dual=d))]
        f += [("edge stop, " + g, which, lambda filt, g=g, d=d: check_edge_stop(filt, g, dual=d)) for g in EDGE_GUIDES]
    f += [("colour edge", "single", lambda filt: check_colour_edge(filt, 5 if big else 3)),
          ("two regions, one step", "dual", check_two_region_step)]
    f += [("variance propagation, n_iter %d" % n, "dual", lambda filt, a=(w, h_, n): check_variance_propagation(filt, *a))
          for w, h_, n in ((15, 13, 1), (15, 13, 2)) + (((31, 29, 3),) if big else ())]
    if big:
        f += [("variance calibration", "dual", check_variance_calibration), ("invariants", "single", check_invariants), ("two scales", "single", check_two_scales),
              ("invariants", "dual", check_invariants_dual)]
    return f
