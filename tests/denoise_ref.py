"""The edge-avoiding denoiser (rt_denoise*) once more in numpy, and what the denoiser, dual-denoiser, temporal and adaptive
tests share: random feature buffers, the row lists longer than the row kernel's block, the display value and the invalid
parameter blocks. No GPU is needed.

`restate` is include/rt2022.h's definition once more: the 25 taps one after the other in the header's order, the pixels of a
tap vectorised, a skipped tap through np.where. numpy's element-wise + - * / on float64 are the IEEE operations and nothing
is fused, so the kernels (built with -ffp-contract=off) must give the same doubles."""
import math

import numpy as np

from raytracer_2022_amd import _ffi as F

H5 = [1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0]


def dist(p, q):
    d0, d1, d2 = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
    return (d0 * d0 + d1 * d1) + d2 * d2


def restate(sums, feat, p, rows=None):
    """The definition in numpy. sums (H, W, 3) and feat (H, W) FEATURE_DTYPE in buffer order -> filtered sums, buffer order."""
    H, W = p.height, p.width
    sums = np.asarray(sums, dtype=np.float64).reshape(H, W, 3)
    feat = np.asarray(feat).reshape(H, W)
    if rows is not None:                                   # buffer row i is image row rows[i]
        inv = np.empty(H, dtype=np.int64)
        inv[np.asarray(rows, dtype=np.int64)] = np.arange(H)
        sums, feat = sums[inv], feat[inv]
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        sp = np.float64(p.spp)
        c = np.where(np.isnan(sums), np.float64(0.0), sums) / sp
        a, n, z = feat["albedo"] / sp, feat["normal"] / sp, feat["depth"] / sp
        floor = np.float64(p.albedo_floor)
        m = np.ones_like(a) if p.flags & F.RT_DENOISE_NO_DEMODULATE else np.where(a > floor, a, floor)
        e = c / m
        inv_n = one / (np.float64(p.sigma_normal) * np.float64(p.sigma_normal))
        inv_z = one / (np.float64(p.sigma_depth) * np.float64(p.sigma_depth))
        inv_a = one / (np.float64(p.sigma_albedo) * np.float64(p.sigma_albedo))
        ys, xs = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
        for k in range(p.n_iter):
            s = 1 << k
            sigma_k = np.float64(p.sigma_color) * np.float64(2.0 ** -k)
            inv_c = one / (sigma_k * sigma_k)
            sw, sv = np.zeros((H, W)), np.zeros((H, W, 3))
            for j in range(-2, 3):
                for i in range(-2, 3):
                    qx, qy = xs + i * s, ys + j * s
                    ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    dc, dn, da = dist(e, e[qy, qx]), dist(n, n[qy, qx]), dist(a, a[qy, qx])
                    dz = z - z[qy, qx]
                    den = (((one + dc * inv_c) * (one + dn * inv_n)) * (one + (dz * dz) * inv_z)) * (one + da * inv_a)
                    w = np.float64(H5[j + 2] * H5[i + 2]) / den
                    sw = np.where(ok, sw + w, sw)
                    sv = np.where(ok[..., None], sv + w[..., None] * e[qy, qx], sv)
            e = sv / sw[..., None]
        out = (e * m) * sp
    return out if rows is None else out[np.asarray(rows, dtype=np.int64)]


def buffers(W, H, spp=4, seed=1, hostile=True, nan_albedo=True):
    """Random sums and feature records; hostile: NaN radiance components, zero and NaN albedo, all-zero "miss" records, 1e30s."""
    g = np.random.default_rng(seed)
    sums = g.uniform(0.0, 2.0 * spp, (H, W, 3))
    feat = np.zeros((H, W), dtype=F.FEATURE_DTYPE)
    feat["albedo"] = g.uniform(0.0, 1.0 * spp, (H, W, 3))
    nrm = g.normal(size=(H, W, 3))
    feat["normal"] = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True) * spp
    feat["depth"] = g.uniform(1.0, 20.0, (H, W)) * spp
    feat["hits"] = spp
    # a few flat regions, so that some weights are large
    feat["albedo"][: H // 2, : W // 2] = (0.5 * spp, 0.25 * spp, 0.125 * spp)
    feat["normal"][: H // 2] = (0.0, 0.0, 1.0 * spp)
    if hostile:
        pick = lambda frac, shape: g.random(shape) < frac
        sums[pick(0.03, (H, W, 3))] = np.nan
        sums[pick(0.01, (H, W, 3))] = 1e30
        sums[pick(0.01, (H, W, 3))] = -3.0
        feat["albedo"][pick(0.03, (H, W))] = 0.0
        feat["albedo"][pick(0.01, (H, W, 3))] = 1e30
        feat["depth"][pick(0.01, (H, W))] = 1e30
        if nan_albedo:
            feat["albedo"][pick(0.004, (H, W, 3))] = np.nan
        miss = pick(0.05, (H, W))
        feat.view(np.float64).reshape(H, W, 8)[miss] = 0.0
    return sums, feat


# ---- the parameter sets of the switch tests: keywords of denoise_params, and the sample count --------------------------------
INF = math.inf
SWITCHES = {
    "n_iter 0": dict(n_iter=0), "n_iter 1": dict(n_iter=1), "no demodulation": dict(demodulate=False),
    "colour off": dict(sigma_color=INF), "normal off": dict(sigma_normal=INF), "depth off": dict(sigma_depth=INF),
    "depth on": dict(sigma_depth=2.0), "depth alone off": dict(sigma_depth=INF, sigma_color=0.5, sigma_normal=0.2, sigma_albedo=0.2),
    "albedo off": dict(sigma_albedo=INF), "all off": dict(sigma_color=INF, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF),
    "tight": dict(sigma_color=0.3, sigma_normal=0.05, sigma_depth=0.1, sigma_albedo=0.01, albedo_floor=0.3),
    "spp 1": dict(spp=1), "spp 7, 3 iterations": dict(spp=7, n_iter=3),
}


# ---- row lists longer than the row kernel's block ---------------------------------------------------------------------------
# post_rows (csrc/hip/pt_rows.hip) is ONE workgroup of 1024 threads striding over the list: thread t takes entries t, t + 1024, t + 2048, ... So a
# thread's second trip starts at a height of 1025 (one entry on it) and 2500 rows give every thread two or three entries.
LONG_W, LONG_HEIGHTS, ROW_BLOCK = 3, (1025, 2500), 1024


def long_row_lists(H, seed):
    """A shuffled list of H > 1024 rows and the lists post_rows must refuse -> (rows, {fault: list}). A fault whose entries the
    height does not hold is left out (1025 rows have no entry 1500 or 7 + 1024)."""
    rows = np.random.default_rng(seed).permutation(H).astype(np.uint32)
    assert H > ROW_BLOCK and rows.tolist() != list(range(H))
    bad = {}
    if H > 1500:                                           # a repeat across trips: entry 5 on a first trip, 1500 on thread 476's second
        bad["repeat across trips"] = rows.copy()
        bad["repeat across trips"][5] = rows[1500]
    if H > 7 + ROW_BLOCK:                                  # a repeat inside one thread: entries 7 and 7 + 1024 are both thread 7's
        bad["repeat inside one thread"] = rows.copy()
        bad["repeat inside one thread"][7] = rows[7 + ROW_BLOCK]
    bad["out of range on the last trip"] = rows.copy()
    bad["out of range on the last trip"][H - 1] = H
    return rows, bad


def display(sums, spp):
    c = np.where(np.isnan(sums), 0.0, sums) / spp
    return np.sqrt(np.clip(c, 0.0, 0.999))


def bad_params(rt):
    """(what, params) for every way a parameter block can be invalid."""
    from raytracer_2022_amd import _ffi as F
    cases = []
    for field in ("width", "height", "spp"):
        p = rt.denoise_params(8, 6, 4)
        setattr(p, field, 0)
        cases.append((field + " = 0", p))
    cases.append(("n_iter", rt.denoise_params(8, 6, 4, n_iter=F.RT_DENOISE_MAX_ITER + 1)))
    for field in ("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo", "albedo_floor"):
        for v in (0.0, -1.0, math.nan, -math.inf):
            cases.append(("%s = %r" % (field, v), rt.denoise_params(8, 6, 4, **{field: v})))
    cases.append(("infinite floor", rt.denoise_params(8, 6, 4, albedo_floor=math.inf)))
    for bits in (0x2, 0x80000000, 0x3):
        p = rt.denoise_params(8, 6, 4)
        p.flags = bits
        cases.append(("flags %#x" % bits, p))
    cases.append(("too many pixels", rt.denoise_params(1 << 20, (1 << 16) + 1, 4)))
    return cases
