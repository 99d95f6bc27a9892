"""rt_ray_order's definition (include/rt2022.h) restated twice: in numpy, vectorised the way the kernels work, and as a plain
per-ray loop in Python floats and integers. tests/test_ray_order_ref.py holds the two to each other bit for bit;
tests/test_ray_order_gpu.py holds the device to the first. Rays are structured arrays with "origin" and "direction" fields
(QUERY_RAY_DTYPE, RADIANCE_RAY_DTYPE) or a pair of (n, 3) arrays."""
import math

import numpy as np

ORIGIN_FIRST, DIRECTION_FIRST, FACE_ORIGIN_UV = 0, 1, 2
LAYOUTS = (ORIGIN_FIRST, DIRECTION_FIRST, FACE_ORIGIN_UV)
MAX_COORD = 1e300
STRAGGLER_KEY = 1 << 63


def split(rays):
    if isinstance(rays, tuple):
        o, d = rays
    else:
        o, d = rays["origin"], rays["direction"]
    return np.ascontiguousarray(o, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(d, dtype=np.float64).reshape(-1, 3)


# ---- numpy -----------------------------------------------------------------------------------------------------------------------
def stragglers(o, d):
    with np.errstate(invalid="ignore"):
        ok = np.all(np.abs(o) <= MAX_COORD, axis=1) & np.all(np.abs(d) < np.inf, axis=1) & np.any(d != 0.0, axis=1)
    return ~ok


def origin_box(o, strag):
    """(lo, hi) over the non-stragglers; None when there is none (the box is then never used)."""
    keep = o[~strag]
    return (keep.min(axis=0), keep.max(axis=0)) if len(keep) else None


def cells(x, scale, top):
    """(uint32) min(x * scale, top), x * scale >= 0."""
    return np.minimum(x * np.float64(scale), np.float64(top)).astype(np.uint32)


def words(rays, origin_bits, dir_bits):
    """→ (straggler bool (n,), O uint64, face uint64, uv uint64); the three words are 0 where the ray is a straggler."""
    o, d = split(rays)
    n = len(o)
    strag = stragglers(o, d)
    O = np.zeros(n, dtype=np.uint64)
    box = origin_box(o, strag)
    if box is not None:
        lo, hi = box
        e = hi - lo
        safe_o = np.where(strag[:, None], lo, o)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(e > 0.0, (safe_o - lo) / np.where(e > 0.0, e, 1.0), 0.0)
        k = cells(q, 2.0 ** origin_bits, 2 ** origin_bits - 1)
        for b in range(origin_bits):
            for axis, shift in ((0, 2), (1, 1), (2, 0)):
                O |= ((k[:, axis] >> np.uint32(b)) & np.uint32(1)).astype(np.uint64) << np.uint64(3 * b + shift)
    safe_d = np.where(strag[:, None], np.array([1.0, 0.0, 0.0]), d)
    absd = np.abs(safe_d)
    a = np.argmax(absd, axis=1)                                # the first axis of largest |d|
    row = np.arange(n)
    m, da = absd[row, a], safe_d[row, a]
    face = (2 * a + (da < 0.0)).astype(np.uint64)
    uv = np.zeros(n, dtype=np.uint64)
    for which, j in ((1, (a + 1) % 3), (0, (a + 2) % 3)):
        r = safe_d[row, j] / m
        k = cells(r + 1.0, 0.5 * 2.0 ** dir_bits, 2 ** dir_bits - 1)
        for b in range(dir_bits):
            uv |= ((k >> np.uint32(b)) & np.uint32(1)).astype(np.uint64) << np.uint64(2 * b + which)
    zero = np.uint64(0)
    return strag, np.where(strag, zero, O), np.where(strag, zero, face), np.where(strag, zero, uv)


def keys(rays, origin_bits, dir_bits, layout):
    strag, O, face, uv = words(rays, origin_bits, dir_bits)
    ob3, db2 = np.uint64(3 * origin_bits), np.uint64(2 * dir_bits)
    D = (face << db2) | uv
    if layout == ORIGIN_FIRST:
        key = (O << (db2 + np.uint64(3))) | D
    elif layout == DIRECTION_FIRST:
        key = (D << ob3) | O
    else:
        assert layout == FACE_ORIGIN_UV
        key = (face << (ob3 + db2)) | (O << db2) | uv
    return np.where(strag, np.uint64(STRAGGLER_KEY), key)


def order(rays, origin_bits, dir_bits, layout):
    """The permutation that sorts (key, index) ascending, as uint32."""
    return np.argsort(keys(rays, origin_bits, dir_bits, layout), kind="stable").astype(np.uint32)


# ---- the loop --------------------------------------------------------------------------------------------------------------------
def loop_is_straggler(o, d):
    if not all(math.isfinite(x) for x in o + d):
        return True
    return any(abs(x) > MAX_COORD for x in o) or all(x == 0.0 for x in d)


def loop_cell(x, bits):
    return int(min(x * float(1 << bits), float((1 << bits) - 1)))


def loop_keys(rays, origin_bits, dir_bits, layout):
    """The keys as a list of Python ints, one ray at a time."""
    o_all, d_all = split(rays)
    rays_ = [([float(x) for x in o], [float(x) for x in d]) for o, d in zip(o_all.tolist(), d_all.tolist())]
    strag = [loop_is_straggler(o, d) for o, d in rays_]
    kept = [o for (o, _), s in zip(rays_, strag) if not s]
    lo = [min(o[a] for o in kept) for a in range(3)] if kept else None
    hi = [max(o[a] for o in kept) for a in range(3)] if kept else None
    out = []
    for (o, d), s in zip(rays_, strag):
        if s:
            out.append(STRAGGLER_KEY)
            continue
        O = 0
        for a in range(3):
            e = hi[a] - lo[a]
            q = (o[a] - lo[a]) / e if e > 0.0 else 0.0
            k = loop_cell(q, origin_bits)
            for b in range(origin_bits):
                O |= ((k >> b) & 1) << (3 * b + 2 - a)
        a = 0
        for j in (1, 2):
            if abs(d[j]) > abs(d[a]):
                a = j
        m = abs(d[a])
        face = 2 * a + (1 if d[a] < 0.0 else 0)
        uv = 0
        for which, j in ((1, (a + 1) % 3), (0, (a + 2) % 3)):
            r = d[j] / m
            k = int(min((r + 1.0) * (0.5 * float(1 << dir_bits)), float((1 << dir_bits) - 1)))
            for b in range(dir_bits):
                uv |= ((k >> b) & 1) << (2 * b + which)
        D = (face << (2 * dir_bits)) | uv
        if layout == ORIGIN_FIRST:
            key = (O << (3 + 2 * dir_bits)) | D
        elif layout == DIRECTION_FIRST:
            key = (D << (3 * origin_bits)) | O
        else:
            key = (face << (3 * origin_bits + 2 * dir_bits)) | (O << (2 * dir_bits)) | uv
        out.append(key)
    return out


def loop_order(rays, origin_bits, dir_bits, layout):
    key = loop_keys(rays, origin_bits, dir_bits, layout)
    return sorted(range(len(key)), key=lambda i: (key[i], i))
