"""The rest of a hit record, on top of tests/brute_hits.py: for the winner (path, t) of a brute_hits.Answer the point, the face
normal, front_face, u, v and the material, carried out through the movers and FlipFace refs of the path; the texture value
there; the albedo rule of the feature records. numpy longdouble throughout, an rt_scene_desc read through dtypes of its own,
no code of oracle/ or csrc/. brute_hits holds hit / miss, t and the leaf; this module holds what is computed FROM them.

The leaf's frame (ray o', d' = brute_hits.ray_in of the world ray):
  p        o' + t d'
  n        the unit outward normal: sphere / moving sphere (p - centre(time)) / radius (signed, sphere.rs:59); rect and every box
           face +axis (aarect.rs:58, boxes.rs:24-66); triangle (b - a) x (c - a) normalised; ring +y
  front    d' . n < 0; the record's normal is n where front, -n otherwise (HitRecord::set_face_normal, mod.rs:49-56)
  u, v     sphere theta = acos(-n.y), phi = atan2(-n.z, n.x) + pi, (phi / 2 pi, theta / pi); rect ((a - a0) / (a1 - a0),
           (b - b0) / (b1 - b0)), a box face with the face's own extents; triangle the barycentrics beta, gamma of the
           xy-PROJECTION of p (triangle.rs:65-72); ring (0, 0)
Out through the movers, innermost first, by the reference renderer's definitions (hittable/mod.rs), which are not geometry:
  translate / zoom   p mapped out; set_face_normal(moved ray, rec.normal): front = d . normal < 0 with the normal the record
                     carries, the normal negated where that is false. Over a normal already turned against d that is "front
                     becomes true, normal unchanged" (mod.rs:169, :325) — a FlipFace below such a mover is erased;
  rotate_y           p and the normal through the transpose matrix; front = (R d) . (R^T normal) < 0 — the OBJECT-frame direction
                     against the PARENT-frame normal (mod.rs:258) — and the normal negated where false. Both values occur, and
                     the normal that leaves a RotateY need not face its ray: a Translate or Zoom ABOVE a RotateY therefore takes
                     a real decision too (d . normal may be positive), so every mover applies the one general rule here;
  FlipFace           toggles the flag, never the normal, at the level where the bit sits (LeafPath.flips), a mover's own ref
                     included: after that mover's set_face_normal.
A ConstantMedium's record is constant: normal (1, 0, 0), front 1, u = v = 0 (constantmedium.rs:66-74); its p is o + t_got d.

Classes, decided from the reference alone before any result is looked at; they add to brute_hits' (ambiguous, ties and classes
1 to 3 are left out here as there):
  face-ambiguous  some set_face_normal on the path has |dot| / (|d| |n|) < MARGIN: front_face and the normal's sign are not
                  compared; p, u, v, |normal| still are
  pole            a sphere hit with rho = sqrt(n.x^2 + n.z^2) < POLE: u is not compared (v is)
  seam            every sphere's u is compared modulo 1
  uv-degenerate   a triangle whose xy-projected area over its area, |n.z|, is below MARGIN: u, v not compared (inf / NaN for a
                  triangle in a plane x = const or y = const; pinned by a known-answer test)
  checker-edge    |sin(10 x) sin(10 y) sin(10 z)| < MARGIN at the hit: the texture value is not compared
  texel-edge      u W or v H within TEXEL_EDGE of an integer 1 .. W - 1 (H - 1): the texture value is not compared (0 and W are
                  no edges: the clamps make both sides the same texel — except on a sphere, whose seam joins u = 0 to u = 1)
  medium-moved    a medium under a mover: the mover's set_face_normal turns (1, 0, 0) over; no scene here has one; left out

Tolerances, from brute_hits.TOL and the margins (nothing here is tuned; a ratio over 1 means this derivation or the code is
wrong). brute_hits bounds |dt| |d| <= TOL scale, scale = |o| + |p| + |t| |d| in world units. No mover changes |d|, so that is
the error of p in the LEAF's frame, dp_leaf <= TOL scale. ROUND = 2e-13 is brute_hits' policy applied to what follows t: under
40 f64 operations at 2^-53 (4.4e-15) with 50x headroom.
  p        Translate and RotateY carry dp_leaf out unchanged, a Zoom multiplies it by its rate:
           |dp| <= (TOL + ROUND) scale Z,  Z = prod max(1, |rate|)
  normal   planar kinds: a constant, ROUND. Spheres: n = (p - c) / r, so dn = dp_leaf / |r| + ROUND: the error over the leaf's
           extent. Rotations keep it; Translate and Zoom do not touch the normal.
  u, v     sphere: d(phi) <= dn / (rho - dn) and d(theta) <= dn / (rho - dn) (acos' = 1 / sqrt(1 - y^2) = 1 / rho, bounded over
           the interval by the smaller rho), so du = dn / (rho - dn) / 2 pi and dv = dn / (rho - dn) / pi, + ROUND; POLE = 1e-3
           keeps rho >> dn.  rect: dp_leaf / |a1 - a0| + ROUND (1 + (|a| + |a0|) / |a1 - a0|).  triangle: beta = (c1 b2 - b1 c2)
           / det with c = a - p: d(beta) <= dp_leaf (|b1| + |b2|) / |det|, d(gamma) <= dp_leaf (|a1| + |a2|) / |det|, + ROUND
           (1 + |beta|): the extent factor is the projected edge over the projected area, at most 2 / (MARGIN extent) relative.
  texture  solid, checker (its solids) and image values: one f64 rounding, 2^-53 relative (1 / 255.999 is formed in f64 as
           the reference forms it). Noise: 0.5 (1 + sin(scale z + 10 turb(p, 7))) is Lipschitz with
           L = 0.5 (|scale| + 70 G): turb = |sum_i 2^-i noise(2^i p)| has gradient at most 7 G.  G bounds |grad noise|: with
           s(x) = x^2 (3 - 2x), |s'| <= 1.5, the weights of perlin.rs:81-98 are products of ss = s(s(x)) or 1 - ss; per axis
           d noise / dx = s'(x) [ s'(s) sum_c (dW_c / d ss) (g_c . w_c) + sum_c W_c g_c.x ], |g_c . w_c| <= sqrt(3) (unit g,
           |w| <= sqrt(3)), the first sum is a convex combination of differences of two such dots (<= 2 sqrt(3)), the second of
           components of unit vectors (<= 1): <= 1.5 (1.5 * 2 sqrt(3) + 1) = 9.3 per axis, G = sqrt(3) * 9.3 = 16.1. G is
           checked against finite differences of THIS module's noise in tests/test_brute_records.py, never against the oracle
           or the device. The evaluation's own rounding: the fractions p - floor(p) are exact in f64; 8 corners x 12 operations
           on values under 2 give 2.2e-14 per noise call, NOISE_ROUND = 1.1e-12 with the 50x; the sine's argument carries
           |scale z| 2^-52 from the product: tol = L |dp| + 0.5 (2^-50 |scale z| + 70 NOISE_ROUND) + 2^-50.
Every comparison is reported as error / tolerance; compare() returns the worst ratio per field.
"""
import ctypes as C

import numpy as np

import brute_hits as B
from brute_hits import LD, MARGIN, TOL, K_SPHERE, K_MOVING_SPHERE, K_RECT, K_BOX, K_TRIANGLE, K_RING, K_ROTATE_Y, K_ZOOM

POLE = 1e-3
TEXEL_EDGE = 1e-3
ROUND = 2e-13
NOISE_ROUND = 1.1e-12
NOISE_G = 16.1
CHECKER_DEPTH = 8                                          # the deepest checker chain rt_scene_create accepts
EPS = 2.0 ** -53
(MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT, MAT_ISOTROPIC) = range(5)
(TEX_SOLID, TEX_CHECKER, TEX_NOISE, TEX_IMAGE) = range(4)
FIELDS = ("p", "normal", "u", "v", "front", "mat", "texture")

_f8, _u4 = "<f8", "<u4"
SHADE_DTYPES = {
    "materials": np.dtype([("kind", _u4), ("tex", _u4), ("albedo", _f8, 3), ("param", _f8)]),
    "textures": np.dtype([("kind", _u4), ("a", _u4), ("b", _u4), ("_pad", _u4), ("color", _f8, 3), ("scale", _f8)]),
    "images": np.dtype([("width", _u4), ("height", _u4), ("offset", "<u8")]),
    "perlins": np.dtype([("randvec", _f8, (256, 3)), ("perm_x", "<i4", 256), ("perm_y", "<i4", 256), ("perm_z", "<i4", 256)]),
}
assert [SHADE_DTYPES[k].itemsize for k in ("materials", "textures", "images", "perlins")] == [40, 48, 16, 9216]
LEAF_POOLS = {K_SPHERE: "spheres", K_MOVING_SPHERE: "moving_spheres", K_RECT: "rects", K_BOX: "boxes", K_TRIANGLE: "triangles", K_RING: "rings"}


class Shading:
    """The material, texture, image and Perlin pools of a desc. `edit` (for the tests that must fail) is called with the dict
    of writable copies before anything is derived from them."""

    def __init__(self, desc, edit=None):
        self.pools = {}
        for name, dt in SHADE_DTYPES.items():
            n = int(getattr(desc, "n_" + name))
            raw = C.string_at(getattr(desc, name), n * dt.itemsize) if n else b""
            self.pools[name] = np.frombuffer(raw, dtype=dt).copy()
        nb = int(desc.image_data_bytes)
        self.pools["image_data"] = np.frombuffer(C.string_at(desc.image_data, nb) if nb else b"", dtype=np.uint8).copy()
        if edit:
            edit(self.pools)

    def image(self, i):
        """(H, W, 3) uint8, row 0 the BOTTOM row of the picture (texture/mod.rs:94-99)."""
        im = self.pools["images"][i]
        w, h, off = int(im["width"]), int(im["height"]), int(im["offset"])
        return self.pools["image_data"][off:off + 3 * w * h].reshape(h, w, 3)


def _ld(x):
    return np.asarray(x, dtype=LD)


def _dot(a, b):
    return (a * b).sum(-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


# ---- textures -------------------------------------------------------------------------------------------------------------------
def _as_i32(x):
    """Rust's `f64 as i32`: toward zero, saturating (the argument is already floored)."""
    return np.asarray(np.clip(x, -2147483648.0, 2147483647.0), dtype=np.float64).astype(np.int64)


def perlin_noise(tab, p):
    """Perlin::noise (perlin.rs:52-98) at points p (n, 3) longdouble, `tab` one record of the perlins pool."""
    fl = np.floor(p)
    f = p - fl
    f = f * f * (3 - 2 * f)                                 # smoothed once in noise() ...
    ff = f * f * (3 - 2 * f)                                # ... and again in trilinear_interp, for the weights only
    ijk = _as_i32(fl)
    g = _ld(tab["randvec"])
    perm = (tab["perm_x"].astype(np.int64), tab["perm_y"].astype(np.int64), tab["perm_z"].astype(np.int64))
    acc = np.zeros(len(p), dtype=LD)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                dd = (di, dj, dk)
                idx = perm[0][(ijk[:, 0] + di) & 255] ^ perm[1][(ijk[:, 1] + dj) & 255] ^ perm[2][(ijk[:, 2] + dk) & 255]
                w = _dot(g[idx], f - _ld(dd))
                for ax in range(3):
                    w = w * (ff[:, ax] if dd[ax] else 1 - ff[:, ax])
                acc = acc + w
    return acc


def perlin_turb(tab, p, depth=7):
    acc, weight = np.zeros(len(p), dtype=LD), LD(1)
    q = p
    for _ in range(depth):
        acc = acc + weight * perlin_noise(tab, q)
        weight = weight * LD(0.5)
        q = q * 2
    return np.abs(acc)


class TexValue:
    """value (n, 3) longdouble; checker_edge, texel_edge (n,) bool; tol (n,) float64: the bound on |got - value| per
    component for an argument p in error by dp (tolerance(dp)); kind (n,): the kind of the texture that answered; top (n,): of
    the texture asked."""

    def __init__(self, n):
        self.value, self.kind = np.zeros((n, 3), dtype=LD), np.full(n, -1)
        self.checker_edge, self.texel_edge, self.skip = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
        self.top = np.full(n, -1)                                  # the kind of the texture asked, before a checker chose
        self.seam = np.zeros(n, bool)                              # an image's u W within TEXEL_EDGE of 0 or W: an edge for a sphere's u
        self.lip, self.round_abs = np.zeros(n), np.zeros(n)

    @property
    def edge(self):
        """Where the value is not compared: either edge class, or what the caller adds in `skip`."""
        return self.checker_edge | self.texel_edge | self.skip

    def tolerance(self, dp=0.0):
        mag = np.asarray(np.abs(self.value).max(1), dtype=np.float64)
        return self.lip * dp + self.round_abs + EPS * mag * (1 + 1e-6)


def texture_value_ref(sh, tex, u, v, p):
    """Texture::value(u, v, p) (texture/mod.rs) of texture index `tex` at n points → TexValue."""
    u, v, p = _ld(u).reshape(-1), _ld(v).reshape(-1), _ld(p).reshape(-1, 3)
    out = TexValue(len(u))
    _tex_into(sh, int(tex), u, v, p, np.arange(len(u)), out, 0)
    return out


def _tex_into(sh, tex, u, v, p, where, out, depth):
    if not len(where):
        return
    t = sh.pools["textures"][tex]
    kind = int(t["kind"])
    if depth == 0:
        out.top[where] = kind
    if kind == TEX_CHECKER:
        assert depth < CHECKER_DEPTH, "a checker chain deeper than rt_scene_create accepts"
        sines = np.sin(p[where, 0] * 10) * np.sin(p[where, 1] * 10) * np.sin(p[where, 2] * 10)
        out.checker_edge[where] |= np.asarray(np.abs(sines) < MARGIN)
        odd = np.asarray(sines < 0)
        _tex_into(sh, int(t["a"]), u, v, p, where[odd], out, depth + 1)
        _tex_into(sh, int(t["b"]), u, v, p, where[~odd], out, depth + 1)
        return
    out.kind[where] = kind
    if kind == TEX_SOLID:
        out.value[where] = _ld(t["color"])[None]
    elif kind == TEX_NOISE:
        scale, q = LD(t["scale"]), p[where]
        out.value[where] = (LD(0.5) * (1 + np.sin(scale * q[:, 2] + 10 * perlin_turb(sh.pools["perlins"][int(t["a"])], q, 7))))[:, None]
        out.lip[where] = 0.5 * (abs(float(scale)) + 70 * NOISE_G)
        out.round_abs[where] = 0.5 * (4 * EPS * 2 * np.abs(np.asarray(scale * q[:, 2], dtype=np.float64)) + 70 * NOISE_ROUND) + 8 * EPS
    else:
        assert kind == TEX_IMAGE, kind
        img = sh.image(int(t["a"]))
        h, w = img.shape[:2]
        if w * h == 0:
            out.value[where] = _ld([0, 1, 1])[None]
            return
        ij = []
        for x, n in ((u[where], w), (v[where], h)):
            x = np.clip(x, 0, 1) * n                          # (a NaN stays NaN; `as usize` makes it 0)
            near = np.rint(x)
            out.texel_edge[where] |= np.asarray((np.abs(x - near) < TEXEL_EDGE) & (near >= 1) & (near <= n - 1))
            if n == w:
                out.seam[where] |= np.asarray((x < TEXEL_EDGE) | (x > n - TEXEL_EDGE))
            ij.append(np.minimum(np.nan_to_num(np.asarray(np.trunc(x), dtype=np.float64), nan=0.0).astype(np.int64), n - 1))
        out.value[where] = _ld(img[ij[1], ij[0]].astype(np.float64)) * LD(np.float64(1.0) / np.float64(255.999))


def albedo_ref(sh, mat, front, u, v, p):
    """The feature header's albedo rule (include/rt2022.h) per record: Lambertian / Isotropic the texture value, Metal its albedo,
    Dielectric 1, DiffuseLight the texture on the front face and 0 on the back → TexValue (kind -1 where no texture is read)."""
    mat, front = np.asarray(mat).reshape(-1), np.asarray(front, dtype=bool).reshape(-1)
    u, v, p = _ld(u).reshape(-1), _ld(v).reshape(-1), _ld(p).reshape(-1, 3)
    out = TexValue(len(mat))
    for m in np.unique(mat):
        rec = sh.pools["materials"][int(m)]
        sel = np.flatnonzero(mat == m)
        kind = int(rec["kind"])
        if kind == MAT_METAL:
            out.value[sel] = _ld(rec["albedo"])[None]
        elif kind == MAT_DIELECTRIC:
            out.value[sel] = 1
        else:
            assert kind in (MAT_LAMBERTIAN, MAT_ISOTROPIC, MAT_DIFFUSE_LIGHT), kind
            if kind == MAT_DIFFUSE_LIGHT:
                sel = sel[front[sel]]                        # (the back stays 0)
            _tex_into(sh, int(rec["tex"]), u, v, p, sel, out, 0)
    return out


# ---- records --------------------------------------------------------------------------------------------------------------------
class Records:
    """Per ray, where ans.hit: p, normal (n, 3) and u, v longdouble, front, mat, and what the comparison needs: face_margin (the
    smallest |dot| / |d| of the path's set_face_normal calls), sphere / pole / uv_degenerate, the tolerances tol_p, tol_n, tol_u,
    tol_v, and for the floors moved (a mover on the path), rotated (a RotateY on it), flip_below (a FlipFace bit below a mover)."""
    pass


def _leaf_geometry(scene, path, o, d, t, tm, dp_leaf):
    """→ (n outward unit (k, 3), u, v, pole, uv_degenerate, dn, du, dv) of the leaf at p = o + t d, all in the leaf's frame."""
    P, kind, i = scene.pools, B.ref_kind(path.leaf), B.ref_index(path.leaf)
    k = len(o)
    p = o + t[:, None] * d
    zero, no = np.zeros(k, dtype=LD), np.zeros(k, bool)
    if kind in (K_SPHERE, K_MOVING_SPHERE):
        if kind == K_SPHERE:
            q = P["spheres"][i]
            c = np.broadcast_to(_ld(q["center"]), (k, 3))
        else:
            q = P["moving_spheres"][i]
            f = (_ld(tm) - LD(q["time0"])) / (LD(q["time1"]) - LD(q["time0"]))
            c = _ld(q["center0"])[None] + f[:, None] * (_ld(q["center1"]) - _ld(q["center0"]))[None]
        r = LD(q["radius"])
        n = (p - c) / r
        pi = np.arctan2(LD(0), LD(-1))
        u = (np.arctan2(-n[:, 2], n[:, 0]) + pi) / (2 * pi)
        v = np.arccos(np.clip(-n[:, 1], -1, 1)) / pi
        rho = np.asarray(np.sqrt(n[:, 0] ** 2 + n[:, 2] ** 2), dtype=np.float64)
        dn = dp_leaf / abs(float(r)) + ROUND
        with np.errstate(divide="ignore", invalid="ignore"):
            amp = np.where(rho > 2 * dn, dn / (rho - dn), np.inf)
        return n, u, v, rho < POLE, no, dn, amp / (2 * np.pi) + ROUND, np.minimum(amp, np.sqrt(2 * dn) + dn) / np.pi + ROUND
    if kind in (K_RECT, K_BOX):
        if kind == K_RECT:
            q = P["rects"][i]
            ka, aa, ba = B.RECT_AXES[int(q["axis"])]
            a0, a1, b0, b1 = (np.full(k, LD(q[f])) for f in ("a0", "a1", "b0", "b1"))
            ka = np.full(k, ka); aa = np.full(k, aa); ba = np.full(k, ba)
        else:
            q = P["boxes"][i]
            p0, p1 = _ld(q["p0"]), _ld(q["p1"])
            best = np.full(k, np.inf, dtype=LD)
            ka = np.zeros(k, int); aa = np.zeros(k, int); ba = np.zeros(k, int)
            for fk, fa, fb in B.RECT_AXES.values():                # the face whose plane the hit lies in, inside its extents
                for side in (p0, p1):
                    with np.errstate(all="ignore"):
                        tf = (side[fk] - o[:, fk]) / d[:, fk]
                        pa, pb = o[:, fa] + tf * d[:, fa], o[:, fb] + tf * d[:, fb]
                        slack = MARGIN * np.maximum(p1[fa] - p0[fa], p1[fb] - p0[fb])
                        inside = (pa >= p0[fa] - slack) & (pa <= p1[fa] + slack) & (pb >= p0[fb] - slack) & (pb <= p1[fb] + slack)
                        dist = np.where(inside & np.isfinite(tf), np.abs(tf - t), np.inf)
                    take = dist < best
                    best = np.where(take, dist, best)
                    ka[take], aa[take], ba[take] = fk, fa, fb
            a0, a1, b0, b1 = p0[aa], p1[aa], p0[ba], p1[ba]
        r = np.arange(k)
        n = np.zeros((k, 3), dtype=LD)
        n[r, ka] = 1
        a, b = p[r, aa], p[r, ba]
        u, v = (a - a0) / (a1 - a0), (b - b0) / (b1 - b0)
        f64 = lambda x: np.asarray(x, dtype=np.float64)
        du = dp_leaf / f64(np.abs(a1 - a0)) + ROUND * (1 + f64((np.abs(a) + np.abs(a0)) / np.abs(a1 - a0)))
        dv = dp_leaf / f64(np.abs(b1 - b0)) + ROUND * (1 + f64((np.abs(b) + np.abs(b0)) / np.abs(b1 - b0)))
        return n, u, v, no, no, np.full(k, ROUND), du, dv
    if kind == K_TRIANGLE:
        q = P["triangles"][i]
        A, Bv, Cv = _ld(q["a"]), _ld(q["b"]), _ld(q["c"])
        nn = np.cross(Bv - A, Cv - A)
        nu = nn / _norm(nn)
        a1, b1, a2, b2 = A[0] - Bv[0], A[0] - Cv[0], A[1] - Bv[1], A[1] - Cv[1]
        c1, c2 = A[0] - p[:, 0], A[1] - p[:, 1]
        det = a1 * b2 - b1 * a2
        with np.errstate(all="ignore"):
            beta, gama = (c1 * b2 - b1 * c2) / det, (a1 * c2 - a2 * c1) / det
            adet = abs(float(det))
            du = dp_leaf * float(abs(b1) + abs(b2)) / adet + ROUND * (1 + np.abs(np.asarray(beta, dtype=np.float64)))
            dv = dp_leaf * float(abs(a1) + abs(a2)) / adet + ROUND * (1 + np.abs(np.asarray(gama, dtype=np.float64)))
        degenerate = np.full(k, abs(float(nu[2])) < MARGIN)
        return np.broadcast_to(nu, (k, 3)).copy(), beta, gama, no, degenerate, np.full(k, ROUND), du, dv
    assert kind == K_RING
    n = np.zeros((k, 3), dtype=LD)
    n[:, 1] = 1
    return n, zero, zero, no, no, np.full(k, ROUND), np.zeros(k), np.zeros(k)


def leaf_mat(scene, leaf):
    return int(scene.pools[LEAF_POOLS[B.ref_kind(leaf)]][B.ref_index(leaf)]["mat"])


def records(scene, rays, ans):
    """The reference's record of every ray's winner."""
    n = len(rays)
    o_all, d_all = _ld(rays["origin"]).reshape(n, 3), _ld(rays["direction"]).reshape(n, 3)
    tm_all = np.asarray(rays["time"], dtype=np.float64)
    R = Records()
    R.p, R.normal = np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    R.u, R.v = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    R.front, R.mat, R.face_margin = np.zeros(n, bool), np.zeros(n, np.uint32), np.full(n, np.inf)
    R.sphere, R.pole, R.uv_degenerate = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    R.moved, R.rotated, R.flip_below = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    R.tol_p, R.tol_n, R.tol_u, R.tol_v = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for c in np.unique(ans.path[ans.hit]):
        path = scene.paths[int(c)]
        sel = np.flatnonzero(ans.hit & (ans.path == c))
        o, d, t = o_all[sel], d_all[sel], ans.t[sel]
        dirs = [d]                                               # dirs[j]: the direction in the frame below mover j - 1
        for j in range(len(path.movers)):
            dirs.append(B.ray_in(path.movers[j:j + 1], o, dirs[-1])[1])
        oo = B.ray_in(path.movers, o, d)[0]
        dp_leaf = TOL * ans.scale[sel]
        nrm, u, v, pole, degenerate, dn, du, dv = _leaf_geometry(scene, path, oo, dirs[-1], t, tm_all[sel], dp_leaf)
        dlen = _norm(d)
        dot = _dot(dirs[-1], nrm)
        margin = np.asarray(np.abs(dot) / (dlen * _norm(nrm)), dtype=np.float64)
        front = np.asarray(dot < 0)
        nrm = np.where(front[:, None], nrm, -nrm)
        front = front != path.flips[-1]
        p = oo + t[:, None] * dirs[-1]
        zf = 1.0
        for j in range(len(path.movers) - 1, -1, -1):
            kind, q = path.movers[j]
            p = B.point_out(path.movers[j:j + 1], p)
            if kind == K_ROTATE_Y:
                nrm = B.point_out(path.movers[j:j + 1], nrm)
            elif kind == K_ZOOM:
                zf *= max(1.0, abs(q[0]))
            dot = _dot(dirs[j + 1], nrm)                         # the mover's own ray (moved_r / rotated_r) against the record's normal
            margin = np.minimum(margin, np.asarray(np.abs(dot) / (dlen * _norm(nrm)), dtype=np.float64))
            front = np.asarray(dot < 0)
            nrm = np.where(front[:, None], nrm, -nrm)
            front = front != path.flips[j]
        R.p[sel], R.normal[sel], R.u[sel], R.v[sel], R.front[sel] = p, nrm, u, v, front
        R.mat[sel], R.face_margin[sel] = leaf_mat(scene, path.leaf), margin
        R.sphere[sel] = B.ref_kind(path.leaf) in (K_SPHERE, K_MOVING_SPHERE)
        R.pole[sel], R.uv_degenerate[sel] = pole, degenerate
        R.moved[sel] = bool(path.movers)
        R.rotated[sel] = any(k == K_ROTATE_Y for k, _ in path.movers)
        R.flip_below[sel] = bool(path.movers) and any(path.flips[1:])
        R.tol_p[sel] = (TOL + ROUND) * ans.scale[sel] * zf
        R.tol_n[sel], R.tol_u[sel], R.tol_v[sel] = dn, du, dv
    R.face_ambiguous = ans.hit & (R.face_margin < MARGIN)
    return R


def new_classes(scene, ans, R, tex=None):
    """The rays the NEW classes leave out of at least one comparison, among those brute_hits compares → {class: bool array}.
    tex: the TexValue of the records' textures, where textures are compared."""
    c1, c2, c3, amb = B.classify(scene, ans)
    base = ans.hit & ~(c1 | c2 | c3 | amb | ans.tie)
    out = {"face": base & R.face_ambiguous, "pole": base & R.pole, "uv-degenerate": base & R.uv_degenerate}
    if tex is not None:
        out["checker-edge"] = base & tex.checker_edge
        out["texel-edge"] = base & (tex.texel_edge | (tex.seam & R.sphere))
    return out


class RecordTally:
    """compared: rays whose record was held; worst {field: error / tolerance}; classes {name: rays}; failures [(ray, what)]."""

    def __init__(self):
        self.rays = self.compared = self.media = 0
        self.worst = {f: 0.0 for f in FIELDS}
        self.classes, self.failures = {}, []

    def line(self, scene, family, who):
        return "%-22s %-7s %-6s rays %5d records %5d media %4d | %s | %s%s" % (
            scene, family, who, self.rays, self.compared, self.media,
            " ".join("%s %.2e" % (f, self.worst[f]) for f in ("p", "normal", "u", "v", "texture")),
            " ".join("%s %d" % kv for kv in sorted(self.classes.items())), "" if not self.failures else "  FAILURES %d" % len(self.failures))

    @property
    def worst_ratio(self):
        return max(self.worst.values())


def _ratio(err, tol):
    err, tol = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(tol, dtype=np.float64), np.shape(err))
    with np.errstate(all="ignore"):
        r = np.where(tol == 0, np.where(err == 0, 0.0, np.inf), err / tol)                # (a tolerance of 0 asks for equality)
    return np.where(np.isnan(r), np.inf, r)


def compare(scene, rays, ans, R, got, got_value=None, want_value=None):
    """A set of records against the reference's. got: arrays hit, t, u, v, p, normal, front_face, mat, rng_draws [, prim] (the
    oracle's rto_hit_record or the device's rt_hit). brute_hits.compare holds hit / miss, t and the leaf and is not repeated: a
    ray is compared here where brute_hits compares it in full (no tie either), both sides have a hit and t is within its
    tolerance. A record whose t is not the solid winner's, on a ray that drew, is a medium's: its constants are exact and p is
    o + t_got d.  got_value / want_value (a TexValue): a texture or albedo value per ray to hold as well."""
    n = len(rays)
    ta = RecordTally()
    ta.rays = n
    g = {k: np.asarray(got[k]) for k in ("hit", "t", "u", "v", "p", "normal", "front_face", "mat", "rng_draws")}
    c1, c2, c3, amb = B.classify(scene, ans)
    base = ~(c1 | c2 | c3 | amb | ans.tie) & g["hit"].astype(bool)
    tol_t = B.tolerance(ans, rays["direction"])
    with np.errstate(all="ignore"):
        t_ok = ans.hit & (np.abs(_ld(g["t"]) - ans.t) <= tol_t)
    solid = base & t_ok
    medium = base & ~t_ok & (g["rng_draws"] > 0)
    ta.classes = {k: int(v.sum()) for k, v in new_classes(scene, ans, R, want_value).items()}
    ta.compared, ta.media = int(solid.sum()), int(medium.sum())

    def fail(mask, what, detail):
        for i in np.flatnonzero(mask)[:20]:
            ta.failures.append((int(i), "%s: %s" % (what, detail(i))))

    def hold(field, mask, err, tol):
        r = _ratio(err, tol)
        if mask.any():
            ta.worst[field] = max(ta.worst[field], float(r[mask].max()))
        fail(mask & (r > 1), field, lambda i: "error %.3e tolerance %.3e leaf %#x t %r margin %.2e face margin %.2e" % (
            float(np.asarray(err, dtype=np.float64)[i]), float(np.broadcast_to(tol, (n,))[i]), int(ans.leaf[i]), float(ans.t[i]), ans.margin[i], R.face_margin[i]))
    dp = _norm(_ld(g["p"]) - R.p)
    hold("p", solid, dp, R.tol_p)
    faced = solid & ~R.face_ambiguous
    gn = _ld(g["normal"])
    dn_same, dn_opp = _norm(gn - R.normal), _norm(gn + R.normal)
    hold("normal", faced, dn_same, R.tol_n)
    hold("normal", solid & R.face_ambiguous, np.minimum(dn_same, dn_opp), R.tol_n)
    wrong = faced & (g["front_face"].astype(bool) != R.front)
    ta.worst["front"] = float(wrong.any())
    fail(wrong, "front_face", lambda i: "got %d, reference %d, face margin %.2e, leaf %#x" % (g["front_face"][i], R.front[i], R.face_margin[i], int(ans.leaf[i])))
    wrong = solid & (g["mat"] != R.mat)
    ta.worst["mat"] = float(wrong.any())
    fail(wrong, "mat", lambda i: "got %d, reference %d, leaf %#x" % (g["mat"][i], R.mat[i], int(ans.leaf[i])))
    du = np.abs(_ld(g["u"]) - R.u)
    du = np.where(R.sphere, np.minimum(du, np.abs(1 - du)), du)                      # the seam: modulo 1
    hold("u", solid & ~R.pole & ~R.uv_degenerate, du, R.tol_u)                      # (a ring's u = v = 0 has tolerance 0: exact)
    hold("v", solid & ~R.uv_degenerate, np.abs(_ld(g["v"]) - R.v), R.tol_v)
    # media: the constant record
    if medium.any():
        o, d = _ld(rays["origin"]), _ld(rays["direction"])
        with np.errstate(all="ignore"):
            pm = o + _ld(g["t"])[:, None] * d                     # (rays outside `medium` may hold inf or NaN)
            scale = np.asarray(_norm(o) + _norm(pm) + np.abs(_ld(g["t"])) * _norm(d), dtype=np.float64)
            dpm = _norm(_ld(g["p"]) - pm)
        mats = {m.mat for m in scene.media if m.n_movers == 0}
        plain = medium & np.isin(g["mat"], list(mats))
        hold("p", plain, dpm, ROUND * scale)
        wrong = plain & ~((g["normal"] == np.array([1.0, 0.0, 0.0])).all(1) & (g["front_face"] == 1) & (g["u"] == 0) & (g["v"] == 0))
        fail(wrong, "medium record", lambda i: "normal %s front %d u %r v %r" % (g["normal"][i].tolist(), g["front_face"][i], g["u"][i], g["v"][i]))
        ta.classes["medium-moved"] = int((medium & ~plain).sum())
    if got_value is not None:
        ok = solid & ~want_value.edge & ~(want_value.seam & R.sphere) & ~R.uv_degenerate & ~(R.pole & (want_value.kind == TEX_IMAGE))
        # an image reads u, v: their error must stay inside the texel (TEXEL_EDGE of it), which the class checks at the reference's u, v
        err = np.abs(_ld(got_value) - want_value.value).max(1)
        hold("texture", ok, err, want_value.tolerance(R.tol_p))
    return ta
