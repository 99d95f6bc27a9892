"""The hand-built scenes of the closest-hit query tests (tests/test_query.py), of the feature tests (every_material_scene) and
of the radiance tests (every_kind_lit_scene), in a module of their own so that tools and other test helpers can build them
without importing a test module."""
import numpy as np

from raytracer_2022_amd import _ffi as F

from query_ref import unit_vectors


def every_kind_scene(rt, with_medium=True):
    """The hand-built scene of tests/test_gpu_parity.py: one of each hittable kind under a HittableList root."""
    b = rt.DescBuilder()
    lam = b.lambertian((0.6, 0.5, 0.4))
    img = (np.arange(8 * 4 * 3, dtype=np.uint8).reshape(4, 8, 3) * 7) % 251
    refs = [
        b.sphere((0, -100, 0), 100.0, b.lambertian(tex=b.checker(b.solid((0.2, 0.3, 0.1)), b.solid((0.9, 0.9, 0.9))))),
        b.sphere((0, 1, 0), 1.0, b.lambertian(tex=b.image(img))),
        b.moving_sphere((2.5, 0.5, 0), (2.5, 1.0, 0), 0, 1, 0.5, b.metal((0.8, 0.7, 0.6), 0.3)),
        b.sphere((-2.5, 1, 0), 1.0, b.dielectric(1.5)),
        b.triangle((-1, 0.01, 2), (1, 0.01, 2), (0, 1.5, 2.5), lam),
        b.translate(b.ring(1.5, 0.3, lam), (0, 0.5, -3)),
        b.translate(b.rotate_y(b.zoom(b.box((-0.5, 0, -0.5), (0.5, 1, 0.5), lam), 1.5), 0.5, 0.8660254037844386), (4.5, 0, 2)),
        b.list([b.rect(F.RT_RECT_XZ, -1, 1, -1, 1, 6.0, b.diffuse_light((8, 8, 8)), flip=True),
                b.rect(F.RT_RECT_XY, -6, 6, 0, 4, -6.0, lam)]),
    ]
    if with_medium:
        refs.append(b.medium(b.sphere((-4, 1, 2), 1.0, b.dielectric(1.5)), 0.8, b.isotropic((0.3, 0.3, 0.9))))
    refs.append(b.sphere((5, 6, -2), 0.7, b.diffuse_light((20, 18, 15))))
    b.set_root(b.list(refs))
    cam = rt.camera_new((9, 4, 9), (0, 1, 0), (0, 1, 0), 35.0, 56 / 40, 0.0, 12.0, 0.0, 1.0)
    return b, b.desc(), cam


MOVER_RECORD_ANGLES = (40.0, 80.0, 120.0, -60.0, 160.0, -110.0)
MOVER_RECORD_CONFIGS = ("translate", "rotate_y", "zoom1", "zoom", "chain")


def mover_records_scene(rt):
    """One leaf of each kind under each mover and under the full chain Translate(RotateY(Zoom)), on three stacked grids of 6
    kinds x 5 configurations (each layer shifts the kinds, the angles and the flips by one) under a HittableList of HittableLists (no node: brute_hits' class 2 cannot occur). For tests/brute_records.py: what a
    record becomes on its way out through movers. RotateY angles from 40 to 160 degrees either way, so that the reference's
    mixed-frame set_face_normal (hittable/mod.rs:258) gives both flag values; FlipFace bits on leaves (below the mover), on
    movers and on the chain's inner Zoom; Zoom rates 1 and 1.6; checker, noise, image and nested-checker textures, a light, a
    metal and a glass. A leaf is placed so that the mover brings it to its grid cell — except rings, which lie in y = 0 round
    their frame's origin: those under RotateY or Zoom alone are concentric annuli round the world's origin.
    → (builder, desc, camera)."""
    b = rt.DescBuilder()
    g = np.random.default_rng(2022)
    vec = g.normal(size=(256, 3))
    per = b.perlin(vec / np.linalg.norm(vec, axis=1, keepdims=True), g.permutation(256), g.permutation(256), g.permutation(256))
    img = b.image(g.integers(0, 256, (8, 16, 3), dtype=np.uint8))
    noise = b.noise(per, 4.0)
    chk = b.checker(b.solid((0.2, 0.3, 0.1)), b.solid((0.9, 0.9, 0.9)))
    mats = [b.lambertian(tex=chk), b.lambertian(tex=noise), b.lambertian(tex=img), b.diffuse_light(tex=img), b.metal((0.8, 0.6, 0.2), 0.1),
            b.dielectric(1.5), b.lambertian(tex=b.checker(noise, img)), b.diffuse_light(tex=noise)]
    ring_r = {"rotate_y": (0.6, 0.2), "zoom1": (1.2, 0.2), "zoom": (1.25, 0.125)}

    def leaf(ki, c, f, m, flip, config):
        c = np.asarray(c, dtype=float)
        if ki == 0:
            return b.sphere(tuple(c), 0.8 * f, m, flip=flip)
        if ki == 1:
            return b.moving_sphere(tuple(c), tuple(c + np.array([0.0, 0.4, 0.1]) * f), 0.0, 1.0, 0.7 * f, m, flip=flip)
        if ki == 2:
            axis = MOVER_RECORD_CONFIGS.index(config) % 3
            ka, aa, ba = {0: (2, 0, 1), 1: (1, 0, 2), 2: (0, 1, 2)}[axis]
            return b.rect(axis, c[aa] - 0.8 * f, c[aa] + 0.8 * f, c[ba] - 0.7 * f, c[ba] + 0.7 * f, c[ka], m, flip=flip)
        if ki == 3:
            h = np.array([0.7, 0.6, 0.65]) * f
            return b.box(tuple(c - h), tuple(c + h), m, flip=flip)
        if ki == 4:
            return b.triangle(tuple(c + f * np.array([-0.9, -0.6, 0.2])), tuple(c + f * np.array([0.9, -0.5, -0.3])),
                              tuple(c + f * np.array([0.1, 0.8, 0.4])), m, flip=flip)
        r, t = ring_r.get(config, (0.6, 0.25))
        return b.ring(r * (f if config in ("translate", "chain") else 1.0), t * (f if config in ("translate", "chain") else 1.0), m, flip=flip)
    refs = []
    for layer in range(3):
        for cell in range(6):
            for ci, config in enumerate(MOVER_RECORD_CONFIGS):
                ki = (cell + layer) % 6
                if ki == 5 and layer and config in ring_r:       # (one set of annuli round the origin is all that fits)
                    ki = 0
                pos = np.array([2.5 + 2.0 * cell, 0.11 + 2.0 * layer + 0.3 * ((cell + ci) % 3), 2.5 + 2.0 * ci])     # (y = 0 is an edge of every checker)
                m = mats[(layer * 3 + cell * 5 + ci) % len(mats)]
                leaf_flip, mover_flip = (cell + ci + layer) % 2 == 0, (ci + layer) % 3 == 0 or (ki == 5 and ci == 1)
                a = np.radians(MOVER_RECORD_ANGLES[(cell + 2 * layer) % 6])
                s, c = float(np.sin(a)), float(np.cos(a))
                if config == "translate":
                    ref = b.translate(leaf(ki, (0.1, 0.0, -0.1), 1.0, m, leaf_flip, config), tuple(pos), flip=mover_flip)
                elif config == "rotate_y":
                    ref = b.rotate_y(leaf(ki, (c * pos[0] - s * pos[2], pos[1], s * pos[0] + c * pos[2]), 1.0, m, leaf_flip, config), s, c,
                                     flip=mover_flip)
                elif config in ("zoom1", "zoom"):
                    rate = 1.0 if config == "zoom1" else 1.6
                    ref = b.zoom(leaf(ki, pos / rate, 1.0 / rate, m, leaf_flip, config), rate, flip=mover_flip)
                else:
                    a = np.radians(MOVER_RECORD_ANGLES[(cell + 3 + layer) % 6])
                    s, c = float(np.sin(a)), float(np.cos(a))
                    inner = b.zoom(leaf(ki, (0.1, 0.0, -0.1), 1.0 / 1.6, m, leaf_flip, config), 1.6, flip=(cell + layer) % 2 == 1)
                    ref = b.translate(b.rotate_y(inner, s, c, flip=cell % 3 == 0), tuple(pos), flip=mover_flip)
                refs.append(ref)
    b.set_root(b.list([b.list(refs[i:i + 10]) for i in range(0, len(refs), 10)]))      # (nine lists of ten: a stack need of 21, not 93)
    cam = rt.camera_new((7.5, 9.0, 18.0), (7.5, 2.0, 6.5), (0, 1, 0), 48.0, 1.5, 0.0, 14.0, 0.0, 1.0)
    return b, b.desc(), cam


def composite_boundary_scene(rt):
    """A medium whose boundary is a BVH of a box and a sphere: its two boundary queries are traversals of their own."""
    b = rt.DescBuilder()
    glass = b.dielectric(1.5)
    shell = b.node((-3, -3, -8), (3, 3, -2), b.box((-2, -1, -7), (0.5, 1, -4), glass), b.sphere((1.0, 0, -5), 1.5, glass))
    fog = b.medium(shell, 0.9, b.isotropic((0.8, 0.5, 0.3)))
    floor_ = b.rect(F.RT_RECT_XZ, -20, 20, -20, 20, -1.5, b.lambertian((0.5, 0.5, 0.5)))
    b.set_root(b.list([fog, floor_]))
    cam = rt.camera_new((0, 1, 4), (0, 0, -5), (0, 1, 0), 45.0, 48 / 36, 0.0, 9.0, 0.0, 1.0)
    return b.desc(), cam


def every_material_scene(rt):
    """Every material kind x every texture kind, a back-faced and a flipped light, movers at depth 4, a triangle, a ring,
    media, a moving sphere; no light list (n_lights == 0)."""
    b = rt.DescBuilder()
    g = np.random.default_rng(11)
    vec = g.normal(size=(256, 3))
    vec /= np.linalg.norm(vec, axis=1, keepdims=True)
    pl = b.perlin(vec, g.permutation(256), g.permutation(256), g.permutation(256))
    img = (np.arange(8 * 4 * 3, dtype=np.uint8).reshape(4, 8, 3) * 7) % 251
    textures = lambda: [b.solid((0.7, 0.3, 0.2)), b.checker(b.solid((0.2, 0.3, 0.1)), b.solid((0.9, 0.9, 0.9))), b.noise(pl, 4.0), b.image(img)]
    mats = ([b.lambertian(tex=t) for t in textures()] + [b.diffuse_light(tex=t) for t in textures()] +
            [b.metal((0.8, 0.7, 0.6), 0.3), b.dielectric(1.5)])
    refs = []
    for i, m in enumerate(mats):
        refs.append(b.sphere(((i % 5 - 2) * 1.2, (i // 5) * 1.2, 0.0), 0.45, m))
    glass = b.dielectric(1.5)
    for i, t in enumerate(textures()):                                      # isotropic x every texture: dense media
        refs.append(b.medium(b.sphere(((i - 1.5) * 1.2, 3.6, 0.0), 0.45, glass), 8.0, b.isotropic(tex=t)))
    floor_tex = b.checker(b.noise(pl, 2.0), b.image(img))                   # a checker of a noise and an image
    refs.append(b.rect(F.RT_RECT_XZ, -30, 30, -30, 30, -0.6, b.lambertian(tex=floor_tex)))
    refs.append(b.rect(F.RT_RECT_XZ, -3, 3, -4, 2, 4.3, b.diffuse_light((8, 8, 8))))               # seen from below: back face
    refs.append(b.rect(F.RT_RECT_XY, -6, -3.2, 0, 3, -1.0, b.diffuse_light((4, 5, 6)), flip=True))  # FlipFace ref
    tri_mat, ring_mat, box_mat = b.metal((0.1, 0.9, 0.5), 0.0), b.lambertian((0.9, 0.1, 0.9)), b.lambertian((0.3, 0.6, 0.9))
    refs.append(b.triangle((-4.2, -0.5, 1), (-3.0, -0.5, 1), (-3.6, 0.9, 1.5), tri_mat))
    refs.append(b.translate(b.ring(0.9, 0.3, ring_mat), (3.6, -0.3, 3.0)))
    deep = b.translate(b.rotate_y(b.zoom(b.translate(b.box((-0.4, 0, -0.4), (0.4, 0.8, 0.4), box_mat), (0.1, 0.0, 0.1)), 1.3),
                                  0.5, 0.8660254037844386), (3.8, 1.0, 0.5))
    refs.append(deep)
    mover_mat = b.lambertian((0.5, 0.5, 0.1))
    refs.append(b.moving_sphere((-3.8, 2.2, 0), (-3.8, 3.0, 0), 0, 1, 0.45, mover_mat))
    b.set_root(b.list(refs))
    named = {"triangle": tri_mat, "ring": ring_mat, "box": box_mat, "moving": mover_mat}
    return b, b.desc(), named


def every_kind_lit_scene(rt, lights=True):
    """One of each hittable kind (movers, a list, a flipped light, a medium, a moving sphere) and every texture kind."""
    b = rt.DescBuilder()
    lam = b.lambertian((0.6, 0.5, 0.4))
    img = (np.arange(8 * 4 * 3, dtype=np.uint8).reshape(4, 8, 3) * 7) % 251
    g = np.random.default_rng(11)
    pl = b.perlin(unit_vectors(g, 256), g.permutation(256), g.permutation(256), g.permutation(256))
    rect_light = b.rect(F.RT_RECT_XZ, -1, 1, -1, 1, 6.0, b.diffuse_light((8, 8, 8)), flip=True)
    ball_light = b.sphere((5, 6, -2), 0.7, b.diffuse_light((20, 18, 15)))
    refs = [
        b.sphere((0, -100, 0), 100.0, b.lambertian(tex=b.checker(b.solid((0.2, 0.3, 0.1)), b.solid((0.9, 0.9, 0.9))))),
        b.sphere((0, 1, 0), 1.0, b.lambertian(tex=b.image(img))),
        b.sphere((1.8, 0.6, 1.8), 0.6, b.lambertian(tex=b.noise(pl, 4.0))),
        b.moving_sphere((2.5, 0.5, 0), (2.5, 1.0, 0), 0, 1, 0.5, b.metal((0.8, 0.7, 0.6), 0.3)),
        b.sphere((-2.5, 1, 0), 1.0, b.dielectric(1.5)),
        b.triangle((-1, 0.01, 2), (1, 0.01, 2), (0, 1.5, 2.5), lam),
        b.translate(b.ring(1.5, 0.3, lam), (0, 0.5, -3)),
        b.translate(b.rotate_y(b.zoom(b.box((-0.5, 0, -0.5), (0.5, 1, 0.5), lam), 1.5), 0.5, 0.8660254037844386), (4.5, 0, 2)),
        b.list([rect_light, b.rect(F.RT_RECT_XY, -6, 6, 0, 4, -6.0, lam)]),
        b.medium(b.sphere((-4, 1, 2), 1.0, b.dielectric(1.5)), 0.8, b.isotropic((0.3, 0.3, 0.9))),
        ball_light,
    ]
    b.set_root(b.list(refs))
    if lights:
        b.light(rect_light)
        b.light(ball_light)
    cam = rt.camera_new((9, 4, 9), (0, 1, 0), (0, 1, 0), 35.0, 56 / 40, 0.0, 12.0, 0.0, 1.0)
    return b, b.desc(), cam
