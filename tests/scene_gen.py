"""Seeded random scene graphs inside what rt_scene_create accepts: generate(seed, profile) -> (builder, desc, cameras, facts).
A helper module, not a test: tests/test_scene_gen.py holds the oracle to the BVH-free references on its output, and
tests/test_scene_gen_gpu.py every entry point of the device.

A scene is a pure function of (seed, profile) through np.random.default_rng: no clock, no environment, no GPU. It is built
with rt.DescBuilder only; built BVHs come from b.bvh(refs, build=bvh_ref.build), the CPU builder, and every hand-made node's
box is the union of rt.ref_boxes of its children over the shutter [0, 1] (the reference's bounding_box rule).

The grammar, recursive. gen(P, h) makes a sub-graph round the point P of the CURRENT frame with half-extent about h:
  leaf      sphere, moving sphere, rect (three axes), box, triangle, ring; a random FlipFace bit each. A ring lies in y = 0
            round its frame's origin, so it is made only where P is that origin: straight under a Translate by P, with
            RotateYs and Zooms (which keep the origin) between, or at the world's origin where the profile has no movers
  mover     Translate (any offset; the child is made round P - offset), RotateY (any angle of the circle; the child round R P),
            Zoom (rate 1, or 0.5 .. 2: the child round P / rate with h / rate), nested to RT_MAX_XFORM_DEPTH, FlipFace bits on
            mover refs
  list      1 to 4 items, nested; more than one item halves h
  node      a built BVH of 2 to 4 items; a hand-made node of two; a span-1 node (the same child twice); at the root of the
            chain profiles a left-leaning chain of hand-made nodes that raises the stack need
  medium    Isotropic, never inside a boundary; the boundary one primitive under 0 to 2 movers (the megakernel takes these) or
            a node / list of two primitives (wavefront only)
  shared    one sub-graph made round its frame's origin and referenced by two parents under different movers
  pair      one leaf straight under one mover, and
  chain     one leaf under a Translate, a RotateY and a Zoom in any order: top-level forms that take the next (leaf kind, mover kind,
            flip parity) of a shuffled deck, so that a scene of a dozen sub-graphs does not leave the combinations to luck
Kinds are drawn from shuffled decks too (every kind comes up before one repeats). The profile "movers" is systematic: its top-level
sub-graphs are the 42 pair and chain combinations in turn, 21 a seed, under a list (no node above a Zoom).
FlipFace never sits on a node or list ref; nothing else check_scene refuses is made (tests/test_abi.py holds the refusals).

Sizes: top-level sub-graphs sit in the cells (pitch 3.6) of a 3 x 3 x 3 grid round the origin, h = 1.7; composites halve h twice
at most, and a leaf's half-extent is at least 0.95 h, so every leaf has a WORLD half-extent >= 0.4 (a Zoom scales its child's
frame: h is divided by the rate on the way in). The arena reaches 5.3 + movers' play from the origin; the outer camera is 14
away, so nothing is seen from over 25: (r / distance)^2 > (0.4 / 25)^2 = 2.6e-4 > brute_hits.MARGIN for a central hit. The
inner camera stands between cells.

A Zoom of rate != 1 sits under a node in the profile "class2" alone (brute_hits' class 2 cannot occur elsewhere): elsewhere a
Zoom below any node has rate 1, and rates != 1 occur above every node of their path (profile "lists").
"""
import functools

import numpy as np

import raytracer_2022_amd as rt
from raytracer_2022_amd import _ffi as F

import brute_hits as B
import brute_scenes as S
import bvh_ref
import trace_scenes as T

MAX_PATHS = 64
PITCH, H_TOP, MIN_HALF = 3.6, 1.7, 0.4
SPHERE, MOVING, RECT, BOX, TRIANGLE, RING = "sphere", "moving_sphere", "rect", "box", "triangle", "ring"
KINDS = (SPHERE, MOVING, RECT, BOX, TRIANGLE, RING)
BASE = (SPHERE, MOVING, RECT)

# profile -> what its grammar may use. kinds: leaf kinds; movers / lists / media: whether those records occur at all (they set
# the feature word); root: "bvh" (a built BVH over the top-level sub-graphs), "list", or "chain" (a built BVH under a chain cut
# to the stack need `need`); pad_nodes: the node pool is filled up to that many records with unreachable span-1 nodes (legal:
# rt.rebuild_bvh leaves such records too) — 1741 nodes cannot be REACHED by 64 leaf paths under a stack need of 16, and
# choose_trace reads the pool's count; zoom_under_node: see above; top: top-level sub-graphs.
def _profile(kinds, movers=False, lists=False, media=False, root="bvh", need=None, pad_nodes=0, zoom_under_node=False, top=11):
    return dict(kinds=kinds, movers=movers, lists=lists, media=media, root=root, need=need, pad_nodes=pad_nodes,
                zoom_under_node=zoom_under_node, top=top)


PROFILES = {
    "feat0": _profile(BASE),
    "feat1": _profile(BASE + (TRIANGLE, RING)),
    "feat2": _profile(BASE, movers=True, lists=True),
    "feat3": _profile(BASE + (TRIANGLE, RING), movers=True, lists=True),
    "feat4": _profile(BASE + (BOX,), media=True),
    "feat5": _profile(KINDS, media=True),
    "feat6": _profile(BASE + (BOX,), movers=True, lists=True, media=True),
    "feat7": _profile(KINDS, movers=True, lists=True, media=True),
    "spheres": _profile((SPHERE, MOVING)),                                   # no rect: the all-in-LDS `prims` instance
    "partial": _profile(KINDS, movers=True, lists=True, media=True, pad_nodes=T.NODE_CACHE + 1),
    "need22": _profile(BASE + (TRIANGLE, RING), movers=True, lists=True, root="chain", need=T.STACK_TINY + 1, top=7),     # f32 records in the plain kernel
    "need30": _profile(KINDS, movers=True, lists=True, media=True, root="chain", need=T.STACK_SMALL + 1, top=7),
    "need64": _profile(KINDS, media=True, root="chain", need=T.STACK_MID + 1, top=6),
    "lists": _profile(KINDS, movers=True, lists=True, media=True, root="list"),
    "class2": _profile(KINDS, movers=True, lists=True, media=True, zoom_under_node=True),
    # every (leaf kind, mover kind, flip parity) and every leaf kind under all three movers, in turn: top-level sub-graph i of
    # seed s is combination 21 s + i of the 42, so two seeds hold each once. What the grammar's own draws reach only by luck.
    "movers": _profile(KINDS, movers=True, lists=True, root="list", top=26),
}
COMBOS = [(k, m, f) for k in KINDS for m in "TRZ" for f in (False, True)] + [(k, None, None) for k in KINDS]
# The committed scenes. A gap in the coverage table of tests/test_scene_gen.py is closed by adding a seed here.
SEEDS = {"feat0": (1, 2), "feat1": (1, 2), "feat2": (1, 2), "feat3": (1, 2), "feat4": (1, 2), "feat5": (2, 3), "feat6": (1, 2),
         "feat7": (1, 2), "spheres": (1,), "partial": (1,), "need22": (1,), "need30": (1,), "need64": (1,), "lists": (1, 2),
         "class2": (1,), "movers": (0, 1, 2, 3)}
CASES = [(p, s) for p, seeds in SEEDS.items() for s in seeds]


def case_id(case):
    return "%s-%d" % case


# ---- frames ------------------------------------------------------------------------------------------------------------------
def _into(kind, par, P):
    """A point of the mover's frame in its child's frame (brute_hits.ray_in on points)."""
    if kind == "T":
        return P - par
    if kind == "R":
        s, c = par
        return np.array([c * P[0] - s * P[2], P[1], s * P[0] + c * P[2]])
    return P / par


class _Gen:
    def __init__(self, seed, name):
        self.name, self.pr, self.seed = name, PROFILES[name], seed
        self.g = np.random.default_rng([seed, list(PROFILES).index(name)])
        self.b = rt.DescBuilder()
        self.decks = {}
        self.paths = 0                                   # leaf paths made so far (a shared sub-graph counts per parent)
        self.composite_ok = bool(self.g.random() < 0.5)   # whether this scene's media may have composite boundaries (mega_refuses)
        self.facts = dict(profile=name, seed=seed, span1_nodes=[], one_item_lists=[], one_item_leaves=set(), shared_leaves=set(),
                          composite_boundaries=0, simple_boundaries=0, ring_boundaries=0, built_bvhs=0, hand_nodes=0, chain_links=0, padded_nodes=0,
                          max_mover_depth=0, zoom_rates=set(), checker_depth=0)
        self._materials()

    # -- materials and textures: every kind, made once per scene
    def _materials(self):
        b, g = self.b, self.g
        vec = g.normal(size=(256, 3))
        per = b.perlin(vec / np.linalg.norm(vec, axis=1, keepdims=True), g.permutation(256), g.permutation(256), g.permutation(256))
        img = b.image(g.integers(0, 256, (int(g.integers(2, 7)), int(g.integers(2, 9)), 3), dtype=np.uint8))
        noise = b.noise(per, float(g.uniform(1.0, 6.0)))
        col = lambda: tuple(g.uniform(0.1, 0.9, 3))
        depth = int(g.integers(1, 9))                    # a checker chain of 1 to 8 checkers (kCheckerDepth)
        self.facts["checker_depth"] = depth
        chk = [noise, img, b.solid(col())][int(g.integers(0, 3))]
        for _ in range(depth):
            chk = b.checker(chk, b.solid(col())) if g.random() < 0.5 else b.checker(b.solid(col()), chk)
        self.solids = [b.lambertian(col()), b.lambertian(tex=chk), b.lambertian(tex=noise), b.lambertian(tex=img), b.metal(col(), 0.0),
                       b.metal(col(), float(g.uniform(0.05, 0.6))), b.dielectric(1.5), b.diffuse_light(tuple(g.uniform(2.0, 9.0, 3))),
                       b.diffuse_light(tex=img), b.isotropic(col())]
        self.weights = np.array([4, 3, 2, 2, 1, 1, 2, 1, 1, 0.5])
        self.weights /= self.weights.sum()
        self.fog_textures = [None, noise, chk]
        self.glass = self.solids[6]
        self.lamp = self.solids[7]

    def mat(self):
        return self.solids[int(self.g.choice(len(self.solids), p=self.weights))]

    # -- leaves
    def leaf(self, kind, P, h, mat=None, flip=None):
        """A leaf of half-extent in [0.95 h, h] round P (a ring: round the frame's origin, P is ignored)."""
        b, g = self.b, self.g
        m = self.mat() if mat is None else mat
        flip = bool(g.random() < 0.4) if flip is None else flip
        e = lambda n=None: h * g.uniform(0.95, 1.0, n)
        self.paths += 1
        if kind == SPHERE:
            return b.sphere(tuple(P), float(e()), m, flip=flip)
        if kind == MOVING:
            c1 = P + h * g.uniform(-0.2, 0.2, 3)                  # (the radius + the travel: inside 1.35 h of P)
            return b.moving_sphere(tuple(P), tuple(c1), 0.0, 1.0, float(e()), m, flip=flip)
        if kind == RECT:
            axis = int(g.integers(0, 3))
            ka, aa, ba = B.RECT_AXES[axis]
            ea, eb = e(), e()
            return b.rect(axis, float(P[aa] - ea), float(P[aa] + ea), float(P[ba] - eb), float(P[ba] + eb), float(P[ka] + h * g.uniform(-0.3, 0.3)), m, flip=flip)
        if kind == BOX:
            ext = e(3)
            return b.box(tuple(P - ext), tuple(P + ext), m, flip=flip)
        if kind == TRIANGLE:
            # three points on the sphere of radius h round P, two of them near the ends of an axis: a half-extent of at least 0.95 h
            while True:
                axis = np.eye(3)[int(g.integers(0, 3))]
                v = np.stack([axis, -axis, np.zeros(3)]) + g.normal(size=(3, 3)) * np.array([[0.1], [0.1], [1.0]])
                v /= np.linalg.norm(v, axis=1, keepdims=True)
                n = np.cross(v[1] - v[0], v[2] - v[0])
                if np.ptp(v, axis=0).max() >= 1.9 and np.linalg.norm(n) > 1.8 and abs(n[2]) / np.linalg.norm(n) > 0.05:
                    break
            return b.triangle(*(tuple(P + h * x) for x in v), m, flip=flip)
        assert kind == RING
        outer = float(e())
        t = float(outer * g.uniform(0.15, 0.3))
        return b.ring(outer - t, t, m, flip=flip)

    def draw(self, name, items, ok=lambda x: True):
        """The next item of a shuffled deck of `items` that ok() takes (the deck is reshuffled when it runs out): every kind
        comes up before one repeats, which a scene of a dozen sub-graphs needs to reach the combinations."""
        deck = self.decks.setdefault(name, [])
        for _ in range(2):
            for i, x in enumerate(deck):
                if ok(x):
                    return deck.pop(i)
            deck += [items[i] for i in self.g.permutation(len(items))]
        raise AssertionError("no item of the deck fits")

    def leaf_kind(self, at_origin):
        if at_origin and RING in self.pr["kinds"] and self.g.random() < 0.5:      # (the few places a ring fits)
            return RING
        kinds = [k for k in self.pr["kinds"] if k != RING]
        return self.draw("leaf", kinds + [TRIANGLE] * (TRIANGLE in kinds))       # (twice: a triangle is a thin target and wins few rays)

    # -- boxes
    def union_box(self, refs):
        bx = rt.ref_boxes(self.b.desc(), refs, 0.0, 1.0)
        return tuple(bx[:, :3].min(0)), tuple(bx[:, 3:].max(0))

    def hand_node(self, left, right):
        lo, hi = self.union_box([left, right])
        ref = self.b.node(lo, hi, left, right)
        if left == right:
            self.facts["span1_nodes"].append(F.ref_index(ref))
        else:
            self.facts["hand_nodes"] += 1
        return ref

    def built_bvh(self, refs):
        self.facts["built_bvhs"] += 1
        return self.b.bvh(refs, build=bvh_ref.build)

    # -- the recursion
    def parts(self, P, h, k):
        """k sub-cells of half-extent h / 2 in the cell (P, h): distinct corners."""
        corners = np.array([(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=float)
        pick = self.g.permutation(8)[:k]
        return [P + 0.5 * h * corners[i] for i in pick]

    def gen(self, P, h, world, xdepth, under_node, in_boundary, at_origin=False, level=0):
        """A sub-graph round P with half-extent about h; `world` the product of the Zoom rates above (h * world is the world's
        half-extent), xdepth the movers above."""
        g, pr = self.g, self.pr
        can_split = 0.5 * h * world * 0.95 >= MIN_HALF and level < 3
        forms, w = ["leaf"], [3.0]
        if pr["movers"] and xdepth < F.RT_MAX_XFORM_DEPTH:
            forms.append("mover"); w.append(5.0 if xdepth == 0 else 3.0)
            if xdepth == 0:
                forms.append("chain"); w.append(2.5)
                forms.append("pair"); w.append(3.0)
        if pr["lists"] and level < 3:
            forms.append("list"); w.append(1.5)
        if not in_boundary and level < 3:
            forms.append("node"); w.append(1.5)
        if pr["media"] and not in_boundary:
            forms.append("medium"); w.append(1.2)
        form = forms[int(g.choice(len(forms), p=np.array(w) / sum(w)))]
        if form == "leaf":
            return self.leaf(self.leaf_kind(at_origin), P, h)
        if form == "mover":
            return self.mover(P, h, world, xdepth, under_node, in_boundary, at_origin, level)
        if form == "chain":
            return self.full_chain(P, h, world, under_node, in_boundary)
        if form == "pair":                                       # one leaf straight under one mover, every (kind, mover) pair in turn
            kind, mv, parity = self.draw("pair", [(k, m, f) for k in pr["kinds"] for m in "TRZ" for f in (False, True)])
            return self.full_chain(P, h, world, under_node, in_boundary, kind, ["T", mv] if kind == RING and mv != "T" else [mv], parity)
        if form == "list":
            k = int(g.integers(1, 5)) if can_split else 1
            if k == 1:
                before = self.paths
                item = self.gen(P, h, world, xdepth, under_node, in_boundary, at_origin, level + 1)
                ref = self.b.list([item])
                self.facts["one_item_lists"].append(F.ref_index(ref))
                if F.RT_KIND_SPHERE <= F.ref_kind(item) <= F.RT_KIND_RING and self.paths == before + 1:
                    self.facts["one_item_leaves"].add(int(item))
                return ref
            return self.b.list([self.gen(Q, 0.5 * h, world, xdepth, under_node, in_boundary, False, level + 1) for Q in self.parts(P, h, k)])
        if form == "node":
            sort = g.random()
            if sort < 0.3 or not can_split:                      # span-1
                child = self.gen(P, h, world, xdepth, True, in_boundary, at_origin, level + 1)
                return self.hand_node(child, child)
            k = 2 if sort < 0.65 else int(g.integers(2, 5))
            kids = [self.gen(Q, 0.5 * h, world, xdepth, True, in_boundary, False, level + 1) for Q in self.parts(P, h, k)]
            return self.hand_node(*kids) if sort < 0.65 else self.built_bvh(kids)
        assert form == "medium"
        return self.medium(P, h, world, xdepth, under_node)

    def mover(self, P, h, world, xdepth, under_node, in_boundary, at_origin, level, child=None, kind=None, to_origin=None, flip=None):
        """A mover round P; `child`: a maker (P', h', world', at_origin') -> ref, default the grammar's gen."""
        g, b = self.g, self.b
        flip = bool(g.random() < 0.4) if flip is None else flip
        kind = kind or self.draw("mover", "TRZ")
        self.facts["max_mover_depth"] = max(self.facts["max_mover_depth"], xdepth + 1)
        child = child or (lambda Q, hh, ww, ao: self.gen(Q, hh, ww, xdepth + 1, under_node, in_boundary, ao, level))
        if kind == "T":
            to_origin = bool(g.random() < 0.4) if to_origin is None else to_origin
            off = P.copy() if to_origin else P - h * g.uniform(-1.5, 1.5, 3)
            return b.translate(child(_into("T", off, P), h, world, to_origin), tuple(off), flip=flip)
        if kind == "R":
            a = g.uniform(-np.pi, np.pi)
            s, c = float(np.sin(a)), float(np.cos(a))
            return b.rotate_y(child(_into("R", (s, c), P), h, world, at_origin), s, c, flip=flip)
        rate = 1.0
        if (self.pr["zoom_under_node"] or not under_node) and g.random() < 0.7:
            rate = float(g.uniform(0.5, 2.0))
        self.facts["zoom_rates"].add(rate)
        # (a node BELOW such a Zoom is fine: class 2 needs the node above it)
        return b.zoom(child(_into("Z", rate, P), h / rate, world * rate, at_origin), rate, flip=flip)

    def full_chain(self, P, h, world, under_node, in_boundary, kind=None, order=None, parity=None):
        """One leaf under a Translate, a RotateY and a Zoom in any order (a ring: the Translate outermost, to the ring's origin);
        or under the movers of `order`. parity: the parity of the FlipFace bits on the path (random bits on the movers, the leaf's
        bit makes up the rest)."""
        g = self.g
        kind = kind or self.draw("chain-leaf", list(self.pr["kinds"]))
        if order is None:
            order = ["T"] + [("R", "Z")[i] for i in g.permutation(2)] if kind == RING else ["TRZ"[i] for i in g.permutation(3)]

        flips = [bool(g.random() < 0.4) for _ in order]

        def make(Q, hh, ww, ao, left=tuple(order), depth=0):
            if not left:
                return self.leaf(kind, Q, hh, flip=None if parity is None else bool(parity != (sum(flips) % 2 == 1)))
            return self.mover(Q, hh, ww, depth, under_node, in_boundary, ao, 3, kind=left[0], to_origin=True if kind == RING else None,
                              flip=flips[depth], child=lambda Q2, h2, w2, ao2: make(Q2, h2, w2, ao2, left[1:], depth + 1))
        return make(P, h, world, False)

    def boundary(self, P, h, world, xdepth, under_node):
        """→ (ref, simple): one primitive under 0 to 2 movers, or a node / list of two primitives."""
        g, pr = self.g, self.pr
        closed = list(pr["kinds"])                              # (every leaf kind may bound a medium; only shells give a chord)
        split = 0.5 * h * world * 0.95 >= MIN_HALF                # (room for two primitives side by side)
        if not self.composite_ok or not split or g.random() < 0.5:            # simple
            n_movers = int(g.integers(0, 3)) if pr["movers"] else 0
            n_movers = min(n_movers, F.RT_MAX_XFORM_DEPTH - xdepth)

            # spheres and boxes (closed shells) half the time: only those give a chord; a ring under a Translate to its origin
            shells = [k for k in closed if k in (SPHERE, MOVING, BOX)]
            ring_fits = pr["movers"] and xdepth < F.RT_MAX_XFORM_DEPTH
            kind = self.draw("shell", shells) if g.random() < 0.5 else self.draw("boundary", closed + [k for k in (TRIANGLE, RING) if k in closed], lambda k: k != RING or ring_fits)
            if RING in closed and ring_fits and not self.facts["ring_boundaries"]:       # (the rarest boundary: once per scene where it fits)
                kind = RING
            if kind == RING:
                n_movers = max(1, n_movers)
                self.facts["ring_boundaries"] += 1

            def make(Q, hh, ww, ao, left=n_movers, depth=xdepth):
                if left == 0:
                    return self.leaf(kind, Q, hh, mat=self.glass)
                first = kind == RING and left == n_movers
                return self.mover(Q, hh, ww, depth, under_node, True, ao, 3, kind="T" if first else (self.draw("ring-mover", "RZ") if kind == RING else None),
                                  to_origin=True if first else None, child=lambda Q2, h2, w2, ao2: make(Q2, h2, w2, ao2, left - 1, depth + 1))
            return make(P, h, world, False), True
        kinds = [k for k in closed if k != RING]
        halves = self.parts(P, h, 2)
        a = self.leaf(kinds[int(g.integers(0, len(kinds)))], halves[0], 0.5 * h, mat=self.glass)
        c = self.leaf(kinds[int(g.integers(0, len(kinds)))], halves[1], 0.5 * h, mat=self.glass)
        if pr["lists"] and g.random() < 0.5:
            return self.b.list([a, c]), False
        return self.hand_node(a, c), False

    def medium(self, P, h, world, xdepth, under_node):
        shell, simple = self.boundary(P, h, world, xdepth, under_node)
        self.facts["simple_boundaries" if simple else "composite_boundaries"] += 1
        # a phase function of its own per medium: brute_records tells a medium under movers from a plain one by its material
        tex = self.fog_textures[int(self.g.integers(0, len(self.fog_textures)))]
        fog = self.b.isotropic(tuple(self.g.uniform(0.1, 0.9, 3))) if tex is None else self.b.isotropic(tex=tex)
        return self.b.medium(shell, float(self.g.uniform(0.3, 3.0)), fog)

    # -- the scene
    def shared(self, Pa, Pb, h):
        """One sub-graph round its frame's origin under two parents with different movers."""
        g, b = self.g, self.b
        before = self.paths
        zero = np.zeros(3)
        kinds = [k for k in self.pr["kinds"]]
        pair = [self.leaf(kinds[int(g.integers(0, len(kinds)))], Q, 0.5 * h) for Q in self.parts(zero, h, 2)]
        if RING in kinds and g.random() < 0.5:
            self.paths -= 1
            pair[1] = self.leaf(RING, zero, h)
        sub = b.list(pair) if g.random() < 0.5 else self.hand_node(*pair)
        self.paths += self.paths - before                        # the second parent walks it again
        self.facts["shared_leaves"].update(int(r) for r in pair)
        a = g.uniform(-np.pi, np.pi)
        s, c = float(np.sin(a)), float(np.cos(a))
        first = b.translate(sub, tuple(Pa), flip=bool(g.random() < 0.3))
        second = b.translate(b.rotate_y(sub, s, c), tuple(Pb)) if g.random() < 0.5 else b.translate(b.zoom(sub, 1.0, flip=True), tuple(Pb))
        self.facts["max_mover_depth"] = max(self.facts["max_mover_depth"], 2)
        return first, second

    def build(self):
        g, b, pr = self.g, self.b, self.pr
        cells = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=float) * PITCH
        cells = cells[g.permutation(len(cells))]
        cells = cells + g.uniform(-0.1, 0.1, cells.shape)
        tops, at = [], 0
        budget = MAX_PATHS
        # lights first: 0 to 3 top-level leaves with an emitting material, kinds of every light arm (sphere, rect, FlipFace, default)
        n_lights = int(g.choice([0, 1, 2, 3], p=[0.2, 0.3, 0.3, 0.2]))
        light_kinds = [k for k in pr["kinds"] if k != RING]
        for i in range(n_lights):
            kind = light_kinds[int(g.integers(0, len(light_kinds)))] if g.random() < 0.4 else (RECT if RECT in pr["kinds"] and g.random() < 0.5 else SPHERE)
            flip = bool(g.random() < 0.4)
            ref = self.leaf(kind, cells[at], 0.6 * H_TOP, mat=self.lamp, flip=flip)
            at += 1
            tops.append(ref)
            b.light(ref if g.random() < 0.5 else ref & ~F.RT_REF_FLIP)       # (scene.rs lists the plain object; a FlipFace entry is legal too)
        if RING in pr["kinds"] and not pr["movers"]:             # the one place a ring fits without a Translate
            tops.append(self.leaf(RING, np.zeros(3), 0.8 * H_TOP))
        if pr["movers"]:
            tops += self.shared(cells[at], cells[at + 1], 0.8 * H_TOP)
            at += 2
        if pr["root"] == "chain":
            budget = MAX_PATHS - 30                              # every link gets a leaf of its own: the oracle and the kernels walk
            # a span-1 node's child twice, as BvhNode::hit does, so a chain of span-1 links would double the work link by link
        first = len(tops)
        while len(tops) < pr["top"] and at < len(cells) and len(tops) - first < 21:
            before = self.paths
            if self.name == "movers":
                kind, mv, parity = COMBOS[(21 * self.seed + len(tops) - first) % len(COMBOS)]
                ref = self.full_chain(cells[at], H_TOP, 1.0, False, False, kind, None if mv is None else (["T", mv] if kind == RING and mv != "T" else [mv]), parity)
            else:
                ref = self.gen(cells[at], H_TOP, 1.0, 0, pr["root"] != "list", False)
            if self.paths > budget:                              # would outgrow the cap: this cell stays empty (the records stay, unreachable)
                self.paths = before
                break
            tops.append(ref)
            at += 1
        if pr["root"] == "list":
            root = b.list(tops)
        else:
            root = self.built_bvh(tops)
        if pr["root"] == "chain":
            b.set_root(root)
            links = pr["need"] - T.stack_need(b.desc())
            assert links > 0
            kinds = [k for k in pr["kinds"] if k not in (RING, RECT, TRIANGLE)]
            assert links <= 30
            for i in range(links):                               # a leaf of its own per link, on two circles above and below the arena
                a = 2 * np.pi * (i % 15) / 15
                P = np.array([4.6 * np.cos(a), 6.6 if i < 15 else -6.6, 4.6 * np.sin(a)])
                root = self.hand_node(root, self.leaf(kinds[i % len(kinds)], P, 0.55))
            self.facts["chain_links"] = links
        while len(b.pools["nodes"]) < pr["pad_nodes"]:
            r = tops[len(b.pools["nodes"]) % len(tops)]
            b.node((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), r, r)
            self.facts["padded_nodes"] += 1
        b.set_root(root)
        d = b.desc()
        d._builder = b
        cams = (rt.camera_new((8.5, 5.5, 9.7), (0.0, 0.0, 0.0), (0, 1, 0), 50.0, 4 / 3, 0.0, 14.0, 0.0, 1.0),       # 14.0 from the origin
                rt.camera_new((1.8, 0.3, 1.8), (-3.0, 0.6, -2.0), (0, 1, 0), 80.0, 4 / 3, 0.0, 4.0, 0.0, 1.0))     # between the cells
        live = _reachable(d)
        f = self.facts
        f["span1_nodes"] = sorted(i for i in f["span1_nodes"] if (F.RT_KIND_NODE, i) in live)
        f["one_item_lists"] = sorted(i for i in f["one_item_lists"] if (F.RT_KIND_LIST, i) in live)
        f["one_item_leaves"] = {r for r in f["one_item_leaves"] if (F.ref_kind(r), F.ref_index(r)) in live}
        self.facts.update(paths=self.paths, n_lights=n_lights, feature_word=T.feature_word(d), stack_need=T.stack_need(d),
                          mega_refuses=T.mega_refuses(d), top=len(tops))
        return b, d, cams, self.facts


def _reachable(d):
    """{(kind, index)} of the records reached from the root (a sub-graph dropped for the path cap stays in the pools)."""
    seen, stack = set(), [int(d.root)]
    while stack:
        ref = stack.pop()
        kind, idx = F.ref_kind(ref), F.ref_index(ref)
        if (kind, idx) in seen:
            continue
        seen.add((kind, idx))
        if kind == F.RT_KIND_NODE:
            stack += [int(d.nodes[idx].left), int(d.nodes[idx].right)]
        elif kind == F.RT_KIND_LIST:
            stack += [int(d.list_items[d.lists[idx].first + i]) for i in range(d.lists[idx].count)]
        elif kind == F.RT_KIND_MEDIUM:
            stack.append(int(d.media[idx].boundary))
        elif F.RT_KIND_TRANSLATE <= kind <= F.RT_KIND_ZOOM:
            stack.append(int(d.xforms[idx].child))
    return seen


def generate(seed, profile):
    """→ (builder, desc, (outer camera, inner camera), facts). The desc keeps its builder alive."""
    return _Gen(seed, profile).build()


# ---- what both test modules run on a generated scene -----------------------------------------------------------------------------
N_RAYS = S.N_RAYS                                            # per camera: four families of 500
CAMERAS = ("outer", "inner")


@functools.lru_cache(maxsize=None)
def solved(profile, seed):
    """(builder, desc, cams, facts, Scene, {(camera, family): (rays, Answer)}): the reference is computed once per scene and
    shared, unchanged."""
    b, d, cams, facts = generate(seed, profile)
    sc = B.Scene(d)
    fams = {}
    for ci, cam in enumerate(cams):
        for family, rays in B.ray_families(sc, *B.camera_of(cam), N_RAYS, 1000 * seed + 10 * list(PROFILES).index(profile) + ci).items():
            fams[(CAMERAS[ci], family)] = (rays, B.solve(sc, rays["origin"], rays["direction"], rays["time"], rays["t_min"], rays["t_max"]))
    return b, d, cams, facts, sc, fams
