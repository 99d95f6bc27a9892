"""Leaf sets for the BVH builder tests (tests/test_bvh_ref.py on the CPU, tests/test_bvh_gpu.py on the device): random boxes,
the hostile sets and the deep chain. → (refs uint32 (n,), boxes6 float64 (n, 6)); everything is decided by the seed."""
import numpy as np

from raytracer_2022_amd import _ffi as F

HOSTILE = ("identical", "line", "plane", "duplicated", "cluster_and_far", "points", "flips_and_nodes")


def sphere_refs(n, first=0):
    return (np.uint32(F.RT_KIND_SPHERE << F.RT_REF_KIND_SHIFT) | np.arange(first, first + n, dtype=np.uint32)).astype(np.uint32)


def random_boxes(n, seed):
    g = np.random.default_rng(seed)
    c, h = g.uniform(-50.0, 50.0, (n, 3)), g.uniform(0.01, 1.5, (n, 3))
    return sphere_refs(n), np.concatenate([c - h, c + h], axis=1)


def hostile(kind, n, seed=11):
    g = np.random.default_rng(seed)
    refs, boxes = random_boxes(n, seed)
    if kind == "identical":                              # one key: the index tie-break builds the whole tree
        boxes[:] = boxes[0]
    elif kind in ("line", "plane"):                      # centres on one line / one plane, equal half sizes: zero-extent axes
        flat = (1, 2) if kind == "line" else (2,)
        c = g.uniform(-50.0, 50.0, (n, 3))
        c[:, flat] = 0.25
        boxes = np.concatenate([c - 0.5, c + 0.5], axis=1)
    elif kind == "duplicated":                           # every box twice, under different refs
        boxes[n // 2:2 * (n // 2)] = boxes[:n // 2]
    elif kind == "cluster_and_far":                      # all keys but one collapse into one cell
        c = g.uniform(-1.0, 1.0, (n, 3)) * 1e-3
        c[n // 3] = 1e12
        boxes = np.concatenate([c - 1e-4, c + 1e-4], axis=1)
    elif kind == "points":
        boxes[:, 3:] = boxes[:, :3]
    else:                                                # flip bits kept as given; NODE refs as leaves (subtrees)
        assert kind == "flips_and_nodes"
        refs = refs.copy()
        refs[::3] |= np.uint32(F.RT_REF_FLIP)
        refs[1::3] = np.arange(len(refs[1::3]), dtype=np.uint32) + np.uint32(1 << 20)      # kind 0 = NODE, far from any node_base used
    return refs, boxes


def chain(n=4096):
    """Unit boxes whose lower corners lie at 2^21 * 2^-i along x, given in ascending x: each split takes one box off the top
    and leaves the rest on the LEFT, until the keys collapse into cell 0 and the index tie-break takes over."""
    x = np.sort(np.ldexp(1.0, 21 - np.arange(n)))
    lo = np.stack([x, np.zeros(n), np.zeros(n)], axis=1)
    return sphere_refs(n), np.concatenate([lo, lo + 1.0], axis=1)
