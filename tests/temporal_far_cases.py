"""Cases for RT_TEMPORAL_FAR_MISSES (no scene, no GPU): cameras that turn, and frames with many miss records.
tests/test_surfaces_ref.py runs them through the far-miss restatement (tests/temporal_far_ref.py), tests/test_temporal_far.py
through the library."""
import math

import numpy as np

import temporal_cases as T
import temporal_ref as R


def turned(rt, W, H, angle, about="v"):
    """T.camera(W, H) turned by `angle` about its own v axis (a pan) or u axis (a tilt), the origin kept."""
    if about == "v":
        return T.camera(rt, W, H, lookat=(math.sin(angle), 0.0, -math.cos(angle)))
    return T.camera(rt, W, H, lookat=(0.0, math.sin(angle), -math.cos(angle)))


def far_cameras(rt, W, H):
    """T.cameras' pairs, and pairs that turn: a translation alone never moves a point at infinity."""
    base = T.camera(rt, W, H)
    pairs = dict(T.cameras(rt, W, H))
    pairs["panned"] = (base, turned(rt, W, H, 0.21))
    pairs["tilted and moved"] = (R.shifted_camera(turned(rt, W, H, -0.17, "u"), (0.3, -0.2, 0.1)), base)
    return pairs


def more_misses(feat, seed, frac=0.35):
    """A copy of the records with `frac` of the pixels turned into all-zero miss records."""
    f = feat.copy()
    H, W = f.shape
    f.view(np.float64).reshape(H, W, 8)[np.random.default_rng(seed).random((H, W)) < frac] = 0.0
    return f
