"""Bit-for-bit comparison of doubles: the one routine behind every "same bits" claim of the suite. No GPU is needed;
tests/test_compare.py pins what passes and what fails here.

Three views of an array of doubles (FEATURE_DTYPE and TEMPORAL_PIXEL_DTYPE records count as the doubles they are made of):
`bits` is the plain uint64 view; `nan_bits` the pair (view with the NaNs zeroed, NaN mask), so that two results agree where
both have a NaN whatever its payload — 0 / 0 and inf * 0 need not agree on a sign (tests/test_shade_arms.py); `same_bits`
and `assert_same_bits` compare two arrays: equal shapes, NaNs in the same places, equal bits everywhere else, and with
payloads=True equal bits in the NaNs too."""
import numpy as np

from raytracer_2022_amd import _ffi as F

RECORD_DTYPES = (F.FEATURE_DTYPE, F.TEMPORAL_PIXEL_DTYPE)


def doubles(a):
    """`a` as a contiguous float64 array, records viewed as their doubles (eight to a record, along the last axis)."""
    a = np.ascontiguousarray(a)
    return a.view(np.float64) if a.dtype in RECORD_DTYPES else np.ascontiguousarray(a, dtype=np.float64)


def bits(a):
    """The uint64 view of the doubles, NaN payloads and all."""
    return doubles(a).view(np.uint64)


def nan_bits(a):
    """(the uint64 view with every NaN zeroed, the NaN mask)."""
    v = doubles(a)
    return np.where(np.isnan(v), np.float64(0), v).view(np.uint64), np.isnan(v)


def same_bits(a, b, *, payloads=False):
    """Equal shapes, NaNs in the same places and equal bits off the NaNs; payloads=True: the NaNs' bits as well."""
    (ab, an), (bb, bn) = nan_bits(a), nan_bits(b)
    if ab.shape != bb.shape or not np.array_equal(an, bn) or not np.array_equal(ab, bb):
        return False
    return not payloads or np.array_equal(bits(a), bits(b))


def assert_same_bits(got, ref, what=""):
    (gb, gn), (rb, rn) = nan_bits(got), nan_bits(ref)
    assert gb.shape == rb.shape, what
    assert np.array_equal(gn, rn), (what, "NaN pattern")
    bad = np.argwhere(gb != rb)
    assert len(bad) == 0, (what, "first differing doubles", bad[:5].tolist(), len(bad))
