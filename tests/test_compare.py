"""tests/compare.py pinned: every bit-for-bit claim of the suite rests on it. What must fail fails — one ulp, the sign of a
zero, a NaN against a number, a shape, a record field's last bit — and a NaN's payload counts only where it is asked for.
No GPU."""
import numpy as np
import pytest

from raytracer_2022_amd import _ffi as F

from compare import assert_same_bits, bits, nan_bits, same_bits

NAN_A = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]      # the default quiet NaN
NAN_B = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]      # another sign and payload
BASE = np.array([1.0, -2.5, 0.0, np.inf, 1e-310, 3.0])


def differs(a, b):
    """a and b are told apart in every mode, either way round."""
    for x, y in ((a, b), (b, a)):
        if same_bits(x, y) or same_bits(x, y, payloads=True):
            return False
        with pytest.raises(AssertionError):
            assert_same_bits(x, y)
    return True


def agrees(a, b, payloads=True):
    assert_same_bits(a, b)
    assert_same_bits(b, a)
    return same_bits(a, b) and same_bits(b, a) and (not payloads or (same_bits(a, b, payloads=True) and same_bits(b, a, payloads=True)))


def test_one_ulp_fails():
    other = BASE.copy()
    other[1] = np.nextafter(other[1], 0.0)
    assert differs(BASE, other)
    other = BASE.copy()
    other[4] = np.nextafter(other[4], 1.0)                                       # a subnormal's last bit
    assert differs(BASE, other)


def test_the_sign_of_a_zero_fails():
    assert np.array_equal(np.array([0.0]), np.array([-0.0]))                     # (== cannot tell them apart)
    assert differs(np.array([1.0, 0.0]), np.array([1.0, -0.0]))


def test_a_nan_against_a_number_fails_either_way_round():
    for number in (0.0, 1.0, np.inf):
        assert differs(np.array([1.0, NAN_A]), np.array([1.0, number]))


def test_a_shape_mismatch_fails():
    assert differs(np.zeros(6), np.zeros((2, 3)))
    assert differs(np.zeros(3), np.zeros(4))
    assert differs(np.zeros((2, 3)), np.zeros((3, 2)))
    assert differs(np.zeros(0), np.zeros(1))


def test_nan_payloads_count_only_where_asked_for():
    a, b = np.array([1.0, NAN_A, 2.0]), np.array([1.0, NAN_B, 2.0])
    assert np.isnan(NAN_A) and np.isnan(NAN_B) and bits(a)[1] != bits(b)[1]
    assert agrees(a, b, payloads=False)
    assert not same_bits(a, b, payloads=True) and not same_bits(b, a, payloads=True)
    assert agrees(a, a.copy()) and agrees(b, b.copy())                           # equal payloads pass in every mode
    off = b.copy()
    off[2] = np.nextafter(off[2], 3.0)                                           # beside the NaN a last bit still counts
    assert differs(a, off)


RECORDS = {"feature": F.FEATURE_DTYPE, "temporal_pixel": F.TEMPORAL_PIXEL_DTYPE}


@pytest.mark.parametrize("record, field", [("feature", "depth"), ("feature", "hits"), ("feature", "albedo"),
                                           ("temporal_pixel", "n"), ("temporal_pixel", "normal"), ("temporal_pixel", "e")])
def test_records_differing_in_one_fields_last_bit_fail(record, field):
    a = np.zeros((2, 3), dtype=RECORDS[record])
    a.view(np.float64)[...] = np.arange(1.0, 49.0).reshape(2, 24)
    assert bits(a).shape == nan_bits(a)[0].shape == (2, 24)                      # records are the doubles they are made of
    b = a.copy()
    assert agrees(a, b)
    last = b[field][1, 2]
    b[field][1, 2] = np.nextafter(last, 0.0)                                     # (a vector field: all its components)
    assert differs(a, b)
    b = a.copy()
    b[field][1, 1, ...] = np.nan                                                 # a NaN in one record's field
    assert differs(a, b)
    assert agrees(b, b.copy())


def test_equal_inputs_pass_in_every_mode():
    hostile = np.array([0.0, -0.0, np.inf, -np.inf, NAN_A, NAN_B, 5e-324, 1.7976931348623157e308])
    assert agrees(hostile, hostile.copy())
    assert agrees(hostile.reshape(2, 4), hostile.reshape(2, 4).copy())
    assert agrees(np.zeros(0), np.zeros(0)) and agrees(np.zeros((0, 3)), np.zeros((0, 3)))
    assert agrees([1.0, 2.0], (1.0, 2.0)) and agrees(np.arange(4), np.arange(4.0))      # what converts to the same doubles
    assert agrees(hostile[::2], hostile[::2].copy())                             # a view that is not contiguous
    v, nan = nan_bits(hostile)
    assert nan.tolist() == [False] * 4 + [True, True, False, False] and v[4] == v[5] == 0
    assert np.array_equal(bits(hostile)[[0, 1]], np.array([0, 1 << 63], dtype=np.uint64))


def test_assert_same_bits_names_the_first_differing_index():
    a = np.arange(8.0).reshape(2, 4)
    b = a.copy()
    b[1, 2] = np.nextafter(b[1, 2], 9.0)
    b[1, 3] = -b[1, 3]
    with pytest.raises(AssertionError) as e:
        assert_same_bits(b, a, "the case")
    what, label, first, count = e.value.args[0]
    assert (what, label, first, count) == ("the case", "first differing doubles", [[1, 2], [1, 3]], 2)
    b = a.copy()
    b[0, 1] = np.nan
    with pytest.raises(AssertionError) as e:
        assert_same_bits(b, a, "nan case")
    assert e.value.args[0] == ("nan case", "NaN pattern")
    with pytest.raises(AssertionError) as e:
        assert_same_bits(a, a.reshape(4, 2), "shape case")
    assert e.value.args[0] == "shape case"
