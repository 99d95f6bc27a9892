"""The redraw loops of the path RNG on the device against the oracle, bit for bit, where the redraw fires and where it cannot.

rt_math.h peels the first draw of gen_range / gen_index out of their `tries < RT_MAX_REJECT` loops (the hot path then holds
one draw, tests/test_rng_draw_blocks.py). These cases pin what must not move: the same draws in the same order, the cap of
128 tries with the last value returned, and the number of words the generator has consumed afterwards.
"""
import ctypes as C

import numpy as np
import pytest

from raytracer_2022_amd import _ffi as F

from compare import bits

pytestmark = pytest.mark.gpu

N = 4096
GAMMA = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
STATE = 0x2022_0BAD_5EED_0001


def device(rt, mode, lo, hi, bound, n=N, state=STATE):
    out = (C.c_uint64 * n)()
    F.check(rt.lib().rt_debug_rng_device(state, mode, lo, hi, bound, out, n))
    return np.array(out[:], dtype=np.uint64)


def oracle_range(O, lo, hi, n=N, state=STATE):
    ref = (C.c_double * n)()
    O.lib().rto_rng_range(state, lo, hi, ref, n)
    return np.array(ref[:])


def oracle_index(O, bound, n=N, state=STATE):
    ref = (C.c_uint64 * n)()
    O.lib().rto_rng_index(state, bound, ref, n)
    return np.array(ref[:], dtype=np.uint64)


def oracle_u64(O, state, n):
    ref = (C.c_uint64 * n)()
    O.lib().rto_rng_u64(state, ref, n)
    return np.array(ref[:], dtype=np.uint64)


def test_unit_bounds_never_redraw(rt, O):
    """(-1, 1): res is a multiple of 2^-51 in [-1, 1 - 2^-51], computed exactly: one draw per value."""
    ref = oracle_range(O, -1.0, 1.0)
    assert np.array_equal(device(rt, 2, -1.0, 1.0, 0), bits(ref))
    # one word per value: the state after value i is STATE + (i + 1) * gamma
    want = np.array([(STATE + (i + 1) * GAMMA) & M64 for i in range(N)], dtype=np.uint64)
    assert np.array_equal(device(rt, 4, -1.0, 1.0, 0), want)


def test_redraw_fires_about_every_second_value(rt, O):
    """(1, 1 + 2^-52): the sum rounds to 1 or to `high`; `high` is redrawn — the slow path behind the peeled draw."""
    hi = float(np.nextafter(1.0, 2.0))
    ref = oracle_range(O, 1.0, hi)
    assert np.all(ref == 1.0)
    assert np.array_equal(device(rt, 2, 1.0, hi, 0), bits(ref))
    # the words consumed say that the redraw did fire: per value 1 / (1 - 1/2) = 2 expected; sd of the mean over 4096 values 0.022
    end = int(device(rt, 4, 1.0, hi, 0)[-1])
    words = ((end - STATE) & M64) * pow(GAMMA, -1, 1 << 64) & M64
    print("words consumed by %d values: %d" % (N, words))
    assert 1.85 * N < words < 2.15 * N
    # and the state is the oracle's: the next word of the device's stream is word `words + 1` of the oracle's
    assert int(oracle_u64(O, end, 1)[0]) == int(oracle_u64(O, STATE, words + 1)[-1])


@pytest.mark.parametrize("lo,hi", [(3.0, 3.0), (0.0, float("nan")), (float("nan"), 1.0)], ids=["lo_eq_hi", "nan_high", "nan_low"])
def test_cap_is_reached_and_state_advances_by_128_draws(rt, O, lo, hi):
    """No value is ever below `high`: 128 tries, the last one returned, 128 words consumed per value."""
    ref = oracle_range(O, lo, hi)
    got = device(rt, 2, lo, hi, 0).view(np.float64)
    if np.isnan(ref).any():
        # (a NaN's payload is not IEEE's business and differs between the two instruction sets: NaN where the oracle has NaN)
        assert np.isnan(ref).all() and np.isnan(got).all()
    else:
        assert np.array_equal(bits(got), bits(ref)) and np.all(got == lo)
    want = np.array([(STATE + 128 * (i + 1) * GAMMA) & M64 for i in range(N)], dtype=np.uint64)
    states = device(rt, 4, lo, hi, 0)
    assert np.array_equal(states, want)
    # gamma and the stride are the oracle's: word 128 * k + 1 of its stream is the first word after state k
    stream = oracle_u64(O, STATE, 128 * 64 + 1)
    for k in (1, 2, 64):
        assert int(oracle_u64(O, int(want[k - 1]), 1)[0]) == int(stream[128 * k])


@pytest.mark.parametrize("n", [(1 << 63) + 1, 1, 2], ids=["2^63+1", "1", "2"])
def test_gen_index_with_half_of_the_draws_rejected(rt, O, n):
    """zone = 2^63 (n = 2^63 + 1) or 2^63 - 1 (n = 1, 2): about every second draw is rejected and redrawn."""
    ref = oracle_index(O, n)
    assert np.array_equal(device(rt, 3, 0.0, 0.0, n), ref)
    end = int(device(rt, 5, 0.0, 0.0, n)[-1])
    words = ((end - STATE) & M64) * pow(GAMMA, -1, 1 << 64) & M64
    print("gen_index(%d): words consumed by %d values: %d" % (n, N, words))
    assert 1.85 * N < words < 2.15 * N
    assert int(oracle_u64(O, end, 1)[0]) == int(oracle_u64(O, STATE, words + 1)[-1])
