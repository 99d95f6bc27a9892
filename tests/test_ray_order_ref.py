"""rt_ray_order's restatement (tests/ray_order_ref.py) against itself, without a GPU: the numpy form — what the device is held to,
tests/test_ray_order_gpu.py — against the per-ray loop in Python floats and integers, bit for bit, and the properties the
definition promises."""
import numpy as np
import pytest

import ray_order_cases as K
import ray_order_ref as R


def check_order(rays, ob, db, layout, what):
    key = R.keys(rays, ob, db, layout)
    order = R.order(rays, ob, db, layout)
    n = len(rays)
    assert order.dtype == np.uint32 and np.array_equal(np.sort(order), np.arange(n)), (what, "not a permutation")
    ks = key[order]
    assert np.all(ks[:-1] <= ks[1:]), (what, "keys decrease")
    tie = ks[:-1] == ks[1:]
    assert np.all(order[:-1][tie] < order[1:][tie]), (what, "a tie not broken by index")
    strag = R.stragglers(*R.split(rays))
    n_keyed = n - int(strag.sum())
    assert not strag[order[:n_keyed]].any() and np.array_equal(order[n_keyed:], np.flatnonzero(strag)), (what, "stragglers not last in index order")
    assert np.all(key[strag] == np.uint64(R.STRAGGLER_KEY)) and np.all(key[~strag] < np.uint64(1 << (3 * ob + 3 + 2 * db))), what
    return key, order


def against_the_loop(rays, what):
    for ob, db in K.BITS:
        for layout in R.LAYOUTS:
            key, order = check_order(rays, ob, db, layout, (what, ob, db, layout))
            assert key.tolist() == R.loop_keys(rays, ob, db, layout), (what, ob, db, layout, "keys")
            assert order.tolist() == R.loop_order(rays, ob, db, layout), (what, ob, db, layout, "order")


@pytest.mark.parametrize("n", K.SIZES)
def test_numpy_form_equals_the_loop(n):
    against_the_loop(K.random_rays(n, 100 + n), n)


@pytest.mark.parametrize("kind", K.HOSTILE)
def test_hostile_sets(kind):
    rays = K.hostile(kind, 4099)
    against_the_loop(rays, kind)
    o, d = R.split(rays)
    strag = R.stragglers(o, d)
    if kind == "all_stragglers":
        assert strag.all()
        for layout in R.LAYOUTS:
            assert R.order(rays, 10, 4, layout).tolist() == list(range(len(rays)))
    elif kind in ("tied_directions", "subnormal_directions", "equal_origins"):
        assert not strag.any() or kind == "subnormal_directions"          # (a subnormal draw of three zeros is a straggler)
    else:
        assert strag.any() and not strag.all()
    if kind == "non_finite":
        bad = ~np.isfinite(o).all(axis=1) | ~np.isfinite(d).all(axis=1)
        assert np.array_equal(strag, bad)
        for what in (np.isnan, np.isposinf, np.isneginf):
            assert what(o).any() and what(d).any()
    if kind == "limit_origins":
        assert np.array_equal(strag, (np.abs(o) > 1e300).any(axis=1)) and (np.abs(o) == 1e300).any(axis=1)[~strag].any()
    if kind == "zero_directions":
        assert np.array_equal(strag, (d == 0.0).all(axis=1)) and ((d == 0.0).sum(axis=1) == 2)[~strag].any()
    if kind == "equal_origins":
        assert not R.words(rays, 16, 6)[1].any()                          # e = 0: every origin word is 0


def test_first_axis_wins_a_tie():
    """Two equal largest components: the face is the first of them; the other one's cell is the last (r = +1) or the first (r = -1)."""
    d = np.array([[2.0, 2.0, 1.0], [2.0, -2.0, 1.0], [-2.0, 1.0, 2.0], [1.0, 3.0, -3.0], [1.0, -3.0, 3.0], [-4.0, 4.0, -4.0], [0.0, 0.0, -0.5]])
    rays = (np.zeros_like(d), d)
    strag, O, face, uv = R.words(rays, 4, 3)
    assert not strag.any() and face.tolist() == [0, 0, 1, 2, 3, 1, 5]
    cell = lambda r: int(min((r + 1.0) * 4.0, 7.0))
    spread = lambda k, which: sum(((k >> b) & 1) << (2 * b + which) for b in range(3))
    want = [spread(cell(1.0), 1) | spread(cell(0.5), 0), spread(cell(-1.0), 1) | spread(cell(0.5), 0), spread(cell(0.5), 1) | spread(cell(1.0), 0),
            spread(cell(-1.0), 1) | spread(cell(1 / 3), 0), spread(cell(1.0), 1) | spread(cell(1 / 3), 0), spread(cell(1.0), 1) | spread(cell(-1.0), 0),
            spread(cell(0.0), 1) | spread(cell(0.0), 0)]
    assert uv.tolist() == want


def test_a_pinhole_cameras_rays_have_no_origin_word():
    rays = K.pinhole(4099, 3)
    strag, O, face, uv = R.words(rays, 16, 6)
    assert not strag.any() and not O.any() and len(np.unique(uv)) > 100
    for layout in R.LAYOUTS:                                              # ... so every layout sorts them by direction alone
        assert np.array_equal(R.order(rays, 16, 6, layout), np.argsort((face << np.uint64(12)) | uv, kind="stable"))


def test_bit_63_is_clear_on_every_keyed_ray_at_the_widest_key():
    for rays in (K.random_rays(4099, 5), K.hostile("limit_origins", 4099), K.hostile("tied_directions", 4099)):
        strag = R.stragglers(*R.split(rays))
        for layout in R.LAYOUTS:
            key = R.keys(rays, 16, 6, layout)
            assert not (key[~strag] >> np.uint64(63)).any() and (key[~strag] >> np.uint64(60)).any()
            assert np.all(key[strag] == np.uint64(1 << 63))


def test_the_words_fill_their_ranges():
    """Random rays reach the first and the last cell of every axis, all six faces, and every layout orders them differently."""
    rays = K.random_rays(4099, 6)
    strag, O, face, uv = R.words(rays, 10, 4)
    assert sorted(np.unique(face).tolist()) == [0, 1, 2, 3, 4, 5] and int(uv.max()) == 255 and int(uv.min()) == 0
    assert int(O.max()) >> 27 == 7 and len({R.order(rays, 10, 4, layout).tobytes() for layout in R.LAYOUTS}) == 3
    assert R.order(rays, 0, 0, R.ORIGIN_FIRST).tolist() == np.argsort(face, kind="stable").tolist()
