"""The numpy restatement of the device BVH builder (tests/bvh_ref.py) on the CPU: build() against the plain per-range loop bit
for bit, the properties every tree must have, and the restated tree under the CPU oracle against the BVH-free reference
(tests/brute_hits.py) with the acceptance tests/test_brute_hits.py applies to the same scenes' own BVHs. The device is held to
build() by tests/test_bvh_gpu.py."""
import numpy as np
import pytest

import brute_hits as B
import brute_scenes as S
import bvh_cases as K
import bvh_ref as R
import raytracer_2022_amd as rt
from raytracer_2022_amd import _ffi as F

SIZES = (1, 2, 3, 5, 64, 65, 1000)


@pytest.mark.parametrize("n", SIZES)
def test_build_equals_the_plain_loop(n):
    refs, boxes = K.random_boxes(n, 40 + n)
    for base in (0, 12345):
        got, need = R.build(refs, boxes, node_base=base, want_need=True)
        assert got.tobytes() == R.build_plain(refs, boxes, node_base=base).tobytes()
        assert R.check_tree(got, refs, boxes, base) == need
    assert R.build(refs, boxes, swap=False).tobytes() == R.build_plain(refs, boxes, swap=False).tobytes()


@pytest.mark.parametrize("kind", K.HOSTILE)
@pytest.mark.parametrize("n", (65, 257))
def test_hostile_sets(kind, n):
    refs, boxes = K.hostile(kind, n)
    got = R.build(refs, boxes, node_base=3)
    assert got.tobytes() == R.build_plain(refs, boxes, node_base=3).tobytes()
    R.check_tree(got, refs, boxes, 3)
    if kind == "flips_and_nodes":                        # refs go in as given
        leaves = R.walk(got, 3)[0]
        assert sorted(leaves) == sorted(refs.tolist()) and any(r & F.RT_REF_FLIP for r in leaves)


def test_keys_take_21_bits_an_axis_and_ties_break_by_index():
    boxes = np.array([[0, 0, 0, 0, 0, 0], [1, 2, 4, 1, 2, 4], [1, 0, 0, 1, 0, 0], [0, 2, 0, 0, 2, 0], [0, 0, 4, 0, 0, 4], [1, 2, 4, 1, 2, 4]], dtype=np.float64)
    key = R.morton_keys(boxes)
    top = 2097151
    spread = lambda k, s: sum(((k >> b) & 1) << (3 * b + s) for b in range(21))
    assert key.tolist() == [0, spread(top, 2) | spread(top, 1) | spread(top, 0), spread(top, 2), spread(top, 1), spread(top, 0), key[1]]
    assert int(key.max()) < 1 << 63
    assert R.sorted_order(key).tolist() == [0, 4, 3, 2, 1, 5]


def test_the_swap_rule_bounds_the_need_of_a_deep_chain():
    refs, boxes = K.chain()
    nodes, need = R.build(refs, boxes, want_need=True)
    assert need <= 13 and R.check_tree(nodes, refs, boxes) == need
    plain, need_plain = R.build(refs, boxes, swap=False, want_need=True)
    assert need_plain > 13 and R.walk(plain, 0)[2] == need_plain
    print("chain of %d: need %d with the swap, %d without" % (len(refs), need, need_plain))


# ---- the restated tree under the oracle ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rebuilt():
    cache = {}

    def get(name):
        if name not in cache:
            d0, cam = S.make(name)
            d = rt.rebuild_bvh(d0, float(cam.time0), float(cam.time1), build=R.build)
            cache[name] = (d0, d, cam, B.Scene(d))
        return cache[name]
    return get


@pytest.mark.parametrize("name", ["random_scene", "cornell_box", "final_scene", "wwscene"])
def test_restated_tree_under_the_oracle(O, rebuilt, name):
    d0, d, cam, sc = rebuilt(name)
    assert d.n_nodes == d0.n_nodes + max(1, len(rt.tree_leaves(d0)) - 1) and F.ref_index(d.root) == d0.n_nodes
    assert sorted(rt.tree_leaves(d).tolist()) == sorted(rt.tree_leaves(d0).tolist())
    violations, _ = B.enclosure_violations(sc, np.linspace(float(cam.time0), float(cam.time1), 5))
    assert not violations, violations[:5]
    tallies = {}
    for family, rays in S.families(B, sc, cam, S.seed_of(name)).items():
        ans = B.solve(sc, rays["origin"], rays["direction"], rays["time"], rays["t_min"], rays["t_max"])
        assert B.classify(sc, ans)[3].sum() <= S.AMBIGUOUS_SHARE * len(rays), (name, family)
        hit, t, draws, _ = S.oracle_results(O, d, rays)
        tallies[family], _ = B.compare(sc, rays, hit, t, draws, ans=ans)
        print(tallies[family].line(name, family, "oracle/lbvh"))
    assert set(tallies) == set(B.FAMILIES)
    for family, ta in tallies.items():                   # (tests/test_brute_hits.py: test_root_against_brute_force)
        assert ta.rays == S.N_RAYS // 4, (name, family)
        assert not ta.failures, (name, family, ta.failures[:5])
        assert ta.worst <= 1.0
    if not B.flat_node_paths(sc).any():
        assert sum(ta.class1 for ta in tallies.values()) == 0
    if not any(p.zoomed for p in sc.paths):
        assert sum(ta.class2 for ta in tallies.values()) == 0
    if not any(B.ref_kind(p.leaf) == B.K_RING for p in sc.paths):
        assert sum(ta.class3 for ta in tallies.values()) == 0
    assert sum(ta.compared for ta in tallies.values()) >= 0.5 * S.N_RAYS
