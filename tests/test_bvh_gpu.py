"""The device BVH builder (rt_bvh_build / rt_bvh_build_device) on the GPU: the node array against the numpy restatement
(tests/bvh_ref.py) bit for bit, the refusals that only the device can decide, torch buffers on a caller's stream, and whole
scenes whose root tree it built — accepted by rt_scene_create, queried and rendered against the CPU oracle on the same
description bit for bit, and held to the BVH-free reference (tests/brute_hits.py) under tests/test_brute_hits_gpu.py's acceptance."""
import ctypes as C

import numpy as np
import pytest

import brute_hits as B
import brute_scenes as S
import bvh_cases as K
import bvh_ref as R
import bvh_scenes as BS
from compare import same_bits
from gpu_first import torch_first  # noqa: F401
from query_ref import oracle_hits
from raytracer_2022_amd import _ffi as F

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 63, 64, 65, 257, 4099, 100000)
BASE = 1000                                              # the device form's node_base
FILL = 0xA5


@pytest.fixture(scope="module")
def workspace(rt):
    """One workspace for the largest size, reused by every device-form build of the module."""
    import torch
    n = rt.bvh_workspace_bytes(max(SIZES))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    return ws


def device_form(rt, refs, boxes, base, ws, ws_bytes=None, stream=None, shift_out=0, shift_boxes=0):
    """rt_bvh_build_device on torch buffers → (rc, the node buffer's bytes, the whole output buffer filled with FILL before)."""
    import torch
    n = len(refs)
    d_refs = torch.from_numpy(np.ascontiguousarray(refs).view(np.uint8).copy()).cuda()
    d_boxes = torch.zeros(boxes.size * 8 + 16, dtype=torch.uint8, device="cuda")
    d_boxes[shift_boxes:shift_boxes + boxes.size * 8] = torch.from_numpy(np.ascontiguousarray(boxes).view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.full((max(1, n - 1) * 64 + 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = F.lib().rt_bvh_build_device(d_refs.data_ptr(), d_boxes.data_ptr() + shift_boxes, n, base, d_out.data_ptr() + shift_out, ws.data_ptr(),
                                     ws.numel() if ws_bytes is None else ws_bytes, stream)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy()


def both_forms(rt, refs, boxes, ws, what):
    want0 = R.build(refs, boxes)
    got0 = rt.bvh_build(refs, boxes)
    assert got0.tobytes() == want0.tobytes(), (what, "host form")
    rc, raw = device_form(rt, refs, boxes, BASE, ws)
    assert rc == F.RT_OK, (what, F.lib().rt_last_error())
    n_bytes = len(want0) * 64
    assert raw[:n_bytes].tobytes() == R.build(refs, boxes, node_base=BASE).tobytes(), (what, "device form")
    assert np.all(raw[n_bytes:] == FILL), (what, "wrote past the records")
    return got0


@pytest.mark.parametrize("n", SIZES)
def test_node_array_equals_the_restatement(rt, workspace, n):
    refs, boxes = K.random_boxes(n, 500 + n)
    nodes = both_forms(rt, refs, boxes, workspace, n)
    if n <= 4099:
        R.check_tree(nodes, refs, boxes)


@pytest.mark.parametrize("kind", K.HOSTILE)
def test_hostile_sets(rt, workspace, kind):
    refs, boxes = K.hostile(kind, 4099)
    nodes = both_forms(rt, refs, boxes, workspace, kind)
    R.check_tree(nodes, refs, boxes)


def test_need_of_a_deep_chain_with_and_without_the_swap(rt, workspace):
    refs, boxes = K.chain()
    nodes = both_forms(rt, refs, boxes, workspace, "chain")
    need = R.check_tree(nodes, refs, boxes)
    without = R.build(refs, boxes, swap=False, want_need=True)[1]
    print("chain of %d: need %d on the device, %d for the restatement without the swap" % (len(refs), need, without))
    assert need <= 13 < without


BAD_BOXES = {"nan": (5, 1, np.nan), "inf": (17, 4, np.inf), "minus_inf": (3, 0, -np.inf), "beyond_1e300": (40, 5, 1e301),
             "minus_beyond_1e300": (41, 2, -1e301), "min_above_max": (63, 0, None)}


@pytest.mark.parametrize("what", list(BAD_BOXES))
@pytest.mark.parametrize("n", (1, 65, 4099))
def test_bad_boxes_are_refused_with_the_output_untouched(rt, workspace, what, n):
    refs, boxes = K.random_boxes(n, 9)
    i, k, v = BAD_BOXES[what]
    i %= n
    boxes[i, k] = boxes[i, 3 + k] + 1.0 if v is None else v
    out = np.zeros(max(1, n - 1), dtype=F.BVH_NODE_DTYPE)
    out.view(np.uint8)[:] = FILL
    assert F.lib().rt_bvh_build(refs.ctypes.data, boxes.ctypes.data, n, 0, out.ctypes.data) == F.RT_ERR_INVALID
    assert b"leaf box" in F.lib().rt_last_error() and np.all(out.view(np.uint8) == FILL)
    rc, raw = device_form(rt, refs, boxes, BASE, workspace)
    assert rc == F.RT_ERR_INVALID and b"leaf box" in F.lib().rt_last_error()
    assert np.all(raw == FILL)


def test_box_reduction_beyond_one_grid(rt):
    """bvh_box_partial's grid-stride loop (pt_bvh.hip): its grid is capped at kBvhReduceBlocks = 1024 blocks of 256, so a thread
    takes a second box from n = 262 145 on. n = 262 144 + 257: the last box, which only a second trip reads, is moved out to
    +-1000 — the scene box, and with it every Morton key and the whole tree, depends on it. Then the same set with a NaN in
    that box: refused, the output untouched."""
    import torch
    n = 1024 * 256 + 257
    refs, boxes = K.random_boxes(n, 77)
    boxes[n - 1, :3], boxes[n - 1, 3:] = -1000.0, 1000.0
    ws = torch.empty(rt.bvh_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    want = R.build(refs, boxes, node_base=BASE)
    assert want["bmin"][0].tolist() == [-1000.0] * 3 and want["bmax"][0].tolist() == [1000.0] * 3       # (the root's box is the scene's)
    rc, raw = device_form(rt, refs, boxes, BASE, ws)
    assert rc == F.RT_OK, F.lib().rt_last_error()
    n_bytes = len(want) * 64
    assert raw[:n_bytes].tobytes() == want.tobytes(), "device form"
    assert np.all(raw[n_bytes:] == FILL), "wrote past the records"
    boxes[n - 1, 4] = np.nan
    rc, raw = device_form(rt, refs, boxes, BASE, ws)
    assert rc == F.RT_ERR_INVALID and b"leaf box" in F.lib().rt_last_error()
    assert np.all(raw == FILL)


def test_limit_coordinates_are_accepted(rt, workspace):
    refs, boxes = K.random_boxes(65, 10)
    boxes[7, :3], boxes[7, 3:] = -1e300, 1e300
    both_forms(rt, refs, boxes, workspace, "1e300")


def test_workspace_and_alignment_refusals_on_real_buffers(rt, workspace):
    refs, boxes = K.random_boxes(257, 12)
    need = rt.bvh_workspace_bytes(257)
    for kw in ({"ws_bytes": need - 1}, {"shift_out": 8}, {"shift_boxes": 8}):
        rc, raw = device_form(rt, refs, boxes, BASE, workspace, **kw)
        assert rc == F.RT_ERR_INVALID and np.all(raw == FILL), kw
    rc, raw = device_form(rt, refs, boxes, BASE, workspace, ws_bytes=need)           # exactly enough, inside a larger buffer
    assert rc == F.RT_OK and raw[:256 * 64].tobytes() == R.build(refs, boxes, node_base=BASE).tobytes()


def test_torch_buffers_on_a_callers_stream(rt, workspace):
    """Upload, build and a dependent copy all on one side stream, with no synchronisation between them but the build's own."""
    import torch
    refs, boxes = K.random_boxes(4099, 13)
    stream = torch.cuda.Stream()
    h_refs, h_boxes = torch.from_numpy(refs.view(np.int32).copy()).pin_memory(), torch.from_numpy(boxes.copy()).pin_memory()
    with torch.cuda.stream(stream):
        d_refs, d_boxes = h_refs.to("cuda", non_blocking=True), h_boxes.to("cuda", non_blocking=True)
        d_out = torch.zeros(4098 * 64, dtype=torch.uint8, device="cuda")
        rt.bvh_build_device(d_refs.data_ptr(), d_boxes.data_ptr(), 4099, d_out.data_ptr(), workspace.data_ptr(), workspace.numel(),
                            node_base=BASE, stream_ptr=stream.cuda_stream)
        behind = torch.empty_like(d_out)
        behind.copy_(d_out, non_blocking=True)
    stream.synchronize()
    assert behind.cpu().numpy().tobytes() == R.build(refs, boxes, node_base=BASE).tobytes()


# ---- scenes whose root tree the device built -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BS.NAMES)
def test_scene_on_a_built_tree(rt, O, name):
    d, cam, refs, boxes, base = BS.make(name)                                            # (the device builds the tree)
    nodes = rt.host.desc_nodes(d)[base:]
    assert nodes.tobytes() == R.build(refs, boxes, node_base=base).tobytes()
    dev = rt.DeviceScene(d)                                                              # rt_scene_create accepts it
    memo = {}
    need = R.walk(nodes, base, leaf_need=lambda r: BS.ref_need(d, r, memo))[2]
    deepest_leaf = max(BS.ref_need(d, int(r), memo) for r in refs)
    assert dev.info()["stack_need"] == need <= R.need_bound(len(refs)) + deepest_leaf - 1
    # queries: the oracle on the same description bit for bit, and the BVH-free reference
    sc = B.Scene(d)
    compared = 0
    for family, rays in S.families(B, sc, cam, 300 + len(name)).items():
        ans = B.solve(sc, rays["origin"], rays["direction"], rays["time"], rays["t_min"], rays["t_max"])
        assert B.classify(sc, ans)[3].sum() <= S.AMBIGUOUS_SHARE * len(rays), (name, family)
        q = np.ascontiguousarray(rays, dtype=F.QUERY_RAY_DTYPE)
        got = dev.intersect(q)
        ref, _ = oracle_hits(O, d, q)
        assert np.array_equal(got["hit"], ref["hit"]) and np.array_equal(got["rng_draws"], ref["rng_draws"]), (name, family)
        h = ref["hit"] == 1
        for f in ("t", "u", "v", "p", "normal"):
            assert same_bits(got[f][h], ref[f][h]), (name, family, f)
        assert np.array_equal(got["front_face"][h], ref["front_face"][h]) and np.array_equal(got["mat"][h], ref["mat"][h])
        assert np.all(got["prim"][~h] == F.RT_REF_NONE)
        ta, _ = B.compare(sc, rays, got["hit"], got["t"], got["rng_draws"], got["prim"], ans=ans)
        print(ta.line(name, family, "hip/lbvh"))
        assert not ta.failures, (name, family, ta.failures[:5])
        assert ta.worst <= 1.0
        compared += ta.compared
        if not B.flat_node_paths(sc).any():
            assert ta.class1 == 0
        if not any(p.zoomed for p in sc.paths):
            assert ta.class2 == 0
    assert compared >= 0.5 * S.N_RAYS
    # a small render with counters against the CPU oracle on the same description
    W = H = 32
    spp = 4
    p = rt.make_params(W, H, spp, 50, BS.BACKGROUND, seed=7)
    rows = rt.shuffled_rows(H, 7)
    want, st_want = O.render_cpu(d, cam, p, rows, n_threads=4, want_stats=True)
    out, st = dev.render(cam, p, rows, want_stats=True)
    assert st.as_dict() == st_want.as_dict(), name
    assert same_bits(out, want), name
    assert np.array_equal(rt.write_color(out, spp), O.write_color(want, spp)), name
