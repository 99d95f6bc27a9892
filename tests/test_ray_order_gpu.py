"""The ray ordering on the GPU. rt_ray_order / rt_ray_order_device against the numpy restatement (tests/ray_order_ref.py) byte for
byte; rt_intersect_ordered_device against rt_intersect_device on the same rays, every byte of every record and the counters;
order lists that are no permutations; torch buffers on a caller's stream; beside an asynchronous render; the refusals that
need real buffers."""
import ctypes as C

import numpy as np
import pytest

import ray_order_cases as K
import ray_order_ref as R
from gpu_first import torch_first  # noqa: F401
from query_ref import bounce_rays, camera_rays, mixed_rays, randomise_windows
from query_scenes import every_kind_scene
from raytracer_2022_amd import _ffi as F

pytestmark = pytest.mark.gpu

SIZES = K.SIZES + (100000,)
FILL = 0xA5
M = 4099                                                   # the query batches: a prime, 65 waves
REDUCE_THREADS = 1024 * 256                                # order_box_partial's grid at the most (kOrderReduceBlocks blocks of 256)
MID_BITS = (10, 4)


@pytest.fixture(scope="module")
def workspace(rt):
    """One ordering workspace for the largest size of the module, reused by every device-form call."""
    import torch
    ws = torch.empty(rt.ray_order_workspace_bytes(REDUCE_THREADS + 1 + 257), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    return ws


def to_device(a, pad=0, shift=0, fill=0):
    """The bytes of a numpy array in a torch buffer with `pad` spare bytes, starting `shift` bytes in."""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.full((raw.size + pad,), fill, dtype=torch.uint8, device="cuda")
    buf[shift:shift + raw.size] = torch.from_numpy(raw.copy()).cuda()
    return buf


def device_order(rt, rays, p, ws, ws_bytes=None, stream=None, shift_rays=0, shift_order=0):
    """rt_ray_order_device on torch buffers → (rc, the whole order buffer as bytes: n entries and 16 spare bytes, FILL before)."""
    import torch
    n = len(rays)
    d_rays = to_device(rays, pad=16, shift=shift_rays)
    d_order = torch.full((n * 4 + 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = F.lib().rt_ray_order_device(d_rays.data_ptr() + shift_rays, n, C.byref(p), d_order.data_ptr() + shift_order, ws.data_ptr(),
                                     ws.numel() if ws_bytes is None else ws_bytes, stream)
    torch.cuda.synchronize()
    return rc, d_order.cpu().numpy()


def both_forms(rt, rays, ws, what, bits=(MID_BITS,), layouts=R.LAYOUTS):
    n = len(rays)
    for ob, db in bits:
        for layout in layouts:
            want = R.order(rays, ob, db, layout)
            for records in (rays, K.as_radiance(rays)):                   # strides 80 and 64
                p = rt.ray_order_params(ob, db, layout, records.dtype.itemsize)
                tag = (what, ob, db, layout, p.ray_stride)
                assert rt.ray_order(records, p).tobytes() == want.tobytes(), (tag, "host form")
                rc, raw = device_order(rt, records, p, ws)
                assert rc == F.RT_OK, (tag, F.lib().rt_last_error())
                assert raw[:n * 4].tobytes() == want.tobytes(), (tag, "device form")
                assert np.all(raw[n * 4:] == FILL), (tag, "wrote past the entries")


@pytest.mark.parametrize("n", SIZES)
def test_order_equals_the_restatement(rt, workspace, n):
    both_forms(rt, K.random_rays(n, 100 + n), workspace, n, bits=K.BITS if n in (65, 4099) else (MID_BITS,))


@pytest.mark.parametrize("kind", K.HOSTILE)
def test_hostile_sets(rt, workspace, kind):
    both_forms(rt, K.hostile(kind, 4099), workspace, kind, bits=((16, 6), MID_BITS))


def test_pinhole_rays_and_the_python_defaults(rt, workspace):
    rays = K.pinhole(4099, 3)
    both_forms(rt, rays, workspace, "pinhole")
    want = default_order(rt, rays)
    assert np.array_equal(rt.ray_order(rays), want)
    assert np.array_equal(rt.ray_order(K.as_radiance(rays)), want)                          # the stride is the records' size
    assert np.array_equal(rt.ray_order(K.as_radiance(rays).view(np.uint8), stride=64), want)
    assert rt.ray_order(rays[:0]).shape == (0,)


def test_box_reduction_beyond_one_grid(rt, workspace):
    """order_box_partial's grid-stride loop (pt_order.hip): its grid is capped at kOrderReduceBlocks = 1024 blocks of 256, so a
    thread reads a second ray from n = 262 145 on. n = 262 145 + 257: the last origin, which only a second trip reads, is moved
    out to +1000 on every axis — the upper corner of the origin box, and with it every origin word, depends on it alone."""
    n = REDUCE_THREADS + 1 + 257
    rays = K.random_rays(n, 77)
    rays["origin"][n - 1] = 1000.0
    ob, db = MID_BITS
    want = R.order(rays, ob, db, R.ORIGIN_FIRST)
    o, d = R.split(rays)
    assert R.origin_box(o, R.stragglers(o, d))[1].tolist() == [1000.0] * 3
    without = R.words(rays[:n - 1], ob, db)[1]
    assert (R.words(rays, ob, db)[1][:n - 1] != without).mean() > 0.99                        # (the keys do depend on it)
    p = rt.ray_order_params(ob, db, R.ORIGIN_FIRST, 80)
    rc, raw = device_order(rt, rays, p, workspace)
    assert rc == F.RT_OK, F.lib().rt_last_error()
    assert raw[:n * 4].tobytes() == want.tobytes() and np.all(raw[n * 4:] == FILL)
    rays["direction"][n - 1] = 0.0                                                            # a straggler sets no box
    rc, raw = device_order(rt, rays, p, workspace)
    assert rc == F.RT_OK and raw[:n * 4].tobytes() == R.order(rays, ob, db, R.ORIGIN_FIRST).tobytes()


def test_workspace_and_alignment_refusals_on_real_buffers(rt, workspace):
    rays = K.random_rays(257, 12)
    p = rt.ray_order_params()
    need = rt.ray_order_workspace_bytes(257)
    for kw in ({"ws_bytes": need - 1}, {"shift_rays": 8}, {"shift_order": 2}):
        rc, raw = device_order(rt, rays, p, workspace, **kw)
        assert rc == F.RT_ERR_INVALID and np.all(raw == FILL), kw
    rc, raw = device_order(rt, rays, p, workspace, ws_bytes=need)                 # exactly enough, inside a larger buffer
    assert rc == F.RT_OK and raw[:257 * 4].tobytes() == default_order(rt, rays).tobytes()
    rc, raw = device_order(rt, rays, p, workspace, shift_order=4)                 # 4-byte alignment is all an order needs
    assert rc == F.RT_OK and raw[4:4 + 257 * 4].tobytes() == default_order(rt, rays).tobytes() and np.all(raw[:4] == FILL)


# ---- queries in a given order ----------------------------------------------------------------------------------------------------
def hostile_query_rays(rt):
    """The hostile rays of tests/test_query.py::test_hostile_rays."""
    rays = []
    for o in [(0, 1, 8), (0.0, 0.5, 0.0), (4.5, 0.5, 2.0), (-4, 1, 2), (0, 0, 0)]:
        for dvec in [(0, 0, -1), (0, -1, 0), (1, 0, 0), (0, 0, 1), (0, 0, 0), (1e-300, 0, -1), (-0.0, -1, 0),
                     (np.nan, 0, -1), (0, np.nan, 0), (np.inf, 0, 0), (1, 1, 1)]:
            for t_min, t_max in [(0.001, np.inf), (5.0, 5.0), (5.0, 1.0), (-np.inf, np.inf), (np.nan, np.inf), (0.001, np.nan),
                                 (0.0, 3.0)]:
                rays.append((o, dvec, t_min, t_max))
    rays += [((np.nan, 0, 0), (0, 0, -1), 0.001, np.inf), ((0, np.inf, 0), (0, -1, 0), 0.001, np.inf)]
    return np.concatenate([rt.query_rays(o, dv, time=0.3, t_min=a, t_max=b, rng_state=i) for i, (o, dv, a, b) in enumerate(rays)])


class Case:
    """A scene on the device, M mixed camera, random and bounce rays in random order with random windows, times and RNG states,
    and what rt_intersect_device makes of them: the reference, computed once."""

    def __init__(self, rt, name):
        import torch
        if name in ("every_kind", "hostile"):
            self.keep, self.desc, cam = every_kind_scene(rt)
        elif name == "every_kind_no_medium":
            self.keep, self.desc, cam = every_kind_scene(rt, with_medium=False)
        else:
            self.keep = rt.HostScene(name, seed=2022)
            self.desc, cam = self.keep.desc, self.keep.default_view(1.5)[0]
        self.cam = cam
        self.dev = rt.DeviceScene(self.desc)
        first, g = mixed_rays(rt, self.desc, cam, 3 * 1600, seed=len(name))
        rays = np.concatenate([first, bounce_rays(rt, self.dev.intersect(first), g, 1600)])
        if len(rays) < M:
            rays = np.concatenate([rays, camera_rays(rt, cam, M - len(rays), g)])
        rays = randomise_windows(rays, g)
        rays = rays[g.permutation(len(rays))[:M]]
        if name == "hostile":
            h = hostile_query_rays(rt)
            rays[g.permutation(M)[:len(h)]] = h
        self.rays = np.ascontiguousarray(rays)
        self.d_rays = to_device(self.rays)
        self.ws = torch.empty(rt.intersect_ordered_workspace_bytes(M), dtype=torch.uint8, device="cuda")
        self.plain = {}

    def reference(self, any_hit=False):
        """(the bytes rt_intersect_device leaves in a buffer of FILL, its RT_FLAG_COUNTERS stats)"""
        import torch
        if any_hit not in self.plain:
            d_hits = torch.full((M * 96 + 16,), FILL, dtype=torch.uint8, device="cuda")
            st = F.rt_stats()
            self.dev.intersect_device(self.d_rays.data_ptr(), M, d_hits.data_ptr(), any_hit=any_hit, stats=st)
            torch.cuda.synchronize()
            self.plain[any_hit] = (d_hits.cpu().numpy(), st)
        return self.plain[any_hit]


CASES = {}


def case_of(rt, name):
    if name not in CASES:
        CASES[name] = Case(rt, name)
    return CASES[name]


def ordered(dev, d_rays, order, n, ws, any_hit=False, want_stats=True, stream=None):
    """rt_intersect_ordered_device under `order` (a numpy array, or a device buffer) into a buffer of FILL → (its bytes, 16 spare
    ones included, the stats)."""
    import torch
    d_order = to_device(np.asarray(order, dtype=np.uint32)) if isinstance(order, np.ndarray) else order
    d_hits = torch.full((n * 96 + 16,), FILL, dtype=torch.uint8, device="cuda")
    st = F.rt_stats() if want_stats else None
    torch.cuda.synchronize()
    dev.intersect_ordered_device(d_rays.data_ptr(), d_order.data_ptr(), n, d_hits.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr=stream,
                                 any_hit=any_hit, stats=st)
    torch.cuda.synchronize()
    return d_hits.cpu().numpy(), st


def default_order(rt, rays):
    """The restatement under RAY_ORDER_DEFAULTS, what rt.ray_order_params() asks for."""
    d = rt.RAY_ORDER_DEFAULTS
    return R.order(rays, d["origin_bits"], d["dir_bits"], d["layout"])


def traversal(st):
    return st.node_visits, list(st.prim_tests), st.rng_draws


ORDERS = ("computed", "random", "identity")
FINE = MID_BITS + (R.ORIGIN_FIRST,)                    # the key the query tests order by: fine enough that few rays share one


def fine_params(rt):
    return rt.ray_order_params(*FINE)


def order_of(rt, c, which, workspace):
    if which == "computed":
        rc, raw = device_order(rt, c.rays, fine_params(rt), workspace)
        assert rc == F.RT_OK
        order = raw[:M * 4].view(np.uint32).copy()
        assert np.array_equal(order, R.order(c.rays, *FINE)) and len(np.unique(R.keys(c.rays, *FINE))) > M // 4
        return order
    if which == "random":
        return np.random.default_rng(5).permutation(M).astype(np.uint32)
    return np.arange(M, dtype=np.uint32)


@pytest.mark.parametrize("which", ORDERS)
@pytest.mark.parametrize("name", ["random_scene", "cornell_smoke", "every_kind", "hostile"])
def test_hits_are_rt_intersect_devices_byte_for_byte(rt, workspace, name, which):
    c = case_of(rt, name)
    want, st_want = c.reference()
    hits = want[:M * 96].view(F.HIT_DTYPE)
    assert hits["hit"].sum() > 100 and (hits["hit"] == 0).sum() > 0              # (what the batch shows, on the reference)
    if name == "cornell_smoke":
        assert hits["rng_draws"].sum() > 0 and len(np.unique(c.rays["rng_state"])) == M
    if name == "hostile":
        assert np.isnan(hits["t"][hits["hit"] == 1]).any()
    order = order_of(rt, c, which, workspace)
    got, st = ordered(c.dev, c.d_rays, order, M, c.ws)
    assert got.tobytes() == want.tobytes(), (name, which)                           # every field, the padding, the spare bytes
    assert st.rays == st_want.rays == M and traversal(st) == traversal(st_want) and st.ms > 0
    assert st.paths == 0 and st.passes == 0 and st.pool_slots == 0 and st.partial_bytes == 0
    plain, none = ordered(c.dev, c.d_rays, order, M, c.ws, want_stats=False)       # the plain kernel instance, no synchronisation
    assert none is None and plain.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["random_scene", "every_kind_no_medium"])
def test_any_hit_in_a_given_order(rt, workspace, name):
    c = case_of(rt, name)
    assert c.desc.n_media == 0
    want, st_want = c.reference(any_hit=True)
    closest = c.reference()[0][:M * 96].view(F.HIT_DTYPE)
    assert np.array_equal(want[:M * 96].view(F.HIT_DTYPE)["hit"], closest["hit"])
    assert name != "random_scene" or want.tobytes() != c.reference()[0].tobytes()         # (the first accepted is not always the closest)
    for which in ORDERS:
        got, st = ordered(c.dev, c.d_rays, order_of(rt, c, which, workspace), M, c.ws, any_hit=True)
        assert got.tobytes() == want.tobytes(), (name, which)
        assert st.rays == M and traversal(st) == traversal(st_want)
    smoke = case_of(rt, "cornell_smoke")
    with pytest.raises(rt.RtError) as e:
        ordered(smoke.dev, smoke.d_rays, np.arange(M, dtype=np.uint32), M, smoke.ws, any_hit=True)
    assert e.value.code == F.RT_ERR_UNSUPPORTED and "ConstantMedium" in str(e.value)


@pytest.mark.parametrize("n", (1, 65))
def test_small_batches(rt, workspace, n):
    c = case_of(rt, "random_scene")
    want = c.reference()[0]
    rc, raw = device_order(rt, c.rays[:n], fine_params(rt), workspace)
    assert rc == F.RT_OK
    got, st = ordered(c.dev, c.d_rays, raw[:n * 4].view(np.uint32).copy(), n, c.ws)
    assert got[:n * 96].tobytes() == want[:n * 96].tobytes() and np.all(got[n * 96:] == FILL) and st.rays == n
    st.rays = 77
    c.dev.intersect_ordered_device(0, 0, 0, 0, 0, 0, stats=st)                       # n = 0: RT_OK, the stats zeroed, no launch
    assert st.rays == 0


def test_a_batch_beyond_the_persistent_grid(rt):
    """More rays than the query kernel's grid has lanes (at most 2048 a CU), as in tests/test_beyond_one_grid.py: K random
    permutations of the M-ray base, n = K M > 2 L. The order is computed on the device over all n rays; every record must be the
    base ray's, and the counters K times the base's."""
    import torch
    c = case_of(rt, "random_scene")
    want, st_want = c.reference()
    base = want[:M * 96].reshape(M, 96)
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 2048
    k = (2 * lanes + 1 + M - 1) // M
    g = np.random.default_rng(k)
    idx = np.concatenate([g.permutation(M) for _ in range(k)])
    n = k * M
    assert n > 2 * lanes
    d_rays = to_device(c.rays[idx])
    d_order = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ws_order = torch.empty(rt.ray_order_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    ws = torch.empty(rt.intersect_ordered_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    rt.ray_order_device(d_rays.data_ptr(), n, fine_params(rt), d_order.data_ptr(), ws_order.data_ptr(), ws_order.numel())
    got, st = ordered(c.dev, d_rays, d_order, n, ws)
    order = d_order.cpu().numpy().view(np.uint32)
    assert np.array_equal(np.sort(order), np.arange(n))
    assert np.array_equal(order, R.order(c.rays[idx], *FINE))
    assert np.array_equal(got[:n * 96].reshape(n, 96), base[idx]) and np.all(got[n * 96:] == FILL)
    nodes, prims, draws = traversal(st_want)
    assert st.rays == n and traversal(st) == (k * nodes, [k * x for x in prims], k * draws)


def test_order_lists_that_are_no_permutations(rt):
    """Entries >= n (0xFFFFFFFF among them) do nothing, repeats compute a ray twice, and a ray that no entry names keeps its bytes."""
    c = case_of(rt, "every_kind")
    want, _ = c.reference()
    base = want[:M * 96].reshape(M, 96)
    g = np.random.default_rng(8)
    order = g.integers(0, M, M).astype(np.uint32)                                   # with repeats: about a third of the rays unnamed
    beyond = g.permutation(M)[:500]
    order[beyond] = np.concatenate([[M, M + 1, 0xFFFFFFFF, 0x80000000, 1 << 20], g.integers(M, 1 << 32, 495)]).astype(np.uint32)
    valid = order < M
    named = np.zeros(M, dtype=bool)
    named[order[valid]] = True
    assert 0 < named.sum() < M and valid.sum() == M - 500 and len(np.unique(order[valid])) < valid.sum()
    got, st = ordered(c.dev, c.d_rays, order, M, c.ws)
    rec = got[:M * 96].reshape(M, 96)
    assert np.array_equal(rec[named], base[named])
    assert np.all(rec[~named] == FILL) and np.all(got[M * 96:] == FILL)
    assert st.rays == valid.sum()
    got, st = ordered(c.dev, c.d_rays, np.full(M, 0xFFFFFFFF, dtype=np.uint32), M, c.ws)      # nothing named at all
    assert np.all(got == FILL) and st.rays == 0


def test_torch_buffers_on_a_callers_stream(rt):
    """Upload, ordering, ordered query and a dependent copy all on one side stream, with stats == NULL: no synchronisation
    between them but the stream's order."""
    import torch
    c = case_of(rt, "random_scene")
    want = c.reference()[0]
    stream = torch.cuda.Stream()
    h_rays = torch.from_numpy(c.rays.view(np.uint8).copy()).pin_memory()
    p = fine_params(rt)
    with torch.cuda.stream(stream):
        d_rays = h_rays.to("cuda", non_blocking=True)
        d_order = torch.empty(M, dtype=torch.int32, device="cuda")
        d_hits = torch.full((M * 96,), FILL, dtype=torch.uint8, device="cuda")
        ws_order = torch.empty(rt.ray_order_workspace_bytes(M), dtype=torch.uint8, device="cuda")
        ws = torch.empty(rt.intersect_ordered_workspace_bytes(M), dtype=torch.uint8, device="cuda")
        rt.ray_order_device(d_rays.data_ptr(), M, p, d_order.data_ptr(), ws_order.data_ptr(), ws_order.numel(), stream_ptr=stream.cuda_stream)
        c.dev.intersect_ordered_device(d_rays.data_ptr(), d_order.data_ptr(), M, d_hits.data_ptr(), ws.data_ptr(), ws.numel(),
                                       stream_ptr=stream.cuda_stream)
        behind = torch.empty_like(d_hits)
        behind.copy_(d_hits, non_blocking=True)
        order_behind = d_order.clone()
    stream.synchronize()
    assert behind.cpu().numpy().tobytes() == want[:M * 96].tobytes()
    assert order_behind.cpu().numpy().view(np.uint32).tobytes() == R.order(c.rays, p.origin_bits, p.dir_bits, p.layout).tobytes()


def test_ordered_queries_beside_an_asynchronous_render(rt):
    """As tests/test_query.py does for rt_intersect_device: an RT_FLAG_ASYNC render on one stream, orderings and ordered queries
    of the same scene on another; both keep their serial results bit for bit."""
    import torch
    s = rt.HostScene("final_scene", seed=2022)
    W, H, spp = 64, 48, 4
    cam, bg = s.default_view(W / H)
    rows = rt.shuffled_rows(H, 3)
    p = rt.make_params(W, H, spp, 50, bg, seed=2022, spp_chunk=1)
    dev = rt.DeviceScene(s.desc)
    ref_render = dev.render(cam, p, rows)
    g = np.random.default_rng(9)
    n = 30_000
    batches = [camera_rays(rt, cam, n, g) for _ in range(3)]
    for b_ in batches:
        b_["rng_state"] = g.integers(0, 2**63, n, dtype=np.uint64)
        b_[:] = b_[g.permutation(n)]
    serial = [dev.intersect(b_) for b_ in batches]
    a_stream, b_stream = torch.cuda.Stream(), torch.cuda.Stream()
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    out = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda")
    d_rays = [to_device(b_) for b_ in batches]
    d_hits = [torch.zeros(n * 96, dtype=torch.uint8, device="cuda") for _ in batches]
    d_order = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in batches]
    ws_order = torch.empty(rt.ray_order_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    ws = torch.empty(rt.intersect_ordered_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    op = fine_params(rt)
    torch.cuda.synchronize()
    dev.render_device(cam, p, d_rows.data_ptr(), H, out.data_ptr(), a_stream.cuda_stream, None, asynchronous=True)
    for r_, o_, h_ in zip(d_rays, d_order, d_hits):                                # (one workspace of each kind, reused in stream order)
        rt.ray_order_device(r_.data_ptr(), n, op, o_.data_ptr(), ws_order.data_ptr(), ws_order.numel(), stream_ptr=b_stream.cuda_stream)
        dev.intersect_ordered_device(r_.data_ptr(), o_.data_ptr(), n, h_.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr=b_stream.cuda_stream)
    b_stream.synchronize()
    dev.wait(a_stream.cuda_stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), ref_render.view(np.uint64))
    for h_, o_, b_, want in zip(d_hits, d_order, batches, serial):
        assert np.array_equal(h_.cpu().numpy(), want.view(np.uint8))
        assert o_.cpu().numpy().view(np.uint32).tobytes() == R.order(b_, op.origin_bits, op.dir_bits, op.layout).tobytes()


def test_refused_alignments_and_short_workspaces_leave_the_hits_untouched(rt):
    import torch
    c = case_of(rt, "random_scene")
    n = 257
    need = rt.intersect_ordered_workspace_bytes(n)
    d_order = to_device(np.arange(n, dtype=np.uint32), pad=16, shift=4)
    d_rays = to_device(c.rays[:n], pad=16, shift=8)
    d_hits = torch.full((n * 96 + 16,), FILL, dtype=torch.uint8, device="cuda")
    L = rt.lib()
    good = dict(rays=c.d_rays.data_ptr(), order=d_order.data_ptr() + 4, hits=d_hits.data_ptr(), ws=c.ws.data_ptr(), ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return L.rt_intersect_ordered_device(c.dev._h, a["rays"], a["order"], n, 0, a["hits"], a["ws"], a["ws_bytes"], None, None)
    for kw in ({"ws_bytes": need - 1}, {"ws": c.ws.data_ptr() + 8}, {"rays": d_rays.data_ptr() + 8}, {"hits": d_hits.data_ptr() + 8},
               {"order": d_order.data_ptr() + 6}, {"ws": None}, {"order": None}):
        assert call(**kw) == F.RT_ERR_INVALID and L.rt_last_error().startswith(b"rt_intersect_ordered_device"), kw
        torch.cuda.synchronize()
        assert np.all(d_hits.cpu().numpy() == FILL), kw
    assert call() == F.RT_OK                                                        # exactly enough workspace, an order at 4 mod 16
    torch.cuda.synchronize()
    assert d_hits.cpu().numpy()[:n * 96].tobytes() == c.reference()[0][:n * 96].tobytes()


def test_python_forms(rt):
    """DeviceScene.intersect(order=...): None as ever, "auto" through rt_intersect_ordered with the defaults, an index array."""
    c = case_of(rt, "cornell_smoke")
    want, st_want = c.dev.intersect(c.rays, want_stats=True)
    got, st = c.dev.intersect(c.rays, want_stats=True, order="auto")
    assert got.tobytes() == want.tobytes() and st.rays == M and traversal(st) == traversal(st_want)
    p = rt.ray_order_params(16, 6, F.RT_ORDER_FACE_ORIGIN_UV)
    assert c.dev.intersect(c.rays, order="auto", order_params=p).tobytes() == want.tobytes()
    assert c.dev.intersect(c.rays, order=rt.ray_order(c.rays, p)).tobytes() == want.tobytes()
    half = np.arange(0, M, 2)
    got = c.dev.intersect(c.rays, order=np.concatenate([half, half[:M - len(half)]]))        # a host form: unnamed rays keep zeros
    assert got[half].tobytes() == want[half].tobytes() and not np.ascontiguousarray(got[1::2]).view(np.uint8).any()
    assert c.dev.intersect(c.rays[:0], order="auto").shape == (0,) and c.dev.intersect(c.rays[:0], order=np.zeros(0)).shape == (0,)
    with pytest.raises(ValueError):
        c.dev.intersect(c.rays, order="sorted")
    with pytest.raises(ValueError):
        c.dev.intersect(c.rays, order=np.arange(5))
