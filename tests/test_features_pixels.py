"""Pixel-list feature buffers (rt_features_pixels*) against rt_features and the CPU oracle, bit for bit; the feature merge and
resolve against their numpy restatement (adaptive_features_ref.py); render_adaptive(guides="all") end to end.

Record e of a list is the record rt_features writes for column px of row id frame * height + py, id = frame * (width * height)
+ py * width + px — so with every row of every frame in order, it is record `id` of rt_features' flattened output. The oracle
composition is features_ref.py's (oracle_features), asked for the same pixels. Every comparison is on the uint64 view of the
doubles (NaN where the reference has NaN)."""
import ctypes as C

import numpy as np
import pytest

import adaptive_features_ref as FR
from raytracer_2022_amd import _ffi as F

from compare import assert_same_bits
from features_ref import ASSETS, BUILDERS, all_rows, check_first_hit_counters, oracle_ids, shuffled_ids_with_repeats
from gpu_first import torch_first  # noqa: F401
from query_scenes import every_material_scene

pytestmark = pytest.mark.gpu

W0, H0, SPP0 = 24, 16, 3


# ---- 1. entry by entry against rt_features ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", BUILDERS)
def test_every_scene_builder_entry_by_entry(rt, name):
    s = rt.HostScene(name, seed=2022)
    cam, bg = s.default_view(W0 / H0)
    p = rt.make_params(W0, H0, SPP0, 50, bg, seed=2022, n_frames=2)
    dev = rt.DeviceScene(s.desc)
    rows = rt.two_frame_rows(np.arange(H0, dtype=np.uint32), H0)
    assert np.array_equal(rows, all_rows(H0, 2))
    whole = dev.features(cam, p, rows).reshape(-1)
    ids = shuffled_ids_with_repeats(2 * W0 * H0, seed=len(name))
    got, st = dev.features_pixels(cam, p, ids, want_stats=True)                 # the counter instance
    assert got.shape == (ids.size,) and got.dtype == F.FEATURE_DTYPE
    assert_same_bits(got, whole[ids], "counter instance")
    assert st.paths == st.rays == ids.size * SPP0 and st.ms > 0 and st.node_visits >= st.rays
    assert_same_bits(dev.features_pixels(cam, p, ids), whole[ids], "plain instance")
    assert whole["hits"].sum() > 20


# ---- 2. against the oracle composition, with its counters --------------------------------------------------------------
def oracle_case(rt, which):
    if which == "every_kind":
        b, d, _ = every_material_scene(rt)
        cam = rt.camera_new((0, 1.8, 10), (0, 1.6, 0), (0, 1, 0), 40.0, W0 / H0, 0.0, 10.0, 0.0, 1.0)
        return b, d, cam, (0.25, 0.5, 0.75)
    s = rt.HostScene(which, seed=2022)
    cam, bg = s.default_view(W0 / H0)
    if which == "random_scene":                                                 # an open shutter and a lens
        cam = rt.camera_new((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W0 / H0, 0.3, 10.0, 0.0, 1.0)
    return s, s.desc, cam, bg


@pytest.mark.parametrize("which", ["every_kind", "cornell_smoke", "random_scene"])
def test_oracle_composition_and_counters(rt, O, which):
    keep, d, cam, bg = oracle_case(rt, which)
    p = rt.make_params(W0, H0, SPP0, 50, bg, seed=41, n_frames=2)
    g = np.random.default_rng(3)
    ids = np.concatenate([g.permutation(W0 * H0), W0 * H0 + g.integers(0, W0 * H0, 40), g.integers(0, W0 * H0, 20)]).astype(np.uint64)
    dev = rt.DeviceScene(d)
    got, st = dev.features_pixels(cam, p, ids, want_stats=True)
    ref, st_ref, seen = oracle_ids(O, d, cam, p, ids)
    assert_same_bits(got, ref)
    check_first_hit_counters(st, st_ref, seen, ids.size, SPP0)
    if which == "cornell_smoke":
        assert seen.medium_draws > 0
    if which == "random_scene":
        assert seen.draws > 5 * ids.size * SPP0                                 # two jitter words, at least two lens words, the shutter's
    assert_same_bits(dev.features_pixels(cam, p, ids), ref, "plain instance")


# ---- 3. list lengths --------------------------------------------------------------------------------------------------
def test_list_lengths_and_permutations(rt):
    W = H = 8
    s = rt.HostScene("cornell_box", seed=2022)
    cam, bg = s.default_view(1.0)
    dev = rt.DeviceScene(s.desc)
    p = rt.make_params(W, H, SPP0, 50, bg, seed=6, n_frames=2)
    whole = dev.features(cam, p, all_rows(H, 2)).reshape(-1)
    g = np.random.default_rng(9)
    for n in (1, 63, 64, 65, 257):
        ids = g.integers(0, 2 * W * H, n).astype(np.uint64)
        got = dev.features_pixels(cam, p, ids)
        assert_same_bits(got, whole[ids], "length %d" % n)
        perm = g.permutation(n)
        assert_same_bits(dev.features_pixels(cam, p, ids[perm]), got[perm], "permutation of length %d" % n)
    # one entry more than the persistent grid has lanes (the larger workgroup of the instances, to be past either): every
    # lane claims a second time or idles, and the last entry is claimed by a lane that has finished one
    p1 = rt.make_params(W, H, 1, 50, bg, seed=6, n_frames=2)
    whole1 = dev.features(cam, p1, all_rows(H, 2)).reshape(-1)
    n = dev.info()["grid_blocks"] * 1024 + 1
    assert 1024 < n < (1 << 24)
    ids = (np.arange(n, dtype=np.uint64) * np.uint64(5)) % np.uint64(2 * W * H)
    got, st = dev.features_pixels(cam, p1, ids, want_stats=True)
    assert st.paths == st.rays == n
    assert_same_bits(got, whole1[ids], "past the grid's lanes")


# ---- 4. ids past 2^32 -------------------------------------------------------------------------------------------------
def test_ids_past_32_bits_take_the_64_bit_decode(rt, O):
    W = H = 8
    s = rt.HostScene("cornell_smoke", seed=2022)
    cam, bg = s.default_view(1.0)
    dev = rt.DeviceScene(s.desc)
    far = 1 << 27
    big = rt.make_params(W, H, SPP0, 50, bg, seed=12, n_frames=far + 1)
    assert W * H * big.n_frames > (1 << 32) and H * big.n_frames <= 0xFFFFFFFF
    g = np.random.default_rng(2)
    py, px = g.integers(0, H, 48), g.integers(0, W, 48)
    low = rt.pixel_ids(np.repeat([0, 1], 24), py, px, W, H)
    high = rt.pixel_ids(far, py[:24], px[:24], W, H)
    assert high.min() >= (1 << 32)
    ids = np.concatenate([low, high, [np.uint64(W * H * (far + 1) - 1)]]).astype(np.uint64)
    got, st = dev.features_pixels(cam, big, ids, want_stats=True)
    ref, st_ref, seen = oracle_ids(O, s.desc, cam, big, ids)
    assert_same_bits(got, ref, "64-bit decode")
    check_first_hit_counters(st, st_ref, seen, ids.size, SPP0)
    small = rt.make_params(W, H, SPP0, 50, bg, seed=12, n_frames=2)            # the same entries through the 32-bit decode
    assert_same_bits(dev.features_pixels(cam, small, low), got[:48], "32-bit decode")
    edge = rt.make_params(W, H, SPP0, 50, bg, seed=12, n_frames=(1 << 32) // (W * H))     # the largest view that still fits: ids < 2^32
    top = np.concatenate([low, [np.uint64((1 << 32) - 1)]]).astype(np.uint64)
    got_edge = dev.features_pixels(cam, edge, top)
    assert_same_bits(got_edge[:48], got[:48], "the last 32-bit view")
    ref_top, _, _ = oracle_ids(O, s.desc, cam, edge, top[-1:])
    assert_same_bits(got_edge[-1:], ref_top, "id 2^32 - 1")


# ---- 5. divide by zero ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 8), (8, 1), (1, 1)])
def test_one_pixel_wide_or_high_divides_by_zero_like_rt_features(rt, W, H):
    s = rt.HostScene("cornell_box", seed=2022)
    cam, bg = s.default_view(1.0)
    p = rt.make_params(W, H, SPP0, 50, (0.1, 0.2, 0.3), seed=2, n_frames=2)
    dev = rt.DeviceScene(s.desc)
    whole = dev.features(cam, p, all_rows(H, 2)).reshape(-1)
    ids = np.random.default_rng(1).permutation(2 * W * H).astype(np.uint64)
    got = dev.features_pixels(cam, p, ids)
    assert_same_bits(got, whole[ids])
    assert (np.isnan(whole.view(np.float64)).any()) or ((whole["hits"] == 0).any())      # (the case is not a plain frame)


# ---- 6. refused device ids --------------------------------------------------------------------------------------------
def test_device_ids_out_of_range_leave_the_output_untouched(rt):
    import torch
    s = rt.HostScene("cornell_box", seed=2022)
    cam, bg = s.default_view(W0 / H0)
    p = rt.make_params(W0, H0, SPP0, 50, bg, seed=8, n_frames=2)
    dev = rt.DeviceScene(s.desc)
    stream = torch.cuda.Stream()
    ids = np.random.default_rng(5).integers(0, 2 * W0 * H0, 100).astype(np.uint64)
    want = dev.features_pixels(cam, p, ids)
    bad = ids.copy()
    bad[37] = 2 * W0 * H0                                                       # == width * height * n_frames
    d_bad, d_ids = torch.from_numpy(bad.view(np.int64)).cuda(), torch.from_numpy(ids.view(np.int64)).cuda()
    poison = np.random.default_rng(6).integers(1, 1 << 62, 100 * 8).astype(np.int64)
    d_out = torch.from_numpy(poison).cuda()
    torch.cuda.synchronize()
    with pytest.raises(rt.RtError) as e:
        dev.features_pixels_device(cam, p, d_bad.data_ptr(), 100, d_out.data_ptr(), stream.cuda_stream)
    assert e.value.code == F.RT_ERR_INVALID and "pixel id out of range" in str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), poison)                          # bit-unchanged
    with pytest.raises(rt.RtError):                                             # ... also when nothing would be traced
        dev.features_pixels_device(cam, rt.make_params(W0, H0, 0, 50, bg, n_frames=2), d_bad.data_ptr(), 100, d_out.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), poison)
    dev.features_pixels_device(cam, p, d_ids.data_ptr(), 100, d_out.data_ptr(), stream.cuda_stream)     # the next valid call
    stream.synchronize()
    assert_same_bits(d_out.cpu().numpy().view(np.float64).view(F.FEATURE_DTYPE), want)
    dev.features_pixels_device(cam, rt.make_params(W0, H0, 0, 50, bg, n_frames=2), d_ids.data_ptr(), 100, d_out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert not d_out.cpu().numpy().any()                                        # spp == 0: zeros


# ---- 7. torch buffers, streams and engines ----------------------------------------------------------------------------
def test_torch_buffers_beside_an_asynchronous_render_and_either_engine(rt):
    import torch
    W, H, spp = 24, 16, 3
    s = rt.HostScene("final_scene", seed=2022)
    cam, bg = s.default_view(W / H)
    p = rt.make_params(W, H, spp, 50, bg, seed=2022, spp_chunk=1, n_frames=2)
    dev = rt.DeviceScene(s.desc)
    rows = rt.shuffled_rows(H, 3)
    ids = shuffled_ids_with_repeats(2 * W * H, seed=4)
    n = ids.size
    whole = dev.features(cam, p, all_rows(H, 2)).reshape(-1)
    ref_render = dev.render(cam, p, rows)
    a_stream, b_stream = torch.cuda.Stream(), torch.cuda.Stream()
    d_ids = torch.from_numpy(ids.view(np.int64)).cuda()
    d_out = torch.full((n * 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev.features_pixels_device(cam, p, d_ids.data_ptr(), n, d_out.data_ptr(), b_stream.cuda_stream)     # stats=None: enqueued, not waited for
    b_stream.synchronize()
    out = d_out.cpu().numpy()
    assert_same_bits(out[: n * 8].view(F.FEATURE_DTYPE), whole[ids], "non-default stream")
    assert np.isnan(out[n * 8:]).all()                                          # nothing past the last record
    st = F.rt_stats()
    d_out.fill_(float("nan"))
    torch.cuda.synchronize()
    dev.features_pixels_device(cam, p, d_ids.data_ptr(), n, d_out.data_ptr(), b_stream.cuda_stream, stats=st)
    assert_same_bits(d_out.cpu().numpy()[: n * 8].view(F.FEATURE_DTYPE), whole[ids], "with stats")      # (the call has synchronised)
    assert st.paths == st.rays == n * spp and st.node_visits > st.rays and st.rng_draws >= 5 * st.rays and st.ms > 0
    # beside an RT_FLAG_ASYNC render of the same scene on another stream
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    image = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda")
    feats = [torch.full((n * 8,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    dev.render_device(cam, p, d_rows.data_ptr(), H, image.data_ptr(), a_stream.cuda_stream, None, asynchronous=True)
    for f_ in feats:
        dev.features_pixels_device(cam, p, d_ids.data_ptr(), n, f_.data_ptr(), b_stream.cuda_stream)
    b_stream.synchronize()
    dev.wait(a_stream.cuda_stream)
    assert np.array_equal(image.cpu().numpy().view(np.uint64), ref_render.view(np.uint64))
    for f_ in feats:
        assert_same_bits(f_.cpu().numpy().view(F.FEATURE_DTYPE), whole[ids], "beside a render")
    assert np.array_equal(dev.render(cam, p, rows).view(np.uint64), ref_render.view(np.uint64))         # the render's workspace is untouched
    # the call uses neither engine
    dev.set_engine("mega")
    assert_same_bits(dev.features_pixels(cam, p, ids), whole[ids], "megakernel engine selected")


# ---- 8. a deep-stack instance ------------------------------------------------------------------------------------------
def test_deep_stack_instance_on_single_pixels_of_the_full_view(rt, O):
    """The C5 mesh (0.84 M triangles under three movers): 2 048 entries of the 800 x 800 view, which only a pixel list can ask for."""
    s = rt.HostScene("wwscene", seed=2022, param=3, assets_dir=ASSETS)
    d = s.desc
    assert d.n_nodes > 100_000
    W = H = 800
    spp = 2
    cam, bg = s.default_view(1.0)
    p = rt.make_params(W, H, spp, 50, bg, seed=3, n_frames=2)
    dev = rt.DeviceScene(d)
    assert dev.info()["stack_need"] > 16                                        # not the LDS-prefix instance
    ids = np.random.default_rng(2048).integers(0, 2 * W * H, 2048).astype(np.uint64)
    got, st = dev.features_pixels(cam, p, ids, want_stats=True)
    ref, st_ref, seen = oracle_ids(O, d, cam, p, ids)
    assert_same_bits(got, ref)
    check_first_hit_counters(st, st_ref, seen, ids.size, spp)
    assert_same_bits(dev.features_pixels(cam, p, ids), ref, "plain instance")
    assert got["hits"].sum() > 100


# ---- 9. merge and resolve ---------------------------------------------------------------------------------------------
def nan_eq_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.where(np.isnan(a), 0.0, a).view(np.uint64), np.where(np.isnan(b), 0.0, b).view(np.uint64))


@pytest.mark.parametrize("w,h", [(5, 3), (40, 30)])
def test_feature_merge_and_resolve_match_the_restatement(rt, w, h):
    import torch
    n, max_units, spp = w * h, 3, 4
    g = np.random.default_rng(w)
    err = g.random(n) * 4.5
    err[::4] = 0.0
    err[1] = np.inf
    units, offsets, _, total = rt.adaptive_plan(err.reshape(h, w), rt.adaptive_params(w, h, 1.0, max_units))      # a real plan
    units = units.ravel()
    assert (units == 0).any() and (units == max_units).any() and total == int(units.sum()) > 0
    E = g.normal(size=(2 * total, 8)) * 10.0
    E[2, 3] = np.nan
    E[total + 1, 6] = np.inf
    E[total - 1, 0] = -np.inf
    acc = g.random((2, n, 8))
    poison = np.float64(-1.2345e300)
    acc[:, units == 0] = poison
    acc_n = np.full((2, n), float(spp)) + units * float(spp)
    zero_n = int(np.nonzero(units)[0][0])
    acc_n[0, zero_n] = 0.0                                                      # a pixel with no sample
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_E, d_acc, d_acc_n = cu(E), cu(acc), cu(acc_n)
    d_units, d_offsets = cu(units.view(np.int32)), cu(offsets.view(np.int64))
    torch.cuda.synchronize()
    for half in range(2):
        rt.adaptive_merge_features_device(d_E.data_ptr() + 64 * total * half, d_units.data_ptr(), d_offsets.data_ptr(), n, d_acc[half].data_ptr(), sp)
        FR.merge(E[total * half: total * (half + 1)], units, offsets, acc[half])
    stream.synchronize()
    merged = d_acc.cpu().numpy()
    assert nan_eq_bits(merged, acc)
    assert np.all(merged[:, units == 0] == poison)                              # 0 units: not written
    assert np.array_equal(d_acc_n.cpu().numpy(), acc_n)                         # the merge touches no sample count
    d_out = torch.full((n, 8), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rt.adaptive_resolve_features_device(d_acc[0].data_ptr(), d_acc_n[0].data_ptr(), n, 16, d_out.data_ptr(), sp)
    rt.adaptive_resolve_features_device(d_acc[1].data_ptr(), d_acc_n[1].data_ptr(), n, 16, d_acc[1].data_ptr(), sp)      # out aliases acc
    stream.synchronize()
    want0, want1 = FR.resolve(acc[0], acc_n[0], 16), FR.resolve(acc[1], acc_n[1], 16)
    assert nan_eq_bits(d_out.cpu().numpy(), want0) and nan_eq_bits(d_acc[1].cpu().numpy(), want1)
    assert not np.isfinite(want0[zero_n]).any()                                # acc_n == 0: inf or NaN in every field
    zero_acc = np.zeros((1, 8))
    d_z, d_zn = cu(zero_acc), cu(np.zeros(1))
    rt.adaptive_resolve_features_device(d_z.data_ptr(), d_zn.data_ptr(), 1, 16, d_z.data_ptr(), sp)
    stream.synchronize()
    assert np.isnan(d_z.cpu().numpy()).all()                                    # 0 / 0: NaN in all eight fields


# ---- 10. render_adaptive(guides="all") ---------------------------------------------------------------------------------
def test_render_adaptive_with_guides_from_every_sample(rt):
    W = H = 24
    n = W * H
    spp, total_spp, max_units = 4, 32, 4
    s = rt.HostScene("cornell_box", seed=2022)
    cam, bg = s.default_view(1.0)
    dev = rt.DeviceScene(s.desc)
    p = rt.make_params(W, H, spp, 50, bg, seed=2022)
    run = lambda rounds: rt.render_adaptive(dev, cam, p, total_spp, rounds=rounds, max_units=max_units, want_state=True, guides="all")
    out, counts, log, state = run(2)
    out2, counts2, log2, state2 = run(2)
    o, c = out.cpu().numpy(), counts.cpu().numpy()
    assert nan_eq_bits(o, out2.cpu().numpy()) and nan_eq_bits(c, counts2.cpu().numpy()) and log == log2
    assert nan_eq_bits(state["feat_acc"].cpu().numpy(), state2["feat_acc"].cpu().numpy())
    assert o.shape == (H, W, 3) and c.shape == (H, W) and tuple(state["feat_acc"].shape) == (2, n, 8)
    spent = 2 * spp * n + sum(r["samples"] for r in log)
    assert spent == int(c.sum()) and spent <= total_spp * n
    assert np.all(c >= 2 * spp) and np.all(c % (2 * spp) == 0) and c.max() <= 2 * spp * (1 + 2 * max_units)
    assert len(log) == 2 and all(r["total"] <= r["budget_units"] for r in log) and sum(r["total"] for r in log) > 0
    hits = state["feat_acc"].cpu().numpy()[..., 7]
    assert np.all(hits <= state["acc_n"].cpu().numpy().reshape(2, n)) and np.array_equal(hits, np.floor(hits))
    with pytest.raises(ValueError):
        rt.render_adaptive(dev, cam, p, total_spp, guides="some")
    assert "feat_acc" not in rt.render_adaptive(dev, cam, p, total_spp, want_state=True)[3]
    # one round: the accumulated records are the initial ones plus rt_features of the frames the plan named, in order
    out, counts, log, state = run(1)
    assert log[0]["total"] > 0
    acc_n = state["acc_n"].cpu().numpy().reshape(2, n)
    feat_acc = state["feat_acc"].cpu().numpy()
    want = state["feat"].cpu().numpy().copy()
    pf = rt.make_params(W, H, spp, 50, bg, seed=2022, n_frames=2 + 2 * max_units)
    frames = dev.features(cam, pf, all_rows(H, 2 + 2 * max_units)).view(np.float64).reshape(2 + 2 * max_units, n, 8)
    assert_same_bits(frames[:2], want, "the initial frames")
    for h in range(2):
        units = (acc_n[h] - spp) / spp
        assert np.array_equal(units, np.floor(units)) and units.min() >= 0 and units.max() <= max_units and units.sum() == log[0]["total"]
        for k in range(max_units):
            m = units > k
            want[h, m] = want[h, m] + frames[2 + h * max_units + k, m]
    assert_same_bits(feat_acc, want, "feat_acc after one round")
    # hits == acc_n exactly wherever every camera ray hits. The default view is NOT closed at the image border: the camera
    # stands at z = -800 with a 40 degree field of view, so at the box's opening (z = 0) the view is 2 * 800 * tan(20 deg) =
    # 582 wide around x = y = 278, from -13 to 569 — wider than the 555 opening — and border pixels' rays pass outside the
    # walls. Pixel j spans [j, j + 1) / (W - 1) of that width (the render divides by W - 1), so pixels 1 .. 21 of 24 lie
    # inside (0, 555) and pixels 0, 22 and 23 do not. Inside that border the box is closed; "every ray hits" is read off
    # rt_features itself, over all the frames there are.
    closed = np.all(frames[..., 7] == spp, axis=0)
    inner = np.zeros((H, W), dtype=bool)
    inner[1:22, 1:22] = True
    assert np.all(closed[inner.ravel()]) and not np.all(closed)
    assert np.array_equal(feat_acc[:, closed, 7], acc_n[:, closed]) and np.all(feat_acc[..., 7] <= acc_n)
    assert (acc_n[:, closed] > spp).any()                                       # ... and some of them got units
