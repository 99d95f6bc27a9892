"""Temporal accumulation (rt_temporal / rt_temporal_device) against the numpy restatement of its definition
(tests/temporal_ref.py), bit for bit: every comparison is on the uint64 view, the NaN patterns first. The shapes are those at
which the kernel can go wrong: no multiple of the 64 x 4 workgroup, several workgroups each way, images smaller than one, a
width or a height of one."""
import ctypes as C
import math

import numpy as np
import pytest

from raytracer_2022_amd import _ffi as F

import denoise_dual_ref as D
import temporal_cases as T
import temporal_ref as R
from compare import assert_same_bits
from denoise_ref import LONG_HEIGHTS, LONG_W, long_row_lists
from gpu_first import torch_first  # noqa: F401
from temporal_cases import Device

pytestmark = pytest.mark.gpu

SIZES = [(67, 35), (130, 9), (1, 1), (1, 9), (9, 1), (5, 3)]
CAMERAS = ["moved", "identical", "previous camera facing away", "every tap outside"]
INF = math.inf
SWITCHES = {"n_max 1": dict(n_max=1.0), "depth test off": dict(tol_depth=INF), "normal test off": dict(tol_normal=INF),
            "both tests off": dict(tol_depth=INF, tol_normal=INF), "no demodulation": dict(demodulate=False), "w_min 1": dict(w_min=1.0),
            "tight": dict(tol_depth=0.02, tol_normal=0.05, n_max=2.5, w_min=0.6, albedo_floor=0.3)}


def check(rt, s, f, cam, p, prev=None, prev_cam=None, rows=None, what=""):
    got, state = rt.temporal(s, f, cam, p, prev=prev, prev_cam=prev_cam, row_ids=rows)
    ref, ref_state = R.restate(s, f, cam, p, prev, prev_cam, rows)
    assert got.shape == np.asarray(s).shape and state.shape == (p.height, p.width)
    assert_same_bits(got, ref, what)
    assert_same_bits(state, ref_state, (what, "state"))
    return got, state


def chain(rt, W, H, cams, p, seed, hostile=True, frames=4, what=""):
    """A first frame (no history) and three more on top of each other, the cameras alternating; the third frame's history is
    poisoned. -> the states, and how many pixels took their history."""
    cam, prev_cam = cams
    state, taken, states = None, 0, []
    for k in range(frames):
        s, f = T.frame(W, H, seed=seed + k, hostile=hostile)
        now, before = (cam, prev_cam) if k % 2 else (prev_cam, cam)
        if k == 2 and hostile:
            state = T.poisoned(state, seed)
        _, state = check(rt, s, f, now, p, state, before if k else None, what=(what, "frame", k))
        taken += int((state["n"] > 1.0).sum()) if k else 0
        states.append(state)
    return states, taken


# ---- bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cams", CAMERAS)
@pytest.mark.parametrize("W, H", SIZES)
def test_hostile_frames_chained(rt, W, H, cams):
    p = rt.temporal_params(W, H, 4)
    states, taken = chain(rt, W, H, T.cameras(rt, W, H)[cams], p, seed=W * 16 + H, what=cams)
    assert (states[0]["n"] == 1.0).all()
    if cams in ("moved", "identical") and W * H > 500:
        assert taken > 0, "no pixel ever took its history"
    if min(W, H) == 1:                                     # sc or tc is infinite: every pixel restarts
        assert taken == 0


@pytest.mark.parametrize("name", list(SWITCHES))
def test_switches(rt, name):
    W, H = 67, 35
    p = rt.temporal_params(W, H, 4, **SWITCHES[name])
    states, taken = chain(rt, W, H, T.cameras(rt, W, H)["moved"], p, seed=5, what=name)
    assert taken > 0 or p.n_max == 1.0                      # (taken counts n > 1)
    assert all((s["n"] >= 1.0).all() and s["n"].max() <= p.n_max for s in states)      # (an infinite or NaN length in the history gives n_max)


def test_n_max_1_is_demodulate_then_remodulate(rt):
    """No history is kept: e_out = eh + (e - eh), the frame's own value to rounding, and the sums come back as they went in."""
    W, H = 67, 35
    cam, prev_cam = T.cameras(rt, W, H)["moved"]
    p = rt.temporal_params(W, H, 4, n_max=1.0)
    (s0, f0), (s1, f1) = T.frame(W, H, seed=1, hostile=False), T.frame(W, H, seed=2, hostile=False)
    _, st0 = check(rt, s0, f0, prev_cam, p)
    out, st1 = check(rt, s1, f1, cam, p, st0, prev_cam)
    assert (st1["n"] == 1.0).all()
    # e = c / m, e - eh, eh + (..), * m, * sp: five roundings, the middle two on numbers up to 2 max |e|; m <= 1 here
    bound = 4 * np.finfo(np.float64).eps * max(np.abs(st0["e"]).max(), np.abs(st1["e"]).max()) * p.spp
    assert np.abs(out - s1).max() <= bound
    first, _ = check(rt, s1, f1, cam, p)
    assert np.allclose(first, s1, rtol=1e-13)


@pytest.mark.parametrize("spp", [1, 7])
def test_other_sample_counts(rt, spp):
    W, H = 70, 9
    p = rt.temporal_params(W, H, spp)
    cam, prev_cam = T.cameras(rt, W, H)["moved"]
    (s0, f0), (s1, f1) = T.frame(W, H, spp=spp, seed=1), T.frame(W, H, spp=spp, seed=2)
    _, st0 = check(rt, s0, f0, prev_cam, p)
    check(rt, s1, f1, cam, p, st0, prev_cam)


# ---- the device form on torch buffers (temporal_cases.Device) --------------------------------------------------------------
def two_frames(rt, W, H, seed, rows=None):
    """A first frame's state (the restatement's) and a second frame in the order of `rows`, with the `moved` cameras."""
    cam, prev_cam = T.cameras(rt, W, H)["moved"]
    p = rt.temporal_params(W, H, 4)
    s0, f0 = T.frame(W, H, seed=seed, hostile=False)
    s1, f1 = T.frame(W, H, seed=seed + 1, hostile=True)
    _, st0 = R.restate(s0, f0, prev_cam, p)
    if rows is not None:
        s1, f1 = s1[rows], f1[rows]
    return p, cam, prev_cam, st0, s1, f1


def test_shuffled_rows_give_the_image_order_result_permuted(rt):
    W, H = 67, 35
    p, cam, prev_cam, st0, s1, f1 = two_frames(rt, W, H, 9)
    image_order, image_state = check(rt, s1, f1, cam, p, st0, prev_cam)
    rows = rt.shuffled_rows(H, 2022)
    got, state = check(rt, s1[rows], f1[rows], cam, p, st0, prev_cam, rows=rows, what="shuffled rows")
    assert_same_bits(got[np.argsort(rows)], image_order, "the sums come back in the rows' order")
    assert_same_bits(state, image_state, "the state stays in image order")
    check(rt, s1[rows], f1[rows], cam, p, rows=rows, what="shuffled rows, first frame")


def test_bad_row_lists_are_refused_with_both_outputs_untouched(rt):
    import torch
    W, H = 12, 10
    p, cam, prev_cam, st0, s1, f1 = two_frames(rt, W, H, 3)
    d = Device(rt, s1, f1, p, st0)
    for fault in ("repeated", "out of range", "huge"):
        rows = np.arange(H, dtype=np.uint32)[::-1].copy()
        rows[3] = {"repeated": rows[7], "out of range": H, "huge": 0xFFFFFFFF}[fault]
        with pytest.raises(rt.RtError) as e:
            rt.temporal(s1, f1, cam, p, prev=st0, prev_cam=prev_cam, row_ids=rows)
        assert e.value.code == F.RT_ERR_INVALID and "not a permutation" in str(e.value), fault
        d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
        torch.cuda.synchronize()
        with pytest.raises(rt.RtError) as e:
            d.call(cam, prev_cam, rows=d_rows)
        assert e.value.code == F.RT_ERR_INVALID and "not a permutation" in str(e.value), fault
        torch.cuda.synchronize()
        assert (d.out == 7.0).all() and (d.state == 7.0).all(), (fault, "an output was written")
    # and the good list on the same workspace afterwards
    rows = np.arange(H, dtype=np.uint32)[::-1].copy()
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    torch.cuda.synchronize()
    d.call(cam, prev_cam, rows=d_rows)
    out, state = d.results()
    ref, ref_state = R.restate(s1, f1, cam, p, st0, prev_cam, rows)
    assert_same_bits(out, ref, "good rows after bad ones")
    assert_same_bits(state, ref_state, "good rows after bad ones, state")


@pytest.mark.parametrize("H", LONG_HEIGHTS)
def test_row_lists_longer_than_the_row_kernels_block(rt, H):
    """post_rows' stride loop (pt_rows.hip, one workgroup of 1024 threads): a thread's second trip starts at 1025 rows. One
    chained pair of frames, each in a shuffled order of its own, against the restatement; the device form refuses a repeat
    across trips, a repeat inside one thread and an id out of range on the last trip with both outputs untouched, and takes
    the good list on the same workspace afterwards."""
    import torch
    W = LONG_W
    rows, bad = long_row_lists(H, H + 2)
    rows0 = np.random.default_rng(H + 3).permutation(H).astype(np.uint32)
    cam, prev_cam = T.cameras(rt, W, H)["moved"]
    p = rt.temporal_params(W, H, 4)
    s0, f0 = T.frame(W, H, seed=H, hostile=False)
    s1, f1 = T.frame(W, H, seed=H + 1, hostile=True)
    _, st0 = check(rt, s0[rows0], f0[rows0], prev_cam, p, rows=rows0, what="first frame")
    s1, f1 = s1[rows], f1[rows]
    _, st1 = check(rt, s1, f1, cam, p, st0, prev_cam, rows=rows, what="second frame")
    assert (st1["n"] > 1.0).any(), "no pixel took its history"
    ref, ref_state = R.restate(s1, f1, cam, p, st0, prev_cam, rows)
    d = Device(rt, s1, f1, p, st0, fill=0xFF)
    for fault, lst in bad.items():
        d_rows = torch.from_numpy(lst.view(np.int32)).cuda()
        torch.cuda.synchronize()
        with pytest.raises(rt.RtError) as e:
            d.call(cam, prev_cam, rows=d_rows)
        assert e.value.code == F.RT_ERR_INVALID and "not a permutation" in str(e.value), fault
        torch.cuda.synchronize()
        assert (d.out == 7.0).all() and (d.state == 7.0).all(), (fault, "an output was written")
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    torch.cuda.synchronize()
    d.call(cam, prev_cam, rows=d_rows)
    out, state = d.results()
    assert_same_bits(out, ref, "good rows after bad ones")
    assert_same_bits(state, ref_state, "good rows after bad ones, state")


def test_aliasing_workspace_reuse_and_poisoned_workspace(rt):
    import torch
    W, H = 67, 35
    rows = rt.shuffled_rows(H, 7)
    p, cam, prev_cam, st0, s1, f1 = two_frames(rt, W, H, 5, rows)
    ref = R.restate(s1, f1, cam, p, st0, prev_cam, rows)
    d = Device(rt, s1, f1, p, st0, fill=0xFF)              # a workspace of 0xFF bytes
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    torch.cuda.synchronize()

    def same(what, out=None, r=ref):
        got, state = d.results(out)
        assert_same_bits(got, r[0], what)
        assert_same_bits(state, r[1], (what, "state"))

    d.call(cam, prev_cam, rows=d_rows)
    same("poisoned workspace")
    d.out.fill_(7.0), d.state.fill_(7.0)
    d.call(cam, prev_cam, rows=d_rows)                     # the same workspace again
    same("workspace reused")
    # ... with no row list after a call with one (the inverse map of the last call is still in the workspace)
    d.out.fill_(7.0), d.state.fill_(7.0)
    d.call(cam, prev_cam)
    same("workspace reused without rows", r=R.restate(s1, f1, cam, p, st0, prev_cam))
    # in place: the output is the input sums
    d.state.fill_(7.0)
    d.call(cam, prev_cam, out=d.sums, rows=d_rows)
    same("output aliasing the sums", out=d.sums)
    assert np.array_equal(d.prev.cpu().numpy().view(np.uint64), np.ascontiguousarray(st0).view(np.uint64).reshape(-1))   # read only


def test_analytic_cases_on_the_device(rt):
    """The plane shift and the disocclusion of tests/test_temporal_ref.py through rt_temporal_device."""
    p, (s0, f0), prev_cam, (s1, f1), cam = T.plane_shift_case(rt)
    d0 = Device(rt, s0, f0, p)
    d0.call(prev_cam)
    _, st0 = d0.results()
    d1 = Device(rt, s1, f1, p, st0)
    d1.call(cam, prev_cam)
    _, st1 = d1.results()
    assert_same_bits(st1, R.restate(s1, f1, cam, p, st0, prev_cam)[1], "plane shift")
    own = Device(rt, s1, f1, p)
    own.call(cam)
    T.check_plane_shift(st1, st0, own.results()[1]["e"], p.width)

    p, (s0, f0), prev_cam, (s1, f1), cam, restart = T.disocclusion_case(rt)
    d0 = Device(rt, s0, f0, p)
    d0.call(prev_cam)
    _, st0 = d0.results()
    d1 = Device(rt, s1, f1, p, st0)
    d1.call(cam, prev_cam)
    _, st1 = d1.results()
    assert_same_bits(st1, R.restate(s1, f1, cam, p, st0, prev_cam)[1], "disocclusion")
    assert (st1["n"][:, restart] == 1.0).all() and (st1["n"][:, ~restart] == st0["n"][:, ~restart] + 1.0).all()


def test_two_halves_on_a_stream_then_dual_denoise_and_tonemap(rt):
    """Two halves accumulated over three cameras with torch buffers on a stream of the caller's, rt_denoise_dual_device and
    rt_tonemap_device behind them on the same stream: the host path's bits."""
    import torch
    W, H, spp = 130, 21, 4
    base = T.camera(rt, W, H)
    cams = [R.shifted_camera(base, T.pixel_shift(base, W, T.Z_MID, 1.7 * k)) for k in range(3)]
    frames = [[T.frame(W, H, spp=spp, seed=100 * half + k, hostile=False) for k in range(3)] for half in range(2)]
    p = rt.temporal_params(W, H, spp)
    dp, dq = D.dual_blocks(rt, W, H, spp)
    # the host path
    host_out, host_state = [], []
    for half in range(2):
        state, out = None, None
        for k in range(3):
            out, state = rt.temporal(*frames[half][k], cams[k], p, prev=state, prev_cam=cams[k - 1] if k else None)
        host_out.append(out), host_state.append(state)
    fa, fb = frames[0][2][1], frames[1][2][1]
    host_dual, host_var = rt.denoise_dual(host_out[0], host_out[1], fa, fb, dp, dq, want_variance=True)
    # the device path
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float64).reshape(-1)).cuda()
    d_sums = [[up(s) for s, _ in frames[half]] for half in range(2)]
    d_feat = [[up(f) for _, f in frames[half]] for half in range(2)]
    d_state = [[torch.zeros(W * H * 8, dtype=torch.float64, device="cuda") for _ in range(2)] for half in range(2)]
    d_acc = [torch.zeros(W * H * 3, dtype=torch.float64, device="cuda") for half in range(2)]
    d_ws = torch.zeros(rt.temporal_workspace_bytes(p), dtype=torch.uint8, device="cuda")
    d_dual_ws = torch.zeros(rt.denoise_dual_workspace_bytes(dp), dtype=torch.uint8, device="cuda")
    d_dual = torch.zeros(W * H * 3, dtype=torch.float64, device="cuda")
    d_var = torch.zeros(W * H, dtype=torch.float64, device="cuda")
    d_u8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for half in range(2):
            for k in range(3):
                rt.temporal_device(d_sums[half][k].data_ptr(), d_feat[half][k].data_ptr(), cams[k], p, d_state[half][k & 1].data_ptr(),
                                   d_acc[half].data_ptr(), d_ws.data_ptr(), d_prev_ptr=d_state[half][~k & 1].data_ptr() if k else None,
                                   prev_cam=cams[k - 1] if k else None, stream_ptr=stream.cuda_stream)
        rt.denoise_dual_device(d_acc[0].data_ptr(), d_acc[1].data_ptr(), d_feat[0][2].data_ptr(), d_feat[1][2].data_ptr(), dp, dq,
                               d_dual.data_ptr(), d_dual_ws.data_ptr(), d_out_variance_ptr=d_var.data_ptr(), stream_ptr=stream.cuda_stream)
        F.check(rt.lib().rt_tonemap_device(C.c_void_p(d_dual.data_ptr()), W * H, 2 * spp, C.c_void_p(d_u8.data_ptr()), C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    for half in range(2):
        assert_same_bits(d_acc[half].cpu().numpy().reshape(H, W, 3), host_out[half], ("accumulated half", half))
        assert_same_bits(d_state[half][0].cpu().numpy().view(F.TEMPORAL_PIXEL_DTYPE).reshape(H, W), host_state[half], ("state of half", half))
        ref = R.accumulate([s for s, _ in frames[half]], [f for _, f in frames[half]], cams, p)
        assert_same_bits(host_out[half], ref[0], ("restatement of half", half))
        assert (host_state[half]["n"] > 2.0).any()
    assert_same_bits(d_dual.cpu().numpy().reshape(H, W, 3), host_dual, "dual filter behind the accumulation")
    assert_same_bits(d_var.cpu().numpy().reshape(H, W), host_var, "its variance")
    assert np.array_equal(d_u8.cpu().numpy(), rt.write_color(host_dual, 2 * spp))


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_render_features_temporal_end_to_end(rt, O):
    """DeviceScene.render + .features over the last 4 cameras of cornell_box's path at 48 x 48 x 4 spp through rt.temporal, rows
    shuffled: the oracle-renders-plus-restatement pipeline bit for bit (renders and features are the oracle's already)."""
    name, K = "cornell_box", 4
    W, H, spp = R.PATH_W, R.PATH_H, R.PATH_SPP
    rows = rt.shuffled_rows(H, 2022)
    s, bg, cams, sums, feats = R.oracle_path(rt, O, name, R.PATH_STEP[name], K=K, rows=rows)
    dev = rt.DeviceScene(s.desc)
    p = rt.temporal_params(W, H, spp)
    state, out = None, None
    for k in range(K):
        params = R.frame_params(rt, W, H, spp, bg, k)
        g_sums, g_feat = dev.render(cams[k], params, rows), dev.features(cams[k], params, rows)
        out, state = rt.temporal(g_sums, g_feat, cams[k], p, prev=state, prev_cam=cams[k - 1] if k else None, row_ids=rows)
    ref_out, ref_state, restarts = R.accumulate(sums, feats, cams, p, rows)
    assert_same_bits(out, ref_out, name)
    assert_same_bits(state, ref_state, (name, "state"))
    assert (state["n"] > K - 0.5).sum() > 0.3 * W * H, "much of the box is seen by all four cameras"
    dev.close()
