"""The adaptive planner, merge and resolve (rt_adaptive_*) against their numpy restatement (adaptive_ref.py), bit for bit, and
render_adaptive end to end on the Cornell box."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as R
from raytracer_2022_amd import _ffi as F

pytestmark = pytest.mark.gpu

# 1 x 1: one lane; 64 x 1: one wave; 65 x 3: a wave and a bit, one workgroup; 257 x 33 = 8481 pixels: nine tiles of 1024 —
# the block-totals level, with a last tile that is partly empty.
SIZES = [(1, 1), (64, 1), (65, 3), (257, 33)]


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU: the HIP path has no fallback"
    torch.zeros(1, device="cuda")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def error_maps(w, h, max_units, g):
    n = w * h
    hostile = g.random(n) * 6.0
    hostile[::5] = np.nan
    hostile[1::7] = np.inf
    hostile[2::11] = -np.inf
    hostile[3::13] = -1.5
    hostile[4::17] = -0.0
    hot = np.zeros(n)
    hot[-1] = 2.5
    return {"zeros": np.zeros(n), "all max": np.full(n, float(max_units)), "beyond max": np.full(n, 1e300), "hostile": hostile,
            "one hot pixel in the last place": hot, "random": g.random(n) * (max_units + 1.5), "below one": np.full(n, 0.999999)}


def check_plan(got, want, what):
    units, offsets, entries, total = got
    w_units, w_offsets, w_entries, w_total = want
    assert total == w_total, what
    assert np.array_equal(units.ravel(), w_units), what
    assert np.array_equal(offsets, w_offsets), what
    assert (entries is None) == (w_entries is None), what
    if entries is not None:
        assert np.array_equal(entries, w_entries), what


@pytest.mark.parametrize("w,h", SIZES)
def test_plan_matches_the_restatement(rt, w, h):
    g = np.random.default_rng(w * 1000 + h)
    max_units = 5
    for name, e in error_maps(w, h, max_units, g).items():
        for scale, first in ((1.0, 0), (0.73, 7)):
            p = rt.adaptive_params(w, h, scale, max_units, first_frame=first)
            check_plan(rt.adaptive_plan(e.reshape(h, w), p), R.plan(e, w, h, scale, max_units, first), (name, scale))
    e = error_maps(w, h, max_units, g)["random"]
    e[0] = 2.5                                                                       # (units for certain, also at 1 x 1)
    want = R.plan(e, w, h, 1.0, max_units, 3)
    p = rt.adaptive_params(w, h, 1.0, max_units, first_frame=3)
    total = want[3]
    assert total > 0
    # a capacity one short of the total: no entry, units and offsets valid; capacity 0 counts only; the exact capacity fits
    check_plan(rt.adaptive_plan(e.reshape(h, w), p, capacity=total - 1), R.plan(e, w, h, 1.0, max_units, 3, capacity=total - 1), "one short")
    check_plan(rt.adaptive_plan(e.reshape(h, w), p, capacity=0), R.plan(e, w, h, 1.0, max_units, 3, capacity=0), "capacity 0")
    check_plan(rt.adaptive_plan(e.reshape(h, w), p, capacity=total), want, "exact")
    check_plan(rt.adaptive_plan(e.reshape(h, w), p, capacity=total + 9), want, "roomy")
    # a row permutation: buffer row r is image row rows[r]
    rows = g.permutation(h).astype(np.uint32)
    check_plan(rt.adaptive_plan(e.reshape(h, w), p, row_ids=rows), R.plan(e, w, h, 1.0, max_units, 3, row_ids=rows), "rows")
    # frames at the top of the range, and ids that pass 2^32
    top = rt.adaptive_params(w, h, 1.0, max_units, first_frame=0xFFFFFFFF - max_units)
    check_plan(rt.adaptive_plan(e.reshape(h, w), top), R.plan(e, w, h, 1.0, max_units, 0xFFFFFFFF - max_units), "top frames")


def test_device_form_merge_resolve_and_the_two_half_recipe(rt):
    import torch
    w, h, max_units, spp = 257, 33, 3, 4
    n = w * h
    g = np.random.default_rng(77)
    e = g.random(n) * 4.5
    e[::9] = np.nan
    e[-1] = np.inf
    rows = g.permutation(h).astype(np.uint32)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_err, d_rows = cu(e), cu(rows.view(np.int32))
    d_units = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    p = rt.adaptive_params(w, h, 1.0, max_units, first_frame=2)
    d_ws = torch.empty(rt.adaptive_workspace_bytes(p), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    # a non-permutation is refused with nothing written
    for bad in (np.r_[rows[:-1], rows[0]], np.r_[rows[:-1], np.uint32(h)]):
        d_bad = cu(bad.astype(np.uint32).view(np.int32))
        torch.cuda.synchronize()
        total = C.c_uint64(123)
        rc = rt.lib().rt_adaptive_plan_device(C.c_void_p(d_err.data_ptr()), C.c_void_p(d_bad.data_ptr()), C.byref(p), C.c_void_p(d_units.data_ptr()),
                                              C.c_void_p(d_offsets.data_ptr()), None, 0, C.c_void_p(d_ws.data_ptr()), C.c_void_p(sp), C.byref(total))
        assert rc == F.RT_ERR_INVALID and "not a permutation" in rt.lib().rt_last_error().decode()
        torch.cuda.synchronize()
        assert torch.all(d_units == -1) and torch.all(d_offsets == -1) and total.value == 123
    # count, then the two halves' lists side by side: frames 2.. and 2 + max_units..
    want_a = R.plan(e, w, h, 1.0, max_units, 2, row_ids=rows)
    want_b = R.plan(e, w, h, 1.0, max_units, 2 + max_units, row_ids=rows)
    total = rt.adaptive_plan_device(d_err.data_ptr(), p, d_units.data_ptr(), d_offsets.data_ptr(), None, 0, d_ws.data_ptr(), d_rows.data_ptr(), sp)
    assert total == want_a[3] and np.array_equal(d_units.cpu().numpy().view(np.uint32), want_a[0])
    d_entries = torch.full((2 * total,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert rt.adaptive_plan_device(d_err.data_ptr(), p, d_units.data_ptr(), d_offsets.data_ptr(), d_entries.data_ptr(), total - 1, d_ws.data_ptr(),
                                   d_rows.data_ptr(), sp) == total
    torch.cuda.synchronize()
    assert torch.all(d_entries == -1)                                                # one short: no entry written
    rt.adaptive_plan_device(d_err.data_ptr(), p, d_units.data_ptr(), d_offsets.data_ptr(), d_entries.data_ptr(), total, d_ws.data_ptr(),
                            d_rows.data_ptr(), sp)
    p.first_frame = 2 + max_units
    rt.adaptive_plan_device(d_err.data_ptr(), p, d_units.data_ptr(), d_offsets.data_ptr(), d_entries.data_ptr() + 8 * total, total, d_ws.data_ptr(),
                            d_rows.data_ptr(), sp)
    got = d_entries.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:total], want_a[2]) and np.array_equal(got[total:], want_b[2])
    assert np.array_equal(d_offsets.cpu().numpy().view(np.uint64), want_a[1])
    # merge each half of the entry sums into its own accumulator (hostile sums included), then resolve — once in place
    sums = g.normal(size=(2 * total, 3)) * 10.0
    sums[5] = np.nan
    sums[total + 11, 1] = np.inf
    acc = g.random((2, n, 3))
    acc_n = np.full((2, n), float(spp))
    acc_n[0, 3] = 0.0                                                                # (a pixel with no sample: NaN unless the plan gave it units)
    d_sums, d_acc, d_acc_n = cu(sums), cu(acc), cu(acc_n)
    torch.cuda.synchronize()
    for half in range(2):
        rt.adaptive_merge_device(d_sums.data_ptr() + 24 * total * half, d_units.data_ptr(), d_offsets.data_ptr(), n, spp,
                                 d_acc[half].data_ptr(), d_acc_n[half].data_ptr(), sp)
        R.merge(sums[total * half:total * (half + 1)], want_a[0], want_a[1], spp, acc[half], acc_n[half])
    stream.synchronize()
    assert np.array_equal(bits(d_acc.cpu().numpy()), bits(acc)) and np.array_equal(bits(d_acc_n.cpu().numpy()), bits(acc_n))
    untouched = want_a[0] == 0
    assert untouched.any() and (~untouched).any()
    d_out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rt.adaptive_resolve_device(d_acc[0].data_ptr(), d_acc_n[0].data_ptr(), n, 16, d_out.data_ptr(), sp)
    rt.adaptive_resolve_device(d_acc[1].data_ptr(), d_acc_n[1].data_ptr(), n, 16, d_acc[1].data_ptr(), sp)         # out aliases acc
    stream.synchronize()
    want0, want1 = R.resolve(acc[0], acc_n[0], 16), R.resolve(acc[1], acc_n[1], 16)
    nan_eq = lambda a, b: np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(np.nan_to_num(a, nan=0.0, posinf=np.inf, neginf=-np.inf)),
                                                                                     bits(np.nan_to_num(b, nan=0.0, posinf=np.inf, neginf=-np.inf)))
    assert nan_eq(d_out.cpu().numpy(), want0) and nan_eq(d_acc[1].cpu().numpy(), want1)
    assert np.isnan(want0).any() and np.isfinite(want0).any()


def mean_image(sums, spp):
    return np.nan_to_num(np.asarray(sums, dtype=np.float64), nan=0.0) / float(spp)


def test_render_adaptive_end_to_end_on_the_cornell_box(rt):
    """Two runs give the same bits; the samples spent are the sum of the counts and within the budget; and the resolved image
    is closer to a 512 spp render than the two initial frames alone — a condition, not a figure: every sample added is
    independent of the ones before, so the expected error cannot rise. Seed 2022, the goldens' seed."""
    W = H = 24
    spp, total_spp = 4, 32
    s = rt.HostScene("cornell_box", seed=2022)
    cam, bg = s.default_view(1.0)
    dev = rt.DeviceScene(s.desc)
    p = rt.make_params(W, H, spp, 50, bg, seed=2022)
    out, counts, log = rt.render_adaptive(dev, cam, p, total_spp, rounds=2, max_units=4)
    out2, counts2, log2 = rt.render_adaptive(dev, cam, p, total_spp, rounds=2, max_units=4)
    o, c = out.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(np.isnan(o), np.isnan(out2.cpu().numpy()))
    assert np.array_equal(bits(np.nan_to_num(o)), bits(np.nan_to_num(out2.cpu().numpy())))
    assert np.array_equal(bits(c), bits(counts2.cpu().numpy())) and log == log2
    assert o.shape == (H, W, 3) and c.shape == (H, W)
    spent = 2 * spp * W * H + sum(r["samples"] for r in log)
    assert spent == int(c.sum()) and spent <= total_spp * W * H
    assert np.all(c >= 2 * spp) and np.all(c % (2 * spp) == 0) and c.max() <= 2 * spp * (1 + 2 * 4)
    assert len(log) == 2 and all(r["total"] <= r["budget_units"] for r in log) and sum(r["total"] for r in log) > 0
    print("render_adaptive log:", log)
    rows = np.arange(H, dtype=np.uint32)
    truth = mean_image(dev.render(cam, rt.make_params(W, H, 512, 50, bg, seed=99), rows), 512)
    p2 = F.rt_params.from_buffer_copy(p)
    p2.n_frames = 2
    ab = dev.render(cam, p2, rt.two_frame_rows(rows, H))
    initial = (mean_image(ab[:H], spp) + mean_image(ab[H:], spp)) * 0.5
    mse_initial = float(np.mean((initial - truth) ** 2))
    mse_adaptive = float(np.mean((mean_image(o, total_spp) - truth) ** 2))
    print("MSE against 512 spp: initial two frames %.6g, adaptive at %d spp average %.6g" % (mse_initial, total_spp, mse_adaptive))
    assert mse_adaptive < mse_initial
