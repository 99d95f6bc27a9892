"""The early returns of the three device forms of the feature calls (rt_features_device, rt_features_pixels_device,
rt_features_rays_device): no records, and no samples — what is written, what rt_stats holds, and what each source makes of its
list when there is nothing to trace. One matrix for the three sources, with and without stats. Every expectation is what the
library did when each of the three calls still had an enqueue of its own (the row and the pixel source differ at spp == 0, and
that is kept: FeatureJob, rt_query.hip)."""
import ctypes as C

import numpy as np
import pytest

from raytracer_2022_amd import _ffi as F

from gpu_first import torch_first  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 8, 6
COUNT = {"rows": 6, "pixels": 12, "rays": 12}             # rows, ids, rays
RECORDS = {"rows": 6 * W, "pixels": 12, "rays": 12}


@pytest.fixture(scope="module")
def box(rt):
    s = rt.HostScene("cornell_box", seed=2022)
    cam, bg = s.default_view(W / H)
    return rt.DeviceScene(s.desc), cam, bg


def device_list(source, rt, cam, bad=False):
    """The source's list in HBM (kept alive by the caller): six row ids, twelve pixel ids or twelve rays; `bad`: one id out of range."""
    import torch
    if source == "rows":
        ids = np.arange(6, dtype=np.uint32)
        if bad:
            ids[3] = H                                     # == height * n_frames
        return torch.from_numpy(ids.view(np.int32)).cuda()
    if source == "pixels":
        ids = np.arange(12, dtype=np.uint64) * 3
        if bad:
            ids[7] = W * H                                 # == width * height * n_frames
        return torch.from_numpy(ids.view(np.int64)).cuda()
    rays = rt.radiance_rays((278, 278, -800), [(0.01 * i, 0.0, 1.0) for i in range(12)])
    return torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()


def run(source, rt, box, d_list_ptr, count, spp, d_out, stats):
    dev, cam, bg = box
    if source == "rows":
        dev.features_device(cam, rt.make_params(W, H, spp, 50, bg, seed=3), d_list_ptr, count, d_out.data_ptr(), None, stats)
    elif source == "pixels":
        dev.features_pixels_device(cam, rt.make_params(W, H, spp, 50, bg, seed=3), d_list_ptr, count, d_out.data_ptr(), None, stats)
    else:
        dev.features_rays_device(d_list_ptr, count, d_out.data_ptr(), rt.radiance_params(spp, bg), None, stats)


def used_stats():
    """An rt_stats that looks used: a call that reports zeros has to write them."""
    st = F.rt_stats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    return st


def all_zero(st):
    return not any(bytes(st)) and st.ms == 0.0


def poisoned(records, seed):
    import torch
    poison = np.random.default_rng(seed).integers(1, 1 << 62, (records + 2) * 8).astype(np.int64)
    return poison, torch.from_numpy(poison).cuda()


@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("source", ["rows", "pixels", "rays"])
def test_no_records_write_nothing_and_no_samples_write_zeros(rt, box, source, with_stats):
    import torch
    _, cam, _ = box
    d_list = device_list(source, rt, cam)
    poison, d_out = poisoned(RECORDS[source], 1)
    torch.cuda.synchronize()
    # count == 0 (the buffers are there all the same): nothing written, stats all zero
    st = used_stats() if with_stats else None
    run(source, rt, box, d_list.data_ptr(), 0, 2, d_out, st)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), poison)
    assert st is None or all_zero(st)
    # spp == 0: zeros of exactly the call's records, stats all zero — ms too
    st = used_stats() if with_stats else None
    run(source, rt, box, d_list.data_ptr(), COUNT[source], 0, d_out, st)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert not got[:RECORDS[source] * 8].any() and np.array_equal(got[RECORDS[source] * 8:], poison[RECORDS[source] * 8:])
    assert st is None or all_zero(st)


@pytest.mark.parametrize("with_stats", [False, True])
def test_without_samples_a_row_list_is_not_looked_at(rt, box, with_stats):
    """rt_features_device at spp == 0: row ids out of range, or no row ids at all, and the zeros are written all the same."""
    import torch
    _, cam, _ = box
    d_bad = device_list("rows", rt, cam, bad=True)
    for ptr in (d_bad.data_ptr(), 0):
        poison, d_out = poisoned(RECORDS["rows"], 2)
        torch.cuda.synchronize()
        st = used_stats() if with_stats else None
        run("rows", rt, box, ptr, COUNT["rows"], 0, d_out, st)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert not got[:RECORDS["rows"] * 8].any() and np.array_equal(got[RECORDS["rows"] * 8:], poison[RECORDS["rows"] * 8:])
        assert st is None or all_zero(st)
    with pytest.raises(rt.RtError) as e:                                        # (with samples the same list is refused)
        run("rows", rt, box, d_bad.data_ptr(), COUNT["rows"], 2, d_out, None)
    assert e.value.code == F.RT_ERR_INVALID and str(e.value).endswith("rt_features_device: row id out of range")


@pytest.mark.parametrize("with_stats", [False, True])
def test_without_samples_a_pixel_list_is_still_checked(rt, box, with_stats):
    """rt_features_pixels_device at spp == 0: an id out of range refuses the call, and nothing has written the output."""
    import torch
    _, cam, _ = box
    d_bad = device_list("pixels", rt, cam, bad=True)
    poison, d_out = poisoned(RECORDS["pixels"], 3)
    torch.cuda.synchronize()
    st = used_stats() if with_stats else None
    with pytest.raises(rt.RtError) as e:
        run("pixels", rt, box, d_bad.data_ptr(), COUNT["pixels"], 0, d_out, st)
    assert e.value.code == F.RT_ERR_INVALID
    assert str(e.value).endswith("rt_features_pixels_device: pixel id out of range (>= width * height * n_frames)")
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), poison)                          # bit-unchanged
