"""The device against the per-sample path reference of tests/brute_paths.py directly, not through the oracle: the scatter step,
light sampling, the mixture pdfs and the camera, which the kernels and the oracle share through rt_math.h and which parity
(HIP == oracle) therefore cannot hold.
  rt_radiance        every case of tests/path_cases.py at its depth, with and without RT_FLAG_COUNTERS, with the nearer child
                     first and in the reference's child order; two cases once more through a ring of one plane;
  rt_render          the camera cases on both engines; rt_render_pixels on 200 shuffled pixel ids.
The assertions are the CPU module's own (path_cases.hold) on the device's output; with counters, rng_draws is the reference's
word count over the compared and the left-out samples alike. Classes and tolerances: brute_paths' docstring."""
import numpy as np
import pytest

import path_cases as PC
import trace_scenes as T
from gpu_first import torch_first  # noqa: F401

pytestmark = pytest.mark.gpu

REF_ORDER = 1 << 15                                      # rt2022_debug.h: tuning bit 15, the reference's child order


def radiance(dev, c, counters):
    out = dev.radiance(c.rays, spp=PC.SPP, background=PC.BACKGROUND, t_min=0.001, max_depth=c.depth, want_stats=counters)
    return out if counters else (out, None)


@pytest.mark.parametrize("name", PC.NAMES)
def test_radiance_against_reference(rt, name):
    c = PC.reference(name)
    PC.check_floors(c)                                           # caps and floors, before the device is called
    dev = rt.DeviceScene(c.desc)
    for word in (T.TUNING, T.TUNING | REF_ORDER):
        dev.set_tuning(word)
        for counters in (False, True):
            out, st = radiance(dev, c, counters)
            PC.hold(c, out, "hip%s%s" % ("+c" if counters else "", "/ref" if word & REF_ORDER else ""), st.rng_draws if counters else None)
            if counters:
                assert st.paths == len(c.rays) * PC.SPP


@pytest.mark.parametrize("name", ["floor-three-lights", "glass-outside-3"])
def test_radiance_through_a_ring_of_one_plane(rt, name):
    c = PC.reference(name)
    dev = rt.DeviceScene(c.desc)
    dev.set_partial_ring(1)
    out, st = radiance(dev, c, True)
    PC.hold(c, out, "hip/ring", st.rng_draws)


@pytest.mark.parametrize("engine", ["wavefront", "mega"])
@pytest.mark.parametrize("name", PC.CAMERA_NAMES)
def test_camera_frames_against_reference(rt, name, engine):
    c = PC.camera_reference(name)
    PC.check_camera_floors(c)
    dev = rt.DeviceScene(c.desc)
    dev.set_engine(engine)
    rows = np.arange(PC.H, dtype=np.uint32)
    PC.hold(c, dev.render(c.cam, c.params, rows), "hip/" + engine)
    out, st = dev.render(c.cam, c.params, rows, want_stats=True)
    PC.hold(c, out, "hip+c/" + engine, st.rng_draws)


def test_pixel_list_against_reference(rt):
    c = PC.camera_reference("cam-floor-depth-2")
    dev = rt.DeviceScene(c.desc)
    ids = np.random.default_rng(11).permutation(PC.W * PC.H)[:200]
    out = dev.render_pixels(c.cam, c.params, rt.pixel_ids(0, ids // PC.W, ids % PC.W, PC.W, PC.H))
    listed = PC.Case()
    listed.name, listed.paths = c.name + " pixel list", c.paths
    listed.value, listed.tol, listed.keep = c.value[ids], c.tol[ids], c.keep[ids]
    assert listed.keep.sum() >= 180
    PC.hold(listed, out, "hip")
