"""The HIP path's radiance against closed forms (tests/radiometry_cases.py): every case A-G through rt_radiance at N = 2^24
samples in one call (4096 rays x 4096 spp, batch means per ray), case H through rt_render at 64 x 48 x 4096 spp, and case C
once more through rt_render on the megakernel engine (rt_radiance refuses that engine: a camera so narrow that every pixel
looks at P's neighbourhood stands in for the ray). The criterion is the one of the CPU module, tests/test_radiometry.py.

Detection floor: se / L at 2^24 is 0.5e-4 (glass at 0 degrees) to 4.8e-4 (medium chord), so a relative bias of 8 se / L —
0.04 % to 0.4 % — fails with probability 0.98; the resolution cap keeps a noisier run from passing.
Not pinned here: bits (tests/test_radiance.py does that, against the oracle), variance, textures and the BVH code."""
import numpy as np
import pytest

import radiometry_cases as RC
from compare import same_bits
from gpu_first import torch_first  # noqa: F401

pytestmark = pytest.mark.gpu

N_RAYS, SPP = 4096, 4096


_sums = {}


def device_sums(rt, name):
    if name not in _sums:
        case = RC.CASES[name]
        _, desc = case["scene"](rt)
        dev = rt.DeviceScene(desc)
        _sums[name] = dev.radiance(RC.case_rays(rt, case, N_RAYS, RC.SEED_GPU), spp=SPP, background=tuple(case["background"]),
                                   max_depth=case["depth"])
        _sums[name].setflags(write=False)
        dev.close()
    return _sums[name]


@pytest.mark.parametrize("name", list(RC.CASES))
def test_case_on_the_device(rt, name):
    RC.check(name, device_sums(rt, name), SPP, cap=RC.SE_REL[name][24], tag="gpu")


def test_rect_light_depth_2_and_50_are_the_same_paths(rt):
    assert same_bits(device_sums(rt, "A_rect_d2"), device_sums(rt, "A_rect_d50"))


@pytest.mark.parametrize("aperture", RC.H_APERTURES)
def test_camera_on_the_device(rt, aperture):
    _, desc = RC.camera_scene(rt)
    dev = rt.DeviceScene(desc)
    p = rt.make_params(RC.H_W, RC.H_H, SPP, 50, (0, 0, 0), seed=RC.SEED_GPU)
    sums = dev.render(RC.camera(rt, aperture), p, np.arange(RC.H_H))
    RC.check_camera(sums, SPP, cap=RC.H_SE_REL[aperture][SPP], tag="gpu  H_camera_ap%.1f" % aperture)


@pytest.mark.parametrize("engine", ["mega", "wavefront"])
def test_case_C_through_the_narrow_camera(rt, engine):
    """64 x 64 pixels x 4096 spp = 2^24 samples, batch means per pixel. tests/test_radiometry.py bounds what the pixels'
    different floor points do to the closed form: less than a hundredth of se."""
    _, desc = RC.CASES["C_two_lights_bg"]["scene"](rt)
    dev = rt.DeviceScene(desc)
    dev.set_engine(engine)
    p = rt.make_params(RC.C_CAM_W, RC.C_CAM_H, SPP, 2, tuple(RC.BG_C), seed=RC.SEED_GPU)
    sums = dev.render(RC.narrow_camera(rt), p, np.arange(RC.C_CAM_H))
    RC.check("C_two_lights_bg", sums.reshape(-1, 3), SPP, cap=RC.C_CAM_SE_REL[SPP], tag="gpu camera, %s" % engine)
