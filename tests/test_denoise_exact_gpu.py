"""The denoiser kernels themselves (rt_denoise*, rt_denoise_dual*: dn_prepare, dn_atrous, dn_dual_prepare, dn_dual_prefilter,
dn_dual_atrous in csrc/hip/pt_denoise.hip and post_rows in pt_rows.hip) held to what shares no code with them: every value inside the 53-bit
interval enclosure of tests/denoise_exact.py, and every closed form and exact invariant of tests/denoise_cases.py — through
the host form, and through the device form on torch buffers. tests/test_denoise_ref.py holds the numpy restatements to the
same on the CPU, so two further shapes are compared with the restatements bit for bit, where the enclosure would be slow.

The enclosure cases on the device (denoise_cases.GPU_CASES): 12 x 9, 67 x 9 and 9 x 67 — a lane strip boundary in x, row
groups of 4 in y — default and tight sigmas, n_iter 1 and 5, var_iter 0 and 1, a shuffled row list. The intervals are
computed once per process (denoise_cases.enclosure)."""
import numpy as np
import pytest

import denoise_cases as DC
import denoise_dual_ref as RD
import denoise_ref as RS
from compare import assert_same_bits
from gpu_first import torch_first  # noqa: F401

pytestmark = pytest.mark.gpu

HOST, DEVICE = DC.Library(), DC.Device()


def held(name, filt):
    for what, width, off, outside in DC.against_enclosure(name, filt):
        print("%s, %s, %s: relative width %.3g, off the middle by %.3g half-widths" % (filt.name, name, what, width, off))
        assert width <= DC.WIDTH_CAP, (name, what, width)
        assert outside == 0, (filt.name, name, what, outside, off)


def test_the_device_cases_cover_what_they_are_meant_to():
    cases = [DC.CASES[c] for c in DC.GPU_CASES]
    assert {c[1:3] for c in cases} == {(12, 9), (67, 9), (9, 67)}
    for which in ("single", "dual"):
        mine = [c for c in cases if c[0] == which]
        assert {c[4]["n_iter"] for c in mine} == {1, 5} and any(c[5] for c in mine)
        assert any("sigma_albedo" in c[4] for c in mine) and any("sigma_albedo" not in c[4] for c in mine)
    assert {c[4]["var_iter"] for c in cases if c[0] == "dual"} == {0, 1}


@pytest.mark.parametrize("name", DC.GPU_CASES)
def test_library_inside_the_enclosure(name):
    held(name, HOST)


@pytest.mark.parametrize("name", ["single 9x67 n5 tight rows", "dual 9x67 n5 v0 tight rows", "dual 67x9 n5 v1"])
def test_device_form_inside_the_enclosure(name):
    held(name, DEVICE)


# ---- every closed form and invariant on the device --------------------------------------------------------------------------
FORMS = {"%s, %s" % (w, n): f for n, w, f in DC.closed_forms()}


@pytest.mark.parametrize("name", list(FORMS))
def test_closed_form_holds_for_the_library(name):
    FORMS[name](HOST)


@pytest.mark.parametrize("name", ["single, two scales", "single, impulse, n_iter 3", "single, edge stop, albedo", "single, fixed point, n_iter 6",
                                  "dual, two regions, one step", "dual, variance propagation, n_iter 3", "dual, invariants",
                                  "dual, impulse at the borders"])
def test_closed_form_holds_for_the_device_form(name):
    FORMS[name](DEVICE)


# ---- two shapes the other GPU modules do not have, against the restatements bit for bit -------------------------------------
# 65 x 67 at n_iter = 5 is the smallest image in which a pixel (32, 32 .. 34) has all 25 taps at step 16 inside, in both
# directions; 131 x 9 at n_iter = 7 has taps one and two 64-column strips away, at steps 32 and 64.
LARGE_STEPS = [(65, 67, 5), (131, 9, 7)]


@pytest.mark.parametrize("W, H, n_iter", LARGE_STEPS)
def test_large_steps_single(rt, W, H, n_iter):
    sums, feat = RS.buffers(W, H, seed=W + H, hostile=True, nan_albedo=False)
    prm = dict(DC.SINGLE, n_iter=n_iter)
    ref = DC.Restated().single(sums, DC.unpack(feat), prm)
    assert np.isfinite(ref).all()
    for filt in (HOST, DEVICE):
        assert_same_bits(filt.single(sums, DC.unpack(feat), prm), ref, (filt.name, W, H))


@pytest.mark.parametrize("var_iter", [1, 3])
@pytest.mark.parametrize("W, H, n_iter", LARGE_STEPS)
def test_large_steps_dual(rt, W, H, n_iter, var_iter):
    h = RD.halves(W, H, seed=W + H, hostile=True, nan_albedo=False)
    ga, gb = DC.unpack(h[2]), DC.unpack(h[3])
    prm = dict(DC.DUAL, n_iter=n_iter, var_iter=var_iter)
    ref = DC.Restated().dual(h[0], h[1], ga, gb, prm)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    for filt in (HOST, DEVICE):
        got = filt.dual(h[0], h[1], ga, gb, prm)
        assert_same_bits(got[0], ref[0], (filt.name, W, H))
        assert_same_bits(got[1], ref[1], (filt.name, W, H, "variance"))
