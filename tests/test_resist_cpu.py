"""The CPU restatement of the resist model (tests/resist_oracle.py) pinned by closed-form cases, and the argument checks of
the Python layer and the C entries that need no device."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import resist_oracle as RO
from helpers import ROOT


# ---- diffuse()
@pytest.mark.parametrize("sigma", [0.4, 1.2, 3.0, 8.0])
def test_unit_impulse_diffuses_to_the_outer_product_of_the_taps(sigma):
    g = RO.taps(sigma)
    R = RO.radius(sigma)
    assert R == math.ceil(4 * sigma) and len(g) == 2 * R + 1
    assert abs(g.sum() - 1.0) < (2 * R + 1) * 2.0 ** -25 and np.array_equal(g, g[::-1])      # fp32-rounded, symmetric
    assert np.array_equal(g, g.astype(np.float32).astype(np.float64))
    n = 2 * R + 9
    img = np.zeros((n, n))
    img[R + 3, R + 5] = 1.0
    D = RO.diffuse(img, sigma)
    expect = np.zeros((n, n))
    expect[3: 3 + 2 * R + 1, 5: 5 + 2 * R + 1] = np.outer(g, g)
    assert np.array_equal(D, expect)


def test_sigma_zero_is_the_identity_and_limits_raise():
    rng = np.random.default_rng(1)
    img = rng.random((3, 17, 17)).astype(np.float32)
    assert np.array_equal(RO.diffuse(img, 0.0), img.astype(np.float64))
    assert RO.radius(8.0) == 32
    for bad in (8.01, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            RO.taps(bad)


def test_interior_image_keeps_its_sum_and_stacks_are_plane_by_plane():
    rng = np.random.default_rng(2)
    sigma, R = 1.2, 5
    img = np.zeros((2, 40, 40))
    img[:, R: 40 - R, R: 40 - R] = rng.random((2, 40 - 2 * R, 40 - 2 * R))
    D = RO.diffuse(img, sigma)
    s = RO.taps(sigma).sum() ** 2
    assert np.allclose(D.sum((1, 2)), img.sum((1, 2)) * s, rtol=1e-13, atol=0)
    assert np.array_equal(D[1], RO.diffuse(img[1], sigma))


def test_constant_image_falls_off_at_the_border_as_the_cumulative_tap_sums():
    sigma = 1.2
    g, R = RO.taps(sigma), RO.radius(sigma)
    n = 4 * R
    D = RO.diffuse(np.ones((n, n)), sigma)
    # zero extension: pixel x sees the taps k >= -x; from x = R on, all of them
    edge = np.array([g[R - min(x, R):].sum() for x in range(n)])
    edge = np.minimum(edge, edge[::-1])
    assert np.allclose(D, np.outer(edge, edge), rtol=1e-14, atol=0)
    assert abs(D[n // 2, n // 2] - g.sum() ** 2) < 1e-15
    assert abs(D[0, 0] - ((g.sum() + g[R]) / 2.0) ** 2) < 1e-15                      # the corner sees half the taps + the centre one


# ---- measure_cd()
def test_v_profile_measures_the_closed_form_crossings():
    n, a, x0, T, ps = 48, 0.5, 20.25, 3.0, 25.0
    v = (a * np.abs(np.arange(n) - x0)).astype(np.float32)              # multiples of 1/8: exact in fp32
    cd, x_lo, x_hi, ils_lo, ils_hi, lo, hi, _, _ = RO.measure_line(v, 20, 1.0, T, False, ps)
    assert (x_lo, x_hi) == (x0 - T / a, x0 + T / a) == (14.25, 26.25) and cd == 12.0 * ps
    assert (lo, hi) == (15, 26) and ils_lo == ils_hi == a / (T * ps)
    # the same feature seen with twice the gain and twice the threshold
    assert RO.measure_line(v, 23, 2.0, 2 * T, False, ps)[:3] == (cd, x_lo, x_hi)
    # the exposed side: from the crossing to the right-hand border
    cd_r, xl_r, xh_r, il_r, ih_r, lo_r, hi_r, _, _ = RO.measure_line(v, 40, 1.0, T, True, ps)
    assert (xl_r, xh_r, lo_r, hi_r) == (26.25, n - 0.5, 27, n - 1) and math.isnan(ih_r) and il_r == a / (T * ps)
    # along a column of an image, through measure_cd
    img = np.zeros((2, n, n), dtype=np.float32)
    img[1] = v[:, None]
    table, runs, _ = RO.measure_cd(img, [(20, 7, 1), (7, 20, 0), (n, 0, 0), (0, -1, 1), (3, 3, 2)], [1.0], T, False, ps)
    assert tuple(table[0, 1, 0, :3]) == (12.0 * ps, 14.25, 26.25) and tuple(runs[0, 1, 0]) == (15, 26)
    assert table[0, 1, 1, 0] == 0.0 and np.isnan(table[0, 1, 1, 1:]).all()          # the row is constant 6.125 >= T: not inside
    assert table[0, 0, 0, 0] == n * ps                                               # plane 0 is all zero: inside everywhere
    assert np.isnan(table[0, :, 2:]).all()                                           # gauges outside the grid / bad axis


def test_other_kind_at_the_gauge_gives_zero_and_a_full_run_gives_n_pixels():
    v = np.array([0, 0, 5, 5, 5, 0, 0], dtype=np.float32)
    res = RO.measure_line(v, 3, 1.0, 2.5, False, 10.0)
    assert res[0] == 0.0 and all(math.isnan(t) for t in res[1:5])
    cd, x_lo, x_hi = RO.measure_line(v, 3, 1.0, 2.5, True, 10.0)[:3]
    assert (x_lo, x_hi, cd) == (1.5, 4.5, 30.0)
    full = RO.measure_line(v, 3, 1.0, 9.0, False, 10.0)
    assert full[:3] == (70.0, -0.5, 6.5) and math.isnan(full[3]) and math.isnan(full[4]) and full[5:7] == (0, 6)


def test_subpixel_cd_is_within_one_pixel_of_the_pixel_count_on_random_lines():
    rng = np.random.default_rng(5)
    seen = 0
    for trial in range(300):
        n = int(rng.integers(3, 90))
        v = np.convolve(rng.random(n + 8), np.ones(9) / 9.0, mode="valid").astype(np.float32)      # smooth-ish, n samples
        T, gain, c = float(rng.uniform(0.35, 0.65)), float(rng.uniform(0.8, 1.25)), int(rng.integers(0, n))
        for exposed in (False, True):
            cd, x_lo, x_hi, _, _, lo, hi, _, _ = RO.measure_line(v, c, gain, T, exposed, 1.0)
            mask = RO.contour(v, gain, T) == (1 if exposed else 0)
            if cd == 0.0:
                assert not mask[c]
                continue
            seen += 1
            assert mask[lo: hi + 1].all() and (lo == 0 or not mask[lo - 1]) and (hi == n - 1 or not mask[hi + 1])
            assert lo <= c <= hi and abs(cd - (hi - lo + 1)) <= 1.0
            assert lo - 1 <= x_lo <= lo and hi <= x_hi <= hi + 1
    assert seen > 200


# ---- the Python layer and the C entries: argument checks that need no device
@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", ROOT, "-j", "8", "all"])
    return _native


def test_python_argument_checks_need_no_device(nat):
    import lithographysimulator_amd as L
    raw = torch.zeros(2, 64, 64)
    with pytest.raises(ValueError, match="pixelSize"):
        L.resistContour(raw, 1.0, 0.5, diffusionLength=30.0)
    for bad in (-1.0, float("nan"), float("inf"), 201.0):
        with pytest.raises(ValueError):
            L.resistContour(raw, 1.0, 0.5, diffusionLength=bad, pixelSize=25)
        with pytest.raises(ValueError):
            L.bossungCurves(raw, 1.0, 0.5, [1.0], 25, subpixel=True, diffusionLength=bad)
    with pytest.raises(ValueError):
        L.resistContour(raw, 1.0, 0.5, diffusionLength=30.0, pixelSize=0)
    with pytest.raises(L.imageformation.ShapeError):
        L.bossungCurves(raw[0], 1.0, 0.5, [1.0], 25, subpixel=True)
    img = torch.zeros(2, 16, 16)
    S = L.imageformation.ShapeError
    for image, gauges, doses in ((img.double(), [(1, 1, 0)], (1.0,)), (torch.zeros(16), [(1, 1, 0)], (1.0,)),
                                 (torch.zeros(2, 16, 8), [(1, 1, 0)], (1.0,)), (img, [(1, 1)], (1.0,)), (img, [], (1.0,)),
                                 (img, torch.zeros(1, 3), (1.0,)), (img, [(1, 1, 0)], ()), (img, [(1, 1, 0)], [1.0] * 65)):
        with pytest.raises(S):
            L.measureCD(image, 0.5, gauges, 25, doses=doses)
    with pytest.raises(ValueError):
        L.measureCD(img, 0.5, [(1, 1, 0)], 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                       # all checks passed: now it wants the device
        L.measureCD(img, 0.5, [(1, 1, 0)], 25)
    assert "measureCD" in L.__all__


def test_c_entries_reject_bad_arguments_before_any_gpu_work(nat):
    lib = nat.lib()
    p = ctypes.c_void_p(8)                                                            # never dereferenced: every call fails first
    f = lib.litho_postprocess_resist_diffused
    assert f(p, 1, 64, 1.0, 1.0, 0.5, 1.2, None, None, None) == nat.E_ARG             # both outputs NULL
    assert f(None, 1, 64, 1.0, 1.0, 0.5, 1.2, p, p, None) == nat.E_ARG
    for sigma in (-0.5, float("nan"), float("inf"), 8.01, 8.25):                      # 8.01: R = 33
        assert f(p, 1, 64, 1.0, 1.0, 0.5, sigma, p, p, None) == nat.E_ARG
    assert f(p, 0, 64, 1.0, 1.0, 0.5, 1.2, p, p, None) == nat.E_ARG
    assert f(p, 1, 64, 1.0, float("nan"), 0.5, 1.2, p, p, None) == nat.E_ARG
    assert f(p, 1, 64, 1.0, 1.0, float("nan"), 1.2, p, p, None) == nat.E_ARG
    m = lib.litho_measure_cd
    gains = (ctypes.c_float * 65)(*([1.0] * 65))
    assert m(p, 1, 64, p, 1, gains, 65, 0.5, 0, 25.0, p, None) == nat.E_ARG           # more than 64 gains
    assert m(p, 1, 64, p, 1, gains, 0, 0.5, 0, 25.0, p, None) == nat.E_ARG
    assert m(p, 1, 64, p, 0, gains, 1, 0.5, 0, 25.0, p, None) == nat.E_ARG
    assert m(p, 1, 64, p, 1, None, 1, 0.5, 0, 25.0, p, None) == nat.E_ARG
    assert m(None, 1, 64, p, 1, gains, 1, 0.5, 0, 25.0, p, None) == nat.E_ARG
    assert m(p, 1, 64, p, 1, gains, 1, 0.5, 0, 25.0, None, None) == nat.E_ARG
    assert m(p, 1, 64, p, 1, gains, 1, float("nan"), 0, 25.0, p, None) == nat.E_ARG
    assert m(p, 1, 64, p, 1, gains, 1, 0.5, 0, 0.0, p, None) == nat.E_ARG
    gains[0] = float("nan")
    assert m(p, 1, 64, p, 1, gains, 1, 0.5, 0, 25.0, p, None) == nat.E_ARG
