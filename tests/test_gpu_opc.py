"""The correction loop on the GPU (correctLayout on the HIP path) against the CPU oracle run of tests/golden/g19_opc_loop.npz
(tests/golden/make_g19_opc_loop.py, checked again on the CPU in tests/test_opc_cpu.py): the layout and setup of
tests/opc_case.py at 128^2."""
import numpy as np
import pytest
import torch

import opc_case as C
from helpers import TOL_IMAGE_MAX

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def run(dev, golden):
    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat
    from lithographysimulator_amd import metrology
    g = golden("g19_opc_loop.npz")
    pupil = L.Pupil(C.PN, C.WAVELENGTH, C.NA, None, device=dev).generatePupilFunction()
    source = L.LightSource(C.SIGMA_IN, C.SIGMA_OUT, C.PN, C.NA, device=dev).generateAnnular()
    planned = []
    inner = metrology.measureEPE

    def spy(*a, **k):                                           # after every image: was the Abbe call planned from the record?
        planned.append(int(nat.last_plan()["planned_from_record"]))
        return inner(*a, **k)

    metrology.measureEPE = spy
    try:
        result = L.correctLayout(C.layout(), C.PN, C.PIXEL, C.ORIGIN, C.WAVELENGTH, pupil, source, float(g["threshold"]),
                                 spacing=C.SPACING, iterations=C.ITERATIONS, gain=C.GAIN, maxBias=C.MAX_BIAS,
                                 antialias=C.ANTIALIAS, searchRange=C.RANGE)
    finally:
        metrology.measureEPE = inner
    return dict(L=L, g=g, result=result, planned=planned, source=source)


def test_iteration_zero_matches_the_oracle_site_by_site(run):
    """No feedback yet, so the two loops measure the same layout: the images agree within TOL_IMAGE_MAX of the peak each
    (the parity the image tests hold), an edge moves by du / |du/dx| = du / (ils T) nm -- the derivation of
    test_subpixel_bossung_curves_are_consistent_with_the_pixel_table -- plus the fp32 position tolerance of test_gpu_epe
    (2^-22 (|t_k| + h cond) pixel, with the crossing's own t_k and cond from the fixture)."""
    g, res = run["g"], run["result"]
    assert np.array_equal(res.sites.sites_px, g["sites_px"]) and int(source_points(run)) == int(g["source_points"])
    T, ils = float(g["threshold"]), g["ils0_per_nm"]
    position = 2.0 ** -22 * (np.abs(g["tk0"]) + 0.5 * g["cond0"]) * C.PIXEL
    tol = 2 * TOL_IMAGE_MAX * float(g["peak0"]) * 1.0 / (ils * T) + position
    d = np.abs(res.epe_history[0] - g["epe0_nm"])
    print(f"iteration 0: worst |epe_gpu - epe_oracle| = {float(d.max()):.3e} nm = {float((d / tol).max()):.3f} of its bound "
          f"(bounds {float(tol.min()):.2e} .. {float(tol.max()):.2e} nm)")
    assert res.history[0][2] == 0 and (d <= tol).all(), (float(d.max()), float((d / tol).max()))
    assert float(tol.max()) < 0.05


def source_points(run):
    return int(torch.count_nonzero(run["source"]))


def test_loop_gains_what_the_oracle_loop_gains(run):
    """Later iterates may legitimately differ from the oracle's (a 1e-5 nm difference can move a sub-centre across an edge), so
    the path is not pinned: the best RMS must reach the geometric mean of the oracle loop's first and best RMS."""
    g, res = run["g"], run["result"]
    hist = g["history"]
    want = float(np.sqrt(hist[0, 0] * hist[int(g["best_iteration"]), 0]))
    print("GPU history (rms nm, max nm, NaN sites):", res.history, "oracle:", hist.tolist(), "asked:", want)
    assert len(res.history) == C.ITERATIONS
    assert res.history[res.best_iteration][0] <= want
    again = run["L"].biasLayout(C.layout(), res.sites, res.bias_nm)
    assert all(np.array_equal(a, b) for a, b in zip(res.polygons, again))


def test_plan_cache_is_in_use_from_the_second_image_on(run):
    planned = run["planned"]
    assert len(planned) == C.ITERATIONS
    assert all(p != 0 for p in planned[1:]), planned
