"""The correction loop (correctLayout) on the CPU oracle chain: coverage_oracle -> abbe_oracle -> epe_oracle on the
six-polygon layout of tests/opc_case.py, antialias 16, six iterations, circular sigma 0.5 (797 source points: the run
takes about 5 s).  tests/golden/g19_opc_loop.npz (tests/golden/make_g19_opc_loop.py) holds this run; the GPU loop is checked
against it in tests/test_gpu_opc.py."""
import numpy as np
import pytest

import opc_case as C
from helpers import TOL_IMAGE_MAX


@pytest.fixture(scope="module")
def run():
    import lithographysimulator_amd as L
    model = C.OracleModel()
    threshold = C.THRESHOLD_FRACTION * model.clear
    polygons = C.layout()
    sites = L.layoutSites(polygons, C.SPACING, C.PIXEL, C.ORIGIN, C.PN, C.WAVELENGTH)
    seen = []

    def imager(polys):
        seen.append([q.copy() for q in polys])
        return model.imager(polys)

    result = L.correctLayout(polygons, C.PN, C.PIXEL, C.ORIGIN, C.WAVELENGTH, None, None, threshold, spacing=C.SPACING,
                             iterations=C.ITERATIONS, gain=C.GAIN, maxBias=C.MAX_BIAS, imager=imager,
                             epe=model.epe_at(sites.sites_px, threshold))
    return dict(L=L, model=model, threshold=threshold, polygons=polygons, sites=sites, seen=seen, result=result)


def test_loop_reduces_the_epe_on_the_oracle_chain(run):
    res, seen = run["result"], run["seen"]
    hist = np.array(res.history)
    print("history (rms nm, max nm, NaN sites):", res.history)
    assert hist.shape == (C.ITERATIONS, 3) and len(seen) == C.ITERATIONS and len(res.epe_history) == C.ITERATIONS
    assert hist[0, 2] == 0                                        # every site finds the printed edge of the uncorrected layout
    best = int(res.best_iteration)
    assert best > 0 and hist[best, 0] < hist[0, 0]
    assert hist[best, 0] == hist[hist[:, 2] == hist[:, 2].min(), 0].min()
    # result.polygons is the iterate the history names, and bias_nm the biases that made it
    assert len(res.polygons) == len(seen[best]) and all(np.array_equal(a, b) for a, b in zip(res.polygons, seen[best]))
    again = run["L"].biasLayout(run["polygons"], res.sites, res.bias_nm)
    assert all(np.array_equal(a, b) for a, b in zip(res.polygons, again))
    assert np.array_equal(res.epe_nm, res.epe_history[best])
    assert np.abs(res.bias_nm).max() <= C.MAX_BIAS and np.array_equal(res.sites.sites_px, run["sites"].sites_px)
    # iteration 0 is the target itself
    assert all(np.array_equal(np.sort(a, axis=0), np.sort(b, axis=0)) for a, b in zip(seen[0], run["polygons"]))
    # the loop's first step is the feedback rule
    first = np.clip(-C.GAIN * res.epe_history[0], -C.MAX_BIAS, C.MAX_BIAS)
    assert all(np.array_equal(a, b) for a, b in zip(seen[1], run["L"].biasLayout(run["polygons"], res.sites, first)))


def test_fixture_holds_this_run(run, golden):
    """The fixture's case is this one, and its iteration 0 -- before any feedback, so comparable site by site -- agrees within
    what two fp32 evaluations of the image may differ by: 2 TOL_IMAGE_MAX peak / (ils T) nm (an edge moves by du / |du/dx|).
    Later iterates may part ways (a 1e-5 nm difference can move a sub-centre across an edge): the geometric mean of the first
    and the best RMS is asked of them, as of the GPU loop."""
    g = golden("g19_opc_loop.npz")
    res = run["result"]
    assert np.array_equal(g["sites_px"], run["sites"].sites_px)
    assert np.array_equal(g["polygon_vertices"], np.concatenate(run["polygons"]))
    assert float(g["threshold"]) == pytest.approx(run["threshold"], rel=1e-5)
    tol = 2 * TOL_IMAGE_MAX * float(g["peak0"]) / (g["ils0_per_nm"] * float(g["threshold"]))
    assert np.isfinite(g["epe0_nm"]).all() and float(tol.max()) < 0.05
    assert (np.abs(res.epe_history[0] - g["epe0_nm"]) <= tol).all()
    hist = g["history"]
    assert res.history[res.best_iteration][0] <= np.sqrt(hist[0, 0] * hist[int(g["best_iteration"]), 0])


def test_loop_arguments_and_the_nan_rule():
    import lithographysimulator_amd as L
    polys = [C.rect(100.0, 100.0, 300.0, 300.0)]
    kw = dict(spacing=100.0, maxBias=30.0, iterations=3)
    with pytest.raises(ValueError):
        L.correctLayout(polys, 32, 25.0, (0.0, 0.0), 193.0, None, None, 1.0, imager=lambda p: None, **kw)       # imager without epe
    with pytest.raises(ValueError):
        L.correctLayout([np.array([[0.0, 0.0], [300.0, 0.0], [0.0, 300.0]])], 32, 25.0, (0.0, 0.0), 193.0, None, None, 1.0,
                        imager=lambda p: None, epe=lambda i: np.zeros(3), **kw)                                   # not Manhattan
    with pytest.raises(ValueError):
        L.correctLayout(polys, 32, 25.0, (0.0, 0.0), 193.0, None, None, 1.0, imager=lambda p: p, epe=lambda p: np.zeros(8),
                        exposed=False, **kw)                                                                     # not defined yet
    # nothing printed anywhere: every bias grows by maxBias / 6 per iteration; the first iterate stays the best
    res = L.correctLayout(polys, 32, 25.0, (0.0, 0.0), 193.0, None, None, 1.0, imager=lambda p: p,
                          epe=lambda p: np.full(8, np.nan), **kw)
    assert [h[2] for h in res.history] == [8, 8, 8] and res.best_iteration == 0 and not res.bias_nm.any()
    # a model that prints every edge 4 nm short of where the mask has it: the bias converges to +4
    def epe(p):
        return (p[0][:, 0].max() - p[0][:, 0].min() - 200.0) / 2.0 - 4.0 + np.zeros(8)
    res = L.correctLayout(polys, 32, 25.0, (0.0, 0.0), 193.0, None, None, 1.0, imager=lambda p: p, epe=epe, spacing=100.0,
                          maxBias=30.0, iterations=12, gain=0.6)
    assert res.history[0][0] == 4.0 and res.history[-1][0] < 1e-3 and np.allclose(res.bias_nm, 4.0, atol=1e-2)
