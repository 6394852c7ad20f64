"""Tiled imaging on the host (lithographysimulator_amd/tiling.py): the plan's geometry, the site map of the stitched image, the
float64 restatement of the driver (tests/tiling_oracle.py) against the single-window oracle, and the halo condition measured on
that oracle alone.  No GPU.

Halo condition (epsilon = 1: pixelSize 193 / 8 nm, pn 64, the 16 strided points of the 0.4-0.8 annulus at full rank under the demo
aberrations, 40 seeded rectangles on 192^2 pixels): the discrepancy d(halo) is the largest difference, relative to the image's
maximum, between the tiling on the lattice of the bounds' corner and the tiling whose lattice is shifted by half a core.  Observed
here: d(4) = 0.1151, d(20) = 0.0177 (printed by the test; LABNOTES.md).  The test asserts d(20) < d(4) / 2 and nothing finer: the
fall is not monotone halo by halo."""
import math

import numpy as np
import pytest
import torch

import socs_oracle as SO
import tiling_oracle as TO
from helpers import DEMO_AB, NA, WL, f16
from oracle import abbe_oracle as O

PS_EPS1 = 193.0 / 8.0


@pytest.fixture(scope="module")
def L():
    import lithographysimulator_amd as L
    return L


PLAN_SWEEP = [(pn, halo, ps) for pn in (32, 64, 128, 256) for ps in (25.0, PS_EPS1) for halo in (pn // 16 + 2, pn // 4, pn // 2 - 1)]


@pytest.mark.parametrize("pn,halo,ps", PLAN_SWEEP)
def test_plan_properties(L, pn, halo, ps):
    core = pn - 2 * halo
    for wx, wy, shift in ((2.3 * core + 0.4, 1.1 * core + 0.7, None), (0.5 * core, 3.0 * core, None), (1.7 * core, 1.2 * core, (0.37, 0.61))):
        bounds = (100.0, -250.0, 100.0 + wx * ps, -250.0 + wy * ps)
        origin = None if shift is None else (bounds[0] - shift[0] * core * ps, bounds[1] - shift[1] * core * ps)
        p = L.planTiles(bounds, pn, ps, WL, halo, origin)
        lo, hi = L.tileValidRegion(pn, ps, WL)
        n_out, scale, offset = L.metrology._registration(pn, ps, WL)
        assert scale == 1.0 and p.core == core and p.n == core * max(p.nx, p.ny) and p.count == p.nx * p.ny and p.n_tile == n_out
        assert lo <= p.j0 and p.j0 + core <= hi and 0 <= lo < hi <= n_out
        assert p.j0 == halo + math.floor(offset) and 0.0 <= p.offset_px < 1.0 and abs(p.offset_px - (offset - math.floor(offset))) < 1e-12
        # every pixel of the bounds lies in exactly one core: count the covers on the stitched raster
        cover = np.zeros((p.n, p.n), dtype=np.int32)
        for r0, c0 in p.place.tolist():
            cover[r0:r0 + core, c0:c0 + core] += 1
        gx0, gx1 = math.floor((bounds[0] - p.origin[0]) / ps), math.ceil((bounds[2] - p.origin[0]) / ps)
        gy0, gy1 = math.floor((bounds[1] - p.origin[1]) / ps), math.ceil((bounds[3] - p.origin[1]) / ps)
        assert 0 <= gx0 < core and 0 <= gy0 < core and gx1 <= p.nx * core and gy1 <= p.ny * core       # tile (0, 0) holds the first pixel
        assert gx1 > (p.nx - 1) * core and gy1 > (p.ny - 1) * core                                     # and no tile is idle
        assert (cover[gy0:gy1, gx0:gx1] == 1).all() and cover.max() == 1
        # windows, placements and neighbours say the same thing
        for t in range(p.count):
            iy, ix = divmod(t, p.nx)
            assert p.place[t].tolist() == [iy * core, ix * core]
            want = (p.origin[0] + (ix * core - halo) * ps, p.origin[1] + (iy * core - halo) * ps)
            assert np.allclose(p.windows_nm[t], want, rtol=0, atol=1e-9)
            assert p.neighbours[t].tolist() == [t + 1 if ix + 1 < p.nx else -1, t + p.nx if iy + 1 < p.ny else -1]
        if shift is not None:                                   # the lattice is the caller's
            assert abs((p.origin[0] - origin[0]) / (core * ps) - round((p.origin[0] - origin[0]) / (core * ps))) < 1e-9


def test_plan_errors(L):
    ok = (0.0, 0.0, 3000.0, 2000.0)
    with pytest.raises(ValueError):
        L.planTiles(ok, 64, 25.0, WL, 32)                       # core 0
    with pytest.raises(ValueError):
        L.planTiles(ok, 64, 25.0, WL, 40)                       # core < 0
    with pytest.raises(ValueError):
        L.planTiles(ok, 64, 25.0, WL, 1)                        # the core reaches into the padded pixels [62, 64)
    with pytest.raises(ValueError):
        L.planTiles(ok, 64, 25.0, WL, 0)
    assert L.planTiles(ok, 64, PS_EPS1, WL, 0).core == 64       # epsilon 1: nothing is padded
    for bad in ((0.0, 0.0, float("nan"), 1.0), (0.0, 0.0, float("inf"), 1.0), (0.0, 0.0, 0.0, 10.0), (5.0, 0.0, 1.0, 10.0)):
        with pytest.raises(ValueError):
            L.planTiles(bad, 64, 25.0, WL, 14)
    with pytest.raises(ValueError):
        L.tileValidRegion(128, 48.0, WL)                        # the copy case of _registration: scale != 1
    with pytest.raises(ValueError):
        L.planTiles(ok, 128, 48.0, WL, 32)
    assert L.tileValidRegion(64, 25.0, WL) == (1, 62) and L.tileValidRegion(64, PS_EPS1, WL) == (0, 64)


def _kernels(pn=64, points=16):
    P = O.pupil_function(f16(DEMO_AB), pn, NA, WL)
    W = SO.strided_points(O.source_annular(0.4, 0.8, pn), points)
    phi, lam = SO.exact_kernels(P.numpy(), W.numpy())
    assert phi.shape[0] == points
    return torch.from_numpy(phi)


@pytest.mark.parametrize("ps", [25.0, PS_EPS1])
def test_one_tile_plan_is_the_single_window(L, ps):
    pn, halo = 64, 14
    core = pn - 2 * halo
    rects = TO.rectangles(3, 8, core)
    plan = L.planTiles((0.0, 0.0, core * ps, core * ps), pn, ps, WL, halo)
    assert plan.count == 1 and plan.n == core
    kernels = _kernels()[:4]
    image, seam, err, _ = TO.tiled_image(rects, kernels, plan)
    single = TO.window_image(rects, kernels, pn, ps, WL, (-4 * halo, -4 * halo))
    assert np.array_equal(image, single[:, plan.j0:plan.j0 + core, plan.j0:plan.j0 + core]) and image.max() > 0
    assert np.isnan(seam).all() and math.isnan(err)


@pytest.mark.parametrize("ps", [25.0, PS_EPS1])
def test_sites_of_the_stitched_image(L, ps):
    """A tile's own layoutSites on its own window, moved by the tile's placement, are the stitched image's sites."""
    pn, halo = 64, 14
    core = pn - 2 * halo
    rects = TO.rectangles(5, 12, 3 * core)
    polys = TO.polygons_nm(rects, ps, (40.0, -70.0))
    plan = L.planTiles((40.0, -70.0, 40.0 + 3 * core * ps, -70.0 + 2 * core * ps), pn, ps, WL, halo)
    assert (plan.nx, plan.ny) == (3, 2)
    tiled = L.TiledImage(None, plan, None, float("nan"))
    all_sites = tiled.sites(polys, 60.0)
    seen = 0
    for t in range(plan.count):
        own = L.layoutSites(polys, 60.0, ps, tuple(plan.windows_nm[t]), pn, WL)
        assert np.array_equal(own.xy_nm, all_sites.xy_nm)
        moved = own.sites_px[:, :2].astype(np.float64) - plan.j0 + plan.place[t][::-1]
        r0, c0 = plan.place[t]
        inside = (moved[:, 0] >= c0) & (moved[:, 0] < c0 + core) & (moved[:, 1] >= r0) & (moved[:, 1] < r0 + core)
        seen += int(inside.sum())
        # fp32 sites below 256 pixels: half an ulp is 1.5e-5, two roundings and the float64 arithmetic stay below 1e-4
        assert np.abs(moved[inside] - all_sites.sites_px[inside, :2]).max() < 1e-4
        assert np.array_equal(own.sites_px[:, 2:], all_sites.sites_px[:, 2:])
    assert seen > 20
    back = tiled.toLayout([all_sites.sites_px[:, :2]])[0]
    assert np.abs(back - all_sites.xy_nm).max() < 1e-4 * ps * 4


@pytest.mark.parametrize("pn,ps", [(64, 25.0), (64, PS_EPS1), (128, 48.0), (32, 25.0)])
def test_layout_sites_default_is_unchanged(L, pn, ps):
    polys = TO.polygons_nm(TO.rectangles(7, 6, pn), ps, (10.0, 20.0))
    origin = (3.0, -8.0)
    s = L.layoutSites(polys, 90.0, ps, origin, pn, WL)
    n_out, scale, offset = L.metrology._registration(pn, ps, WL)
    px = np.empty((len(s), 2), dtype=np.float32)
    px[:, 0] = ((s.xy_nm[:, 0] - origin[0]) / ps - 0.5) * scale + offset
    px[:, 1] = ((s.xy_nm[:, 1] - origin[1]) / ps - 0.5) * scale + offset
    assert len(s) > 0 and np.array_equal(s.sites_px[:, :2], px)
    same = L.layoutSites(polys, 90.0, ps, origin, pn, WL, registration=(n_out, scale, offset))
    assert np.array_equal(same.sites_px, s.sites_px)
    other = L.layoutSites(polys, 90.0, ps, origin, pn, WL, registration=(n_out, 1.0, 0.25))
    assert np.array_equal(other.sites_px[:, 0], (((s.xy_nm[:, 0] - origin[0]) / ps - 0.5) + 0.25).astype(np.float32))


def _discrepancy(L, rects, kernels, halo, extent=192, pn=64, ps=PS_EPS1):
    core = pn - 2 * halo
    half = core // 2
    bounds = (0.0, 0.0, extent * ps, extent * ps)
    a = L.planTiles(bounds, pn, ps, WL, halo)
    b = L.planTiles(bounds, pn, ps, WL, halo, origin=(-half * ps, -half * ps))
    assert a.offset_px == 0.0 and b.offset_px == 0.0 and abs(b.origin[0] + half * ps) < 1e-9
    img_a = TO.tiled_image(rects, kernels, a)[0]
    img_b = TO.tiled_image(rects + 4 * half, kernels, b)[0]
    da, db = img_a[0, :extent, :extent], img_b[0, half:half + extent, half:half + extent]
    return float(np.abs(da - db).max() / da.max())


def test_halo_condition_on_the_oracle(L):
    rects = TO.rectangles(11, 40, 192)
    kernels = _kernels()
    d4, d20 = _discrepancy(L, rects, kernels, 4), _discrepancy(L, rects, kernels, 20)
    print(f"two tilings of one layout, epsilon 1, pn 64, 192^2: discrepancy / max at halo 4 {d4:.4f}, at halo 20 {d20:.4f}")
    assert d20 < d4 / 2
