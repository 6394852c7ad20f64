"""Edge placement error, the part that needs no GPU: the CPU restatement tests/epe_oracle.py against closed forms, the site
and bias geometry of lithographysimulator_amd.metrology, and the registration of the image grid against the mask raster on
the oracle chain."""
import math

import numpy as np
import pytest

import epe_oracle as EO
import opc_case as C
from oracle import layout_oracle as LO

PS = 25.0
U = 2.0 ** -24


# ---- the restatement on a plane: the bilinear interpolant of a plane is the plane
def plane(n, a, b, c):
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    return (a * x + b * y + c).astype(np.float32)


def test_crossing_on_a_dyadic_plane_is_analytic():
    n, a, b, c, T = 64, -0.25, 0.125, 12.0, 5.0                  # every sample below is exact in fp32
    img = plane(n, a, b, c)
    x, y = 20.25, 30.5
    u0 = a * x + b * y + c                                       # 10.75: exposed at the site
    sites = [(x, y, 1.0, 0.0), (x, y, 0.0, -1.0), (x, y, 0.6, 0.8)]
    table, cond = EO.measure_epe(img, sites, [1.0, 0.5], T, True, 32.0, PS)
    # along (1, 0) u falls by 0.25 per pixel, along (0, -1) by 0.125: exact
    assert table[0, 0, 0, 0] == (T - u0) / a * PS == 23.0 * PS
    assert table[0, 0, 0, 2] == 23.0                              # the crossing sits ON a sample, and u == T is still inside
    assert math.isnan(table[0, 0, 1, 0])                         # (T - u0) / -b = 46 pixels: beyond the range, and beyond the grid
    assert table[0, 0, 0, 1] == abs(a) * 0.5 / (0.5 * PS * T)
    # half the dose: u0 / 2 = 5.375, slope -0.125 per pixel along x: t* = 3, slope -0.0625 along -y: t* = 6
    assert table[1, 0, 0, 0] == 3.0 * PS and table[1, 0, 1, 0] == 6.0 * PS
    assert table[1, 0, 1, 1] == 0.0625 * 0.5 / (0.5 * PS * T)
    # oblique: slope s = 0.6 a + 0.8 b = -0.05 per pixel; t* = (T - u0) / s = 115 out of range at dose 1, 15 at dose 0.5.
    # Bound: a sample's position is x + t nx in fp32 (three roundings, each <= 2^-24 of a coordinate < n), its value eight more
    # roundings of quantities <= max|img|; du <= 2^-24 (8 max|img| + 3 n (|a| + |b|)), both ends and the division's
    # condition: 3 du / |s| pixels, plus 2^-22 t* for the fp32 normal (0.6f, 0.8f) against the exact one.
    assert math.isnan(table[0, 0, 2, 0])
    s = 0.5 * (0.6 * a + 0.8 * b)
    t_star = (T - 0.5 * u0) / s
    du = U * (8 * float(np.abs(img).max()) + 3 * n * (abs(a) + abs(b)))
    bound = 3 * du / abs(s) + 2.0 ** -22 * t_star
    assert t_star == pytest.approx(15.0)
    assert abs(table[1, 0, 2, 0] / PS - t_star) <= bound < 1e-2
    assert table[1, 0, 2, 2] in (14.5, 15.0)
    assert cond[1, 0, 2] == pytest.approx((T + 2 * T) / (0.5 * abs(s)), rel=0.2)


# ---- every case of the rule on V profiles: v = a * min_i |x - c_i| along x, constant along y; dark features where v < T
def v_image(n, centres, a=0.5):
    x = np.arange(n, dtype=np.float64)
    v = a * np.min([np.abs(x - c) for c in centres], axis=0)
    return np.repeat(v[None, :].astype(np.float32), n, axis=0)


def test_rule_cases_on_v_profiles():
    n, T = 64, 1.0
    img = v_image(n, (20.25, 32.0))                  # dark features (18.25, 22.25) and (30, 34): leaving them going +x at 22.25 and 34
    nan = float("nan")

    def one(x, nx, rng, exposed=False, y=10.0, ny=0.0):
        t, _ = EO.measure_epe(img, [(x, y, nx, ny)], [1.0], T, exposed, rng, PS)
        return tuple(t[0, 0, 0])

    ils = 0.25 / (0.5 * PS * T)                      # |du| = a h
    # the nearest crossing: 22.25 from x = 21
    assert one(21.0, 1.0, 8.0) == (1.25 * PS, ils, 1.0)
    # positive and negative candidates: from 29, +5 (k = 9) beats -6.75 (k = -14); from 27, -4.75 (k = -10) beats +7 (k = 13)
    assert one(29.0, 1.0, 8.0) == (5.0 * PS, ils, 4.5)
    assert one(27.0, 1.0, 8.0) == (-4.75 * PS, ils, -5.0)
    # a tie: from 28.125 the crossings lie at -5.875 (k = -12) and +5.875 (k = 11), |2k + 1| = 23 both: k >= 0 wins
    assert one(28.125, 1.0, 8.0) == (5.875 * PS, ils, 5.5)
    # a crossing in the wrong direction (entering the feature at 18.25) is ignored: nothing within 4 px of 16, 22.25 within 8
    assert all(math.isnan(v) for v in one(16.0, 1.0, 4.0))
    assert one(16.0, 1.0, 8.0) == (6.25 * PS, ils, 6.0)
    # the same edge seen with the normal reversed: leaving the feature going -x at 18.25
    assert one(20.0, -1.0, 8.0) == (1.75 * PS, ils, 1.5)
    # exposed = True: the bright side is the feature; going +x from 17 it ends at 18.25
    assert one(17.0, 1.0, 8.0, exposed=True) == (1.25 * PS, ils, 1.0)
    # dark at the site: going +x the bright side is only ENTERED at 22.25; it was left at 18.25, behind the site
    assert one(21.0, 1.0, 8.0, exposed=True) == (-2.75 * PS, ils, -3.0)
    assert all(math.isnan(v) for v in one(21.0, 1.0, 2.0, exposed=True))
    # a ray that leaves the grid: bright from 34 to the border, no crossing; the samples beyond n - 1 are not read
    assert all(math.isnan(v) for v in one(60.0, 1.0, 8.0, exposed=True))
    # ... and a crossing whose outer sample would lie beyond the border does not count (dark feature touching the border)
    edge = v_image(n, (62.0,))                       # dark from 60 on
    t, _ = EO.measure_epe(edge, [(62.0, 5.0, 1.0, 0.0)], [1.0], T, False, 8.0, PS)
    assert np.isnan(t).all()
    # a site outside the grid whose ray points away, a NaN and an infinite site
    for site in ((-5.0, 10.0, -1.0, 0.0), (n + 3.0, 10.0, 1.0, 0.0), (nan, 10.0, 1.0, 0.0), (20.0, 10.0, nan, 0.0),
                 (float("inf"), 10.0, 1.0, 0.0), (20.0, 10.0, 1.0, float("-inf"))):
        t, c = EO.measure_epe(img, [site], [1.0], T, False, 8.0, PS)
        assert np.isnan(t).all() and (c == 0).all(), site
    # a site outside whose ray enters the grid finds what the valid samples show
    assert one(-2.0, 1.0, 32.0, exposed=True) == ((18.25 + 2.0) * PS, ils, 20.0)
    # along a column nothing changes: no crossing
    assert all(math.isnan(v) for v in one(21.0, 0.0, 8.0, ny=1.0))
    # n = 2: the one cell; n = 1: NaN
    tiny = np.array([[2.0, 0.0], [2.0, 0.0]], dtype=np.float32)
    t, _ = EO.measure_epe(tiny, [(0.0, 0.5, 1.0, 0.0)], [1.0], 1.0, True, 1.0, PS)
    assert tuple(t[0, 0, 0]) == (0.5 * PS, 1.0 / (0.5 * PS), 0.5)
    assert np.isnan(EO.measure_epe(np.ones((1, 1), dtype=np.float32), [(0.0, 0.0, 1.0, 0.0)], [1.0], 0.5, True, 1.0, PS)[0]).all()


def test_c_entry_rejects_bad_arguments_before_any_launch():
    """litho_measure_epe validates on the host: these return LITHO_E_ARG without a device (the pointers are never followed)."""
    import ctypes

    from lithographysimulator_amd import _native as nat
    assert "litho_measure_epe" in nat.exported_symbols()
    f = nat.lib().litho_measure_epe
    buf = (ctypes.c_float * 16)(*([1.0] * 16))
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(image=p, planes=1, n=2, sites=p, n_sites=1, gains=p, n_gains=1, T=0.5, exposed=1, rng=8.0, ps=25.0, out=p)
    nan = (ctypes.c_float * 1)(float("nan"))
    for change in (dict(image=None), dict(sites=None), dict(gains=None), dict(out=None), dict(n_sites=0), dict(planes=0),
                   dict(n=0), dict(n_gains=0), dict(n_gains=65), dict(rng=0.0), dict(rng=-1.0), dict(rng=32.25),
                   dict(rng=float("nan")), dict(rng=float("inf")), dict(ps=0.0), dict(ps=-1.0), dict(ps=float("nan")),
                   dict(gains=ctypes.cast(nan, ctypes.c_void_p))):
        a = dict(good, **change)
        assert f(*a.values(), None) == nat.E_ARG, change
    assert list(buf) == [1.0] * 16


# ---- geometry
def test_layout_sites_on_a_rectangle_and_an_l():
    import lithographysimulator_amd as L
    r = C.rect(100.0, 200.0, 500.0, 350.0)
    s = L.layoutSites([r[::-1]], 150.0, 25.0, (0.0, 0.0), 64, 193.0)             # given clockwise: made counter-clockwise
    assert len(s) == 3 + 1 + 3 + 1
    assert s.edge.tolist() == [0, 0, 0, 1, 2, 2, 2, 3] and s.polygon.tolist() == [0] * 8
    want_n = [(0, -1)] * 3 + [(1, 0)] + [(0, 1)] * 3 + [(-1, 0)]
    assert np.array_equal(s.normal, np.array(want_n, dtype=np.float64))
    assert np.allclose(s.xy_nm[:3], [(100 + 400 / 6, 200), (300, 200), (500 - 400 / 6, 200)]) and tuple(s.xy_nm[3]) == (500.0, 275.0)
    assert np.array_equal(s.fragment_ends_nm[0, 0], [100.0, 200.0]) and np.array_equal(s.fragment_ends_nm[2, 1], [500.0, 200.0])
    _, off = L.imageRegistration(64, 25.0, 193.0)
    assert np.allclose(s.sites_px[:, 0], s.xy_nm[:, 0] / 25.0 - 0.5 + off, atol=1e-5) and s.sites_px.dtype == np.float32
    assert np.array_equal(s.sites_px[:, 2:], s.normal.astype(np.float32))
    ell = C.layout()[4]
    s = L.layoutSites([r, ell], 150.0, 25.0, (0.0, 0.0), 128, 193.0)
    assert len(s) == 8 + (6 + 2 + 4 + 4 + 2 + 6) and s.polygon.tolist() == [0] * 8 + [1] * 24
    for i in range(len(s)):                          # outward: a step along the normal leaves the polygon, against it stays inside
        poly = [r, ell][s.polygon[i]]
        assert not LO.point_in_polygons([poly], *(s.xy_nm[i] + s.normal[i]))
        assert LO.point_in_polygons([poly], *(s.xy_nm[i] - s.normal[i]))
    tri = np.array([[0.0, 0.0], [300.0, 0.0], [0.0, 400.0]])
    s = L.layoutSites([tri], 1000.0, 25.0, None, 64, 193.0)                      # any angle; origin None = rasterizeLayout's window
    assert np.allclose(s.normal[1], (0.8, 0.6)) and np.allclose(s.xy_nm[1], (150.0, 200.0))
    assert np.allclose(s.sites_px[1, :2] - s.sites_px[0, :2], ((150 - 150) / 25.0, 200 / 25.0), atol=1e-5)


def test_registration_sizes_are_those_of_the_library():
    """The host restatement of the FFT sizing and of the post-processed size against the C entries."""
    import ctypes

    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat
    from lithographysimulator_amd import metrology as M
    for pn in (64, 96, 126, 128, 256, 1000, 2048, 4096):
        for pixel in (10.0, 12.5, 25.0, 48.0):
            for wl in (193.0, 248.0, 13.5):
                eps, N = nat.epsilon_n(4.0 / pn, pixel, wl)
                assert M._epsilon_n(4.0 / pn, pixel, wl) == (eps, N), (pn, pixel, wl)
                n_out = ctypes.c_int(0)
                if N < pn or nat.lib().litho_postprocess_size(pn, eps, ctypes.byref(n_out)) != 0:
                    with pytest.raises(ValueError):
                        L.imageRegistration(pn, pixel, wl)
                    continue
                assert L.imageRegistration(pn, pixel, wl)[0] == n_out.value, (pn, pixel, wl)
    for bad in ((128, 25.0, float("nan")), (128, 25.0, 0.0), (128, float("inf"), 193.0), (1, 25.0, 193.0)):
        with pytest.raises(ValueError):
            L.imageRegistration(*bad)
        with pytest.raises(ValueError):
            L.layoutSites([C.rect(0.0, 0.0, 100.0, 100.0)], 50.0, bad[1], (0.0, 0.0), bad[0], bad[2])


def _raster(polys, pn=64, pixel=12.5):
    from lithographysimulator_amd.layout import polygonEdges
    return LO.rasterize_edges(polygonEdges(polys), pn, 0.0, 0.0, pixel)


def _area(q):
    return 0.5 * float(np.sum(q[:, 0] * np.roll(q[:, 1], -1) - np.roll(q[:, 0], -1) * q[:, 1]))


def test_bias_layout():
    import lithographysimulator_amd as L
    polys = [C.rect(100.0, 200.0, 500.0, 350.0), np.array([[150.0, 420.0], [600.0, 420.0], [600.0, 500.0], [330.0, 500.0],
                                                            [330.0, 700.0], [150.0, 700.0]])[::-1]]
    s = L.layoutSites(polys, 70.0, 12.5, (0.0, 0.0), 64, 193.0)
    same = L.biasLayout(polys, s, np.zeros(len(s)))
    assert np.array_equal(_raster(same), _raster(polys)) and _raster(polys).sum() > 100
    assert [len(q) for q in same] == [4, 6]                                      # no vertex added between equal biases
    # a uniform bias b on a w x h rectangle: the (w + 2b) x (h + 2b) rectangle
    r = polys[:1]
    sr = L.layoutSites(r, 70.0, 12.5, (0.0, 0.0), 64, 193.0)
    for b in (7.0, -20.0):
        grown = L.biasLayout(r, sr, np.full(len(sr), b))
        assert len(grown) == 1 and len(grown[0]) == 4
        assert sorted(map(tuple, grown[0])) == sorted(map(tuple, C.rect(100.0 - b, 200.0 - b, 500.0 + b, 350.0 + b)))
    # one displaced fragment: area changes by b x its length, two jogs = four more vertices (two at a corner fragment)
    for i in (1, 0, 6):
        for b in (9.0, -4.0):
            bias = np.zeros(len(sr))
            bias[i] = b
            moved = L.biasLayout(r, sr, bias)[0]
            frag = float(np.linalg.norm(sr.fragment_ends_nm[i, 1] - sr.fragment_ends_nm[i, 0]))
            assert _area(moved) - _area(r[0]) == pytest.approx(b * frag, abs=1e-9)
            assert len(moved) == (4 + 4 if i == 1 else 4 + 2)
    # 45 degrees raises; so do a wrong count and a NaN bias
    tri = [np.array([[0.0, 0.0], [300.0, 0.0], [0.0, 300.0]])]
    st = L.layoutSites(tri, 100.0, 12.5, (0.0, 0.0), 64, 193.0)
    with pytest.raises(ValueError):
        L.biasLayout(tri, st, np.zeros(len(st)))
    with pytest.raises(ValueError):
        L.biasLayout(r, sr, np.zeros(len(sr) + 1))
    with pytest.raises(ValueError):
        L.biasLayout(r, sr, np.full(len(sr), np.nan))


# ---- registration of the image grid against the mask raster, on the oracle chain
@pytest.mark.parametrize("pn,pixel", [(64, 25.0), (96, 25.0), (128, 25.0), (128, 48.0)])
def test_registration_makes_opposite_edges_agree(pn, pixel):
    """A lattice-aligned rectangle placed off-centre, imaged by the oracle chain (circular sigma 0.5, ideal pupil, threshold
    0.3 x clear field): by symmetry its opposite edges have the same EPE, and read on the unregistered grid they do not.
    Measured |EPE_1 - EPE_2| in nm, (x pair, y pair), unregistered -> registered -- a record, not the bound:
      (64, 25):  1.94, 1.90 -> 0.008, 0.026        (96, 25):  16.2, 12.7 -> 1.70, 2.41 (the 0.69x mask resampling is not
      (128, 25): 4.63, 3.88 -> 0.69, 0.001          shift-invariant)       (128, 48): 120.9, 127.4 -> 0.48, 1.12
    (128, 48) post-processes to 126^2 and its second resampling is a copy: the map has the scale epsilon left over."""
    import lithographysimulator_amd as L
    m = C.OracleModel(pn=pn, pixel=pixel, antialias=1)
    n_out, off = L.imageRegistration(pn, pixel, C.WAVELENGTH)
    x0, y0, w, h = round(pn * 0.22) * pixel, round(pn * 0.30) * pixel, round(pn * 0.25) * pixel, round(pn * 0.31) * pixel
    poly = [C.rect(x0, y0, x0 + w, y0 + h)]
    img = m.imager(poly)
    assert img.shape == (n_out, n_out) and n_out == {(64, 25.0): 64, (96, 25.0): 94, (128, 25.0): 128, (128, 48.0): 126}[(pn, pixel)]
    s = L.layoutSites(poly, 1e9, pixel, (0.0, 0.0), pn, C.WAVELENGTH)          # bottom, right, top, left
    assert len(s) == 4
    plain = np.concatenate([s.xy_nm / pixel - 0.5, s.normal], axis=1).astype(np.float32)
    e0 = EO.measure_epe(img, plain, [1.0], 0.3 * m.clear, True, 8.0, pixel)[0][0, 0, :, 0]
    e1 = EO.measure_epe(img, s.sites_px, [1.0], 0.3 * m.clear, True, 8.0, pixel)[0][0, 0, :, 0]
    assert np.isfinite(e0).all() and np.isfinite(e1).all()
    checked = 0
    for a, b in ((1, 3), (0, 2)):
        before, after = abs(e0[a] - e0[b]), abs(e1[a] - e1[b])
        print(f"pn {pn} pixel {pixel}: offset {off:+.4f} px, edges {a},{b}: |dEPE| {before:.3f} nm -> {after:.3f} nm")
        if before > 1.0:
            checked += 1
            assert after < 0.5 * before, (pn, pixel, a, b, before, after)
    assert checked == 2
    # the offset the function reports is the sites' shift at the window centre
    centre = (pn - 1) / 2.0
    sc = L.layoutSites([C.rect(centre * pixel, centre * pixel, (centre + 2) * pixel, (centre + 2) * pixel)], 1e9, pixel, (0.0, 0.0), pn,
                       C.WAVELENGTH)
    assert sc.sites_px[3, 0] == pytest.approx(centre - 0.5 + off, abs=5e-3)
