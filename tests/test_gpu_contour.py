"""GPU parity of the contour tracer (litho_contour_count / litho_contour_emit) and the dose-focus envelope against the CPU
restatement tests/contour_oracle.py (pinned by closed forms and the raster round trip in test_contour_cpu.py).

Classification, numbering, linking and the saddle's centre value are the same fp32 operations on both sides, so vertex
counts, the order of the vertices, `next` and the grid edge every vertex lies on must be IDENTICAL; a difference is a bug,
not noise.  Position on the edge: c + t, t = (T - a) / (b - a) in fp32 -- the difference T - a, the difference b - a, the
division and the sum.  contour.hip is built without fast-math and with -ffp-contract=off, fp32 division on the device is
correctly rounded and fp32 denormals are kept, so these four operations are NumPy float32's, and on the MI355X the device's
division did turn out bit-equal to numpy's: every coordinate of every parity case (n = 2 .. 130, 3 planes x 2 gains, both
tones, samples equal to T, NaN and +-inf among them; 162 012 of 162 012 coordinates at n = 130) has the bits of the float32
restatement.  So EQUALITY OF THE BITS is what is asserted, as the issue asks in that case.  The derived bound
|x - x_f64| <= 2^-22 (|c| + cond), cond = (|T| + |a| + |b|) / |b - a| (four roundings; the derivation of test_gpu_epe.py's
docstring), x_f64 the float64 evaluation from the same fp32 a, b, is asserted as well: it holds the restatement itself, and
with it the device, to the definition, and it is the bound the measureEPE cross-check and the PV-band test build on."""
import ctypes

import numpy as np
import pytest
import torch

import contour_oracle as CO
import epe_oracle as EO
from helpers import NA, PS, WL, f16

pytestmark = pytest.mark.gpu

F = np.float32
T = 0.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    import lithographysimulator_amd as L
    return L


def seeded_stack(n, planes, seed, special=True):
    """Real-valued planes around T = 0.5 (half of the samples inside: saddles, holes and islands in plenty); with `special` a
    few samples whose product with the gains 1 and 0.5 equals T exactly, and a few NaN / inf ones."""
    rng = np.random.default_rng(seed)
    u = rng.random((planes, n, n)).astype(F)
    u = ((u + np.roll(u, 1, 1) + np.roll(u, 1, 2)) / F(3)).astype(F) if n > 3 else u
    if special:
        k = max(1, n // 8)
        for value in (F(0.5), F(1.0), F(np.nan), F(np.inf), F(-np.inf)):
            p, r, c = rng.integers(0, planes, k), rng.integers(0, n, k), rng.integers(0, n, k)
            u[p, r, c] = value
    return u


def split(xy, nxt, offsets):
    xy, nxt = xy.cpu().numpy(), nxt.cpu().numpy()
    return [(xy[a:b], nxt[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]


def compare_with_oracle(got_xy, got_next, u, gain, exposed, stats):
    """The module docstring's assertions for one image: counts, numbering, links and the bits of every coordinate equal to the
    restatement's; besides, the interpolated coordinate inside its edge and within the derived bound of the float64 value."""
    t = CO.trace(u, gain, T, exposed)
    assert len(got_next) == len(t["next"])                                       # vertex count
    assert np.array_equal(got_next, t["next"])                                   # numbering and linking
    assert np.array_equal(got_xy.view(np.int32), t["xy"].view(np.int32))         # every coordinate, bit for bit
    want = t["whole"].astype(np.float64)
    g = got_xy.astype(np.float64)
    moving = np.where(t["horizontal"], 0, 1)
    fixed = 1 - moving
    rows = np.arange(len(g))
    assert np.array_equal(g[rows, fixed], want[rows, fixed])
    d = g[rows, moving] - want[rows, moving]
    assert ((d >= 0) & (d <= 1)).all()                                           # the integer part: on its own grid edge
    tol = 2.0 ** -22 * (np.abs(want[rows, moving]) + t["cond"])
    err = np.abs(d - t["frac64"])
    assert (err <= tol).all(), (float(err.max()), float((err / np.maximum(tol, 1e-300)).max()))
    stats["vertices"] += len(g)
    stats["bit_equal"] += int(np.sum(got_xy.view(np.int32) == t["xy"].view(np.int32)))
    stats["coords"] += 2 * len(g)
    stats["worst"] = max(stats["worst"], float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0)
    stats["saddles"] += sum(t["saddles"])
    return t


@pytest.mark.parametrize("n", [2, 3, 62, 63, 64, 65, 127, 130])
def test_parity_with_the_oracle(L, dev, n):
    planes, doses = 3, [1.0, 0.5]
    u = seeded_stack(n, planes, 1000 + n)
    img = torch.from_numpy(u).to(dev)
    stats = dict(vertices=0, bit_equal=0, coords=0, worst=0.0, saddles=0)
    for exposed in (True, False):
        xy, nxt, offsets = L.contourVertices(img, T, doses, exposed)
        assert xy.dtype == torch.float32 and nxt.dtype == torch.int32 and offsets.dtype == np.int64 and len(offsets) == 7
        assert tuple(xy.shape) == (int(offsets[-1]), 2) and tuple(nxt.shape) == (int(offsets[-1]),)
        parts = split(xy, nxt, offsets)
        for gi, gain in enumerate(doses):
            for p in range(planes):
                gx, gn = parts[gi * planes + p]
                compare_with_oracle(gx, gn, u[p], gain, exposed, stats)
    print(f"n {n}: {stats['vertices']} vertices, {stats['saddles']} saddles, {stats['bit_equal']} of {stats['coords']} coordinates "
          f"bit-equal to the float32 restatement, worst error {stats['worst']:.3f} of its bound")
    assert stats["vertices"] > 0 and stats["bit_equal"] == stats["coords"] and stats["worst"] <= 1.0
    if n >= 62:
        assert stats["saddles"] > 50


def test_batched_call_equals_single_calls(L, dev):
    n, planes, doses = 130, 3, [1.0, 0.5]
    u = seeded_stack(n, planes, 77)
    img = torch.from_numpy(u).to(dev)
    for exposed in (True, False):
        parts = split(*L.contourVertices(img, T, doses, exposed))
        for gi, gain in enumerate(doses):
            for p in range(planes):
                xy, nxt, offsets = L.contourVertices(img[p], T, [gain], exposed)
                assert offsets.tolist() == [0, len(parts[gi * planes + p][1])]
                assert np.array_equal(xy.cpu().numpy().view(np.int32), parts[gi * planes + p][0].view(np.int32))
                assert np.array_equal(nxt.cpu().numpy(), parts[gi * planes + p][1])
    # a stack without any crossing: empty outputs, no launch of the emit pass
    xy, nxt, offsets = L.contourVertices(torch.zeros(2, 9, 9, device=dev), T, doses)
    assert xy.shape == (0, 2) and nxt.shape == (0,) and offsets.tolist() == [0] * 5


def ringed(u, exposed):
    """The round trip's second condition: the image's border ring outside the feature."""
    out = F(0.0) if exposed else F(2.0)
    u[..., 0, :] = u[..., -1, :] = u[..., :, 0] = u[..., :, -1] = out
    return u


@pytest.mark.parametrize("n", [64, 130])
def test_round_trip_on_the_device(L, dev, n):
    """rasterizeLayout(traceContours(image), orient=False) with origin (-0.5, -0.5) and pixel 1 -- pixel centres on the samples
    -- gives back the inside predicate at EVERY sample, provided no product equals T and the border ring is outside."""
    doses = [1.0, 0.8]
    holes = 0
    for exposed in (True, False):
        u = ringed(seeded_stack(n, 2, 500 + n + exposed, special=False), exposed)
        img = torch.from_numpy(u).to(dev)
        for gain in doses:
            assert not bool((img * gain == T).any())
        traced = L.traceContours(img, T, doses, exposed)
        assert len(traced) == 2 and len(traced[0]) == 2
        for gi, gain in enumerate(doses):
            for p in range(2):
                c = traced[gi][p]
                holes += int(c.holes.sum())
                ras = L.rasterizeLayout(c.polygons, n, 1.0, (-0.5, -0.5), dev, orient=False)
                want = ((img[p] * gain) >= T) == exposed
                assert int(((ras != 0) != want).sum()) == 0
                assert abs(c.total_area_px - float(np.sum(c.area_px))) == 0 and np.array_equal(c.holes, c.area_px < 0)
    assert holes > 10


def test_envelope_and_pv_band(L, dev):
    n, planes, doses = 130, 3, [1.0, 0.8]
    rng = np.random.default_rng(9)
    y, x = np.mgrid[0:n, 0:n]
    u = np.stack([np.exp(-(((x - 60 - 3 * p) / (30.0 + p)) ** 2 + ((y - 70 + 2 * p) / (22.0 - p)) ** 2)) for p in range(planes)])
    u = ringed((u + 0.2 * np.exp(-((x - 100) ** 2 + (y - 30) ** 2) / 40.0) + 0.01 * rng.random((planes, n, n))).astype(F) * F(1.5), True)
    u[1, 5, 7] = F(np.inf)
    img = torch.from_numpy(u).to(dev)
    lo, hi = L.doseFocusEnvelope(img, doses)
    prod = np.stack([CO.products(u[p], g) for p in range(planes) for g in doses])
    assert np.array_equal(lo.cpu().numpy().view(np.int32), np.fmin.reduce(prod, axis=0).view(np.int32))
    assert np.array_equal(hi.cpu().numpy().view(np.int32), np.fmax.reduce(prod, axis=0).view(np.int32))
    ins = prod >= F(T)
    assert np.array_equal(hi.cpu().numpy() >= F(T), ins.any(axis=0)) and np.array_equal(lo.cpu().numpy() >= F(T), ins.all(axis=0))
    u[1, 5, 7] = F(0.0)
    img = torch.from_numpy(u).to(dev)
    # the band: nested regions give ordered areas in exact arithmetic (marching squares with the centre-value saddle rule is
    # monotone in the image).  In fp32 every vertex of a contour is displaced along its grid edge by at most its
    # 2^-22 (|c| + cond) <= 2^-22 (n + cond), and that moves the contour's area by at most the displacement times sqrt 2 (the
    # two segments at a vertex lie in one cell each).  An ordering of two areas is therefore asserted up to the sum of the
    # two contours' own bounds: the envelope's and that condition's, each from its own vertices and condition numbers.
    def rounding(field_, gain, exposed):
        return float(np.sum(2.0 ** -22 * (n + CO.trace(field_, gain, T, exposed)["cond"]))) * 2 ** 0.5

    for exposed in (True, False):
        outer, inner, band = L.processVariationBand(img, T, doses, exposed)
        lo_h, hi_h = (a.cpu().numpy() for a in L.doseFocusEnvelope(img, doses))
        s_in, s_out = (rounding(f_, 1.0, exposed) for f_ in ((lo_h, hi_h) if exposed else (hi_h, lo_h)))
        assert band >= 0 and band == outer.total_area_px - inner.total_area_px and len(outer) >= 1 and len(inner) >= 1
        traced = L.traceContours(img, T, doses, exposed)
        worst = 0.0
        for gi, gain in enumerate(doses):
            for p in range(planes):
                c, s_c = traced[gi][p], rounding(u[p], gain, exposed)
                assert inner.total_area_px - (s_in + s_c) <= c.total_area_px <= outer.total_area_px + (s_out + s_c)
                worst = max(worst, s_in + s_c, s_out + s_c)
        areas = [c.total_area_px for per_dose in traced for c in per_dose]
        print(f"exposed {exposed}: inner {inner.total_area_px:.3f} <= conditions {min(areas):.3f} .. {max(areas):.3f} <= outer "
              f"{outer.total_area_px:.3f} px^2, band {band:.3f}, largest rounding tolerance {worst:.2e}")
        # the tolerance is the derived bound and nothing else (a few hundredths of a px^2 on contours of several hundred
        # vertices); what keeps the ordering from being vacuous is that the band it brackets is orders of magnitude wider
        assert band > 10 * worst


@pytest.fixture(scope="module")
def focus_stack(L, dev):
    """The 256^2 five-plane focus stack of test_gpu_epe.py, rebuilt: lines_mask(256), circular sigma 0.5 source, aberration-free
    focal planes -120 .. +120 nm; T between two adjacent distinct sample values next to the mid level of the centre row."""
    from lithographysimulator_amd.synthetic import lines_mask
    pn = 256
    mask = L.Mask(lines_mask(pn), PS, dev)
    mft = mask.fraunhofer(WL, True)
    eps, N = mask.calculateEpsilonN(mask.deltaK, PS, WL)
    stack = L.throughFocusPupils(pn, WL, NA, f16([0, 0, 0, 0, 0]), [-120.0, -60.0, 0.0, 60.0, 120.0], dev)
    sh = L.sourceShifts(L.LightSource(0.0, 0.5, pn, NA, device=dev).generateAnnular(), pn)
    img = L.postProcess(L.abbeIntensity(mft, stack, sh, N), eps)
    n = img.shape[-1]
    row = img[2, n // 2]
    mid = 0.5 * float(row[n // 4: 3 * n // 4].min() + row[n // 4: 3 * n // 4].max())
    values = np.unique(img.cpu().numpy())
    k = int(np.searchsorted(values, F(mid)))
    thr = float(F(0.5 * (float(values[k - 1]) + float(values[k]))))
    if thr == float(values[k - 1]) or thr == float(values[k]):                  # neighbours one ulp apart: no fp32 between them
        thr = float(values[k])
    return dict(img=img, n=n, thr=thr)


def test_cross_check_with_measure_epe(L, dev, focus_stack):
    """A site on a sample of row r with normal (+-1, 0) looks along the very line segments the tracer interpolates on (the
    half-pixel sample between two pixels is their mean), so site + t* is the contour vertex on that grid line.  Tolerance: the
    two derived bounds, EPE's 2^-22 (|t_k| + h cond_epe) and the tracer's 2^-22 (|c| + cond); anything larger is a bug."""
    s = focus_stack
    img, n, thr = s["img"], s["n"], s["thr"]
    host = img.cpu().numpy()
    checked, worst = 0, 0.0
    for p in range(img.shape[0]):
        xy, nxt, offsets = L.contourVertices(img[p], thr, [1.0], True)
        xy = xy.cpu().numpy().astype(np.float64)
        for r in (n // 2 - 40, n // 2, n // 2 + 33):
            on_row = xy[(xy[:, 1] == r) & (xy[:, 0] != np.floor(xy[:, 0]))]       # H-edge vertices of row r
            assert len(on_row) >= 4
            sites, conds, cols = [], [], []
            for xv in on_row[:, 0]:
                c = int(np.floor(xv))
                a, b = float(host[p, r, c]), float(host[p, r, c + 1])
                assert (a >= thr) != (b >= thr)
                sites.append((c, r, 1, 0) if a >= thr else (c + 1, r, -1, 0))    # on the inside sample, looking outward
                conds.append((abs(thr) + abs(a) + abs(b)) / abs(b - a))
                cols.append(c)
            sites = np.array(sites, dtype=F)
            e = L.measureEPE(img[p], thr, sites, PS, exposed=True, searchRange=2.0).cpu().numpy().astype(np.float64)[0, 0]
            table, cond_epe = EO.measure_epe(host[p], sites, [1.0], thr, True, 2.0, PS)
            assert np.isfinite(e).all()
            for k, xv in enumerate(on_row[:, 0]):
                edge = sites[k, 0] + sites[k, 2] * e[k, 0] / PS
                tol = 2.0 ** -22 * (abs(table[0, 0, k, 2]) + EO.H * cond_epe[0, 0, k]) + 2.0 ** -22 * (cols[k] + conds[k])
                worst = max(worst, abs(edge - xv) / tol)
                assert abs(edge - xv) <= tol, (p, r, k, edge, xv, tol)
                assert tol < 0.01
                checked += 1
    print(f"measureEPE cross-check: {checked} edges, worst |site + t* - vertex| = {worst:.3f} of its bound")
    assert checked >= 60


def test_end_to_end_on_the_focus_stack(L, dev, focus_stack):
    s = focus_stack
    img, n, thr = s["img"], s["n"], s["thr"]
    doses = [0.9, 1.0, 1.1]
    assert not bool((img == thr).any())
    xy, nxt, offsets = L.contourVertices(img, thr, doses, True)
    from lithographysimulator_amd.contours import linkContours
    for a, b in zip(offsets[:-1], offsets[1:]):
        order, starts = linkContours(nxt[a:b].cpu().numpy())                     # raises unless next is a permutation: all close
        assert len(order) == b - a and len(starts) >= 2
    traced = L.traceContours(img, thr, doses, True)
    assert len(traced) == 3 and all(len(t) == 5 for t in traced)
    for gi, gain in enumerate(doses):
        for p in range(5):
            prod = img[p] * gain
            assert not bool((prod == thr).any())                                 # the round trip's first condition
            c = traced[gi][p]
            assert len(c) >= 3 and (c.area_px[~c.holes] > 0).all()
            ras = L.rasterizeLayout(c.polygons, n, 1.0, (-0.5, -0.5), dev, orient=False)
            want = prod >= thr
            # the lines run into the image border, so border samples lie ON the contour: the interior is what must agree
            assert int(((ras != 0) != want)[1:-1, 1:-1].sum()) == 0
    # a higher dose prints more: areas ordered in the dose at every plane
    for p in range(5):
        assert traced[0][p].total_area_px < traced[1][p].total_area_px < traced[2][p].total_area_px


def test_argument_errors_through_the_wrapper_and_stale_offsets(L, dev):
    from lithographysimulator_amd import _native as nat
    from lithographysimulator_amd.imageformation import ShapeError
    img = torch.from_numpy(seeded_stack(33, 2, 3, special=False)).to(dev)
    with pytest.raises(ShapeError):
        L.contourVertices(img.double(), T)
    with pytest.raises(ShapeError):
        L.contourVertices(img[:, :, :32], T)
    with pytest.raises(ShapeError):
        L.contourVertices(img, T, doses=[1.0] * 65)
    with pytest.raises(ValueError):
        L.contourVertices(img, T, doses=[float("nan")])
    with pytest.raises(RuntimeError):
        L.contourVertices(img.cpu(), T)                                          # no CPU fallback
    # offsets that do not match the counts found: that image is left unwritten, nothing is written out of place
    lib = nat.lib()
    one = (ctypes.c_float * 1)(1.0)
    nbytes = lib.litho_contour_work_bytes(33, 2, 1)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = nat.stream_ptr(dev)
        assert lib.litho_contour_count(nat.ptr(img), 2, 33, one, 1, T, 1, nat.ptr(work), nbytes, nat.ptr(counts), st) == 0
        c = counts.cpu().numpy()
        good = np.array([0, c[0], c[0] + c[1]], dtype=np.int64)
        bad = np.array([0, c[0], c[0] + c[1] - 1], dtype=np.int64)               # the second image is one short
        xy = torch.full((int(good[-1]), 2), -7.0, device=dev)
        nx = torch.full((int(good[-1]),), -7, dtype=torch.int32, device=dev)
        assert lib.litho_contour_emit(nat.ptr(img), 2, 33, one, 1, T, 1, nat.ptr(work), nbytes, bad.ctypes.data, nat.ptr(xy), nat.ptr(nx), st) == 0
        torch.cuda.synchronize()
        assert bool((nx[:c[0]] >= 0).all()) and bool((nx[c[0]:] == -7).all()) and bool((xy[c[0]:] == -7.0).all())
        assert lib.litho_contour_emit(nat.ptr(img), 2, 33, one, 1, T, 1, nat.ptr(work), nbytes, good.ctypes.data, nat.ptr(xy), nat.ptr(nx), st) == 0
        torch.cuda.synchronize()
    ref_xy, ref_nx, ref_off = L.contourVertices(img, T)
    assert ref_off.tolist() == good.tolist() and torch.equal(ref_xy, xy) and torch.equal(ref_nx, nx)
