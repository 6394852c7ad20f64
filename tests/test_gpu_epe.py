"""GPU parity of the edge-placement-error kernel (litho_measure_epe) against the CPU restatement tests/epe_oracle.py
(pinned by closed forms in test_epe_cpu.py).

The samples and their classification are the same fp32 operations on both sides, so the NaN pattern and the chosen interval
t_k must be IDENTICAL; a difference is a bug, not noise.  Position: t* = t_k + h (T - u_a) / (u_b - u_a) in fp32 -- the
difference T - u_a, the difference u_b - u_a, the division, the product with h (exact), the sum and the product with the
pixel size: at most four ulps of |t_k| + h cond, cond = (|T| + |u_a| + |u_b|) / |u_b - u_a| the division's condition:
|epe - epe_f64| <= 2^-22 (|t_k| + h cond) pixel_size.  ils = |u_b - u_a| / ((h ps) T): three roundings, 4 * 2^-24 relative."""
import numpy as np
import pytest
import torch

import epe_oracle as EO
import resist_oracle as RO
from helpers import NA, PS, WL, f16

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
H = 0.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    import lithographysimulator_amd as L
    return L


@pytest.fixture(scope="module")
def focus_stack(L, dev):
    """The focus stack of test_gpu_resist.py, rebuilt: lines_mask(256), circular sigma 0.5 source, five aberration-free focal
    planes -120 .. +120 nm; plus its 30 nm diffused image."""
    from lithographysimulator_amd.synthetic import lines_mask
    pn = 256
    mask = L.Mask(lines_mask(pn), PS, dev)
    mft = mask.fraunhofer(WL, True)
    eps, N = mask.calculateEpsilonN(mask.deltaK, PS, WL)
    stack = L.throughFocusPupils(pn, WL, NA, f16([0, 0, 0, 0, 0]), [-120.0, -60.0, 0.0, 60.0, 120.0], dev)
    sh = L.sourceShifts(L.LightSource(0.0, 0.5, pn, NA, device=dev).generateAnnular(), pn)
    raw = L.abbeIntensity(mft, stack, sh, N)
    img = L.postProcess(raw, eps)
    n = img.shape[-1]
    r = n // 2
    row = img[2, r]
    c_dark = int(torch.argmin(row[n // 4: 3 * n // 4])) + n // 4
    c_bright = int(torch.argmax(row[n // 4: 3 * n // 4])) + n // 4
    thr = 0.5 * float(row[c_dark] + row[c_bright])
    diffused = L.resistContour(raw, eps, thr, return_image=True, diffusionLength=30.0, pixelSize=PS)[0]
    return dict(img=img, diffused=diffused, n=n, r=r, c_dark=c_dark, c_bright=c_bright, thr=thr)


def seeded_sites(n, count, seed):
    """`count` sites with seeded positions (some beyond the border) and angles, then axis-aligned ones on integer and
    half-integer positions, the four corners with outward normals, sites outside the grid, and NaN / inf sites."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-4.0, n + 3.0, (count, 2))
    ang = rng.uniform(0.0, 2 * np.pi, count)
    rows = [np.concatenate([xy, np.cos(ang)[:, None], np.sin(ang)[:, None]], axis=1)]
    ax = rng.integers(0, n, (40, 2)).astype(np.float64)
    ax[20:] += 0.5
    rows.append(np.concatenate([ax, np.tile([[1, 0], [-1, 0], [0, 1], [0, -1]], (10, 1))], axis=1))
    d = 2.0 ** -0.5
    m = n - 1.0
    rows.append(np.array([[0, 0, -d, -d], [m, 0, d, -d], [0, m, -d, d], [m, m, d, d], [0, 0, -1, 0], [m, m, 0, 1],
                          [-40, 5, -1, 0], [n + 40, n + 40, 1, 1], [5, -70, 0, -1], [np.nan, 5, 1, 0], [5, 5, np.nan, 0],
                          [np.inf, 5, 1, 0], [5, 5, 1, -np.inf], [5, np.nan, 0, np.inf]]))
    return np.concatenate(rows).astype(np.float32)


def compare(got, image, sites, doses, thr, exposed, rng, ps=PS):
    """The assertions of the module docstring; returns the restatement's table."""
    table, cond = EO.measure_epe(image.cpu().numpy(), sites, [float(np.float32(d)) for d in doses], thr, exposed, rng, ps)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == table.shape
    assert np.array_equal(np.isnan(got), np.isnan(table))
    fin = ~np.isnan(table[..., 2])
    assert np.array_equal(np.isnan(table[..., 0]), ~fin) and np.array_equal(np.isnan(table[..., 1]), ~fin)
    assert np.array_equal(got[..., 2][fin], table[..., 2][fin])                  # t_k: the chosen interval, exactly
    if fin.any():
        tol = 2.0 ** -22 * (np.abs(table[..., 2]) + H * cond) * ps
        d = np.abs(got[..., 0] - table[..., 0])[fin]
        print(f"exposed {exposed} range {rng}: {int(fin.sum())} crossings, worst |epe_gpu - epe_f64| = {float(d.max()):.3e} nm = "
              f"{float((d / tol[fin]).max()):.3f} of its bound")
        assert (d <= tol[fin]).all(), (float(d.max()), float((d / tol[fin]).max()))
        assert (np.abs(got[..., 1] - table[..., 1])[fin] <= 4 * U * np.abs(table[..., 1])[fin]).all()
    return table


@pytest.mark.parametrize("which", ["aerial", "diffused"])
def test_kernel_against_the_restatement_on_the_focus_stack(L, dev, focus_stack, which):
    s = focus_stack
    n, thr = s["n"], s["thr"]
    image = s["img"] if which == "aerial" else s["diffused"]
    sites = seeded_sites(n, 400, 19)
    doses = [0.8, 1.0, 1.25]
    outward = inward = lost = 0
    for exposed in (False, True):
        for rng in (8.0, 32.0):
            got = L.measureEPE(image, thr, sites, PS, doses=doses, exposed=exposed, searchRange=rng)
            assert tuple(got.shape) == (3, 5, len(sites), 3) and got.dtype == torch.float32
            table = compare(got, image, sites, doses, thr, exposed, rng)
            outward += int((table[..., 2] >= 0).sum())
            inward += int((table[..., 2] < 0).sum())
            lost += int(np.isnan(table[:, :, :440, 2]).sum())
            assert np.isnan(table[:, :, -8:]).all()                              # outside the grid, NaN, inf
    _, valid, _ = EO.samples(image.cpu().numpy(), sites, 32.0)
    cut = valid.any(axis=1) & ~valid.all(axis=1)
    found = ~np.isnan(EO.measure_epe(image.cpu().numpy(), sites, [1.0], thr, True, 32.0, PS)[0][0, 2, :, 2])
    print(f"{which}: {outward} crossings outward, {inward} inward, {lost} without; {int(cut.sum())} rays cut by the border, "
          f"{int((cut & found).sum())} of them with a crossing")
    assert outward > 500 and inward > 500 and lost > 100 and int((cut & found).sum()) > 5 and int((cut & ~found).sum()) > 0
    # a LayoutSites-free tensor on the device gives the same rows
    dev_sites = torch.from_numpy(sites).to(dev)
    a = L.measureEPE(image, thr, dev_sites, PS, doses=doses, exposed=True, searchRange=32.0)
    assert torch.equal(torch.nan_to_num(a, nan=-1e9), torch.nan_to_num(got, nan=-1e9))


def test_consistent_with_measure_cd(L, dev, focus_stack):
    """Between two pixels of a row the bilinear interpolant at integer y is the very line segment measureCD interpolates on, so
    a site on that row with normal (+-1, 0) finds measureCD's edge: x + t* = x_hi, x - t* = x_lo.  Tolerance: the two derived
    position tolerances, 2^-22 (n + cond_cd) of test_gpu_resist and 2^-22 (|t_k| + h cond) here (the fp32 rounding of the
    half-pixel sample between the two pixels, 2^-24 |u| / |b - a| px, lies inside the latter)."""
    s = focus_stack
    n, r, thr, img = s["n"], s["r"], s["thr"], s["img"]
    checked, worst = 0, 0.0
    for col, exposed in ((s["c_dark"], False), (s["c_bright"], True)):
        gauges = [(r, col, 0), (r - 40, col, 0), (r + 33, col, 0)]
        cd = L.measureCD(img, thr, gauges, PS, exposed=exposed).cpu().numpy().astype(np.float64)[0]      # [planes, G, 5]
        _, runs, cd_tol = RO.measure_cd(img.cpu().numpy(), gauges, [1.0], thr, exposed, PS)
        for p in range(img.shape[0]):
            for g, (row, _, _) in enumerate(gauges):
                lo, hi = int(runs[0, p, g, 0]), int(runs[0, p, g, 1])
                if lo <= 0 or hi >= n - 1 or hi - lo < 1:
                    continue
                back = min(3, hi - lo)                                           # at the edge sample, and up to 3 px inside
                sites = np.array([[hi, row, 1, 0], [hi - back, row, 1, 0], [lo, row, -1, 0], [lo + back, row, -1, 0]], dtype=np.float32)
                e = L.measureEPE(img[p], thr, sites, PS, exposed=exposed, searchRange=8.0).cpu().numpy().astype(np.float64)[0, 0]
                table, cond = EO.measure_epe(img[p].cpu().numpy(), sites, [1.0], thr, exposed, 8.0, PS)
                assert np.isfinite(e).all()
                for k in range(4):
                    sign = 1.0 if k < 2 else -1.0
                    edge = sites[k, 0] + sign * e[k, 0] / PS
                    want = cd[p, g, 2 if k < 2 else 1]
                    tol = 2.0 ** -22 * (n + cd_tol[0, p, g, 1 if k < 2 else 0]) + 2.0 ** -22 * (abs(table[0, 0, k, 2]) + H * cond[0, 0, k])
                    worst = max(worst, abs(edge - want) / tol)
                    assert abs(edge - want) <= tol, (p, g, k, edge, want, tol)
                    assert tol < 0.01
                    checked += 1
    print(f"measureCD consistency: {checked} edges, worst |x + t* - x_cd| = {worst:.3f} of its bound")
    assert checked >= 40


def test_shapes_at_which_the_kernel_can_go_wrong(L, dev):
    gen = torch.Generator().manual_seed(23)
    # n = 126 (what a 128^2 mask at 48 nm post-processes to), three planes
    img = torch.rand(3, 126, 126, generator=gen).to(dev)
    sites = seeded_sites(126, 120, 5)
    for exposed in (False, True):
        got = L.measureEPE(img, 0.5, sites, PS, doses=[1.0, 0.6], exposed=exposed, searchRange=3.0)
        compare(got, img, sites, [1.0, 0.6], 0.5, exposed, 3.0)
    # a 2-D image and the one-plane stack give the same rows
    a = L.measureEPE(img[1], 0.5, sites, PS, searchRange=3.0)
    b = L.measureEPE(img[1:2], 0.5, sites, PS, searchRange=3.0)
    assert tuple(a.shape) == (1, 1, len(sites), 3) and torch.equal(torch.nan_to_num(a, nan=-1e9), torch.nan_to_num(b, nan=-1e9))
    # n = 2, the smallest grid with a cell; S = 1
    tiny = torch.tensor([[2.0, 0.0], [2.0, 0.0]], device=dev)
    one = L.measureEPE(tiny, 1.0, [(0.0, 0.5, 1.0, 0.0)], PS, searchRange=1.0).cpu()
    assert tuple(one.shape) == (1, 1, 1, 3) and one[0, 0, 0].tolist() == [0.5 * PS, float(np.float32(1.0 / (0.5 * PS))), 0.5]
    few = np.array([[0.0, 0.5, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0], [0.25, 0.25, 0.5, 0.5], [1.0, 0.0, -1.0, 0.0]], dtype=np.float32)
    compare(L.measureEPE(tiny, 1.0, few, PS, searchRange=32.0), tiny, few, [1.0], 1.0, True, 32.0)
    # n = 1: no cell, three NaN, nothing read
    assert bool(torch.isnan(L.measureEPE(torch.ones(1, 1, device=dev), 0.5, few, PS)).all())
    # the four corners with outward normals, sites outside the grid, NaN / inf sites.  A corner's outward half is all invalid
    # beyond the corner sample itself (so nothing is found at t_k >= 0: interval 0 needs sample 1), its inward half runs
    # along the diagonal or the border inside the grid and was compared on the random image above; the sites beyond the
    # corners are invalid throughout and give NaN on any image
    tail = seeded_sites(126, 0, 0)[-14:]
    _, valid, t = EO.samples(img.cpu().numpy(), tail, 32.0)
    assert valid[:6][:, t == 0].all() and not valid[:6][:, t > 0].any() and valid[:6][:, (t < 0) & (t >= -8)].all()
    assert not valid[6:].any()
    corners = L.measureEPE(img, 0.5, tail, PS, searchRange=32.0)
    table = compare(corners, img, tail, [1.0], 0.5, True, 32.0)
    assert not (table[..., :6, 2] >= 0).any() and np.isfinite(table[..., :6, 2]).any()
    assert bool(torch.isnan(corners[:, :, 6:]).all())
    flat = torch.full((126, 126), 2.0, device=dev)                                # no contour at all: NaN everywhere
    for exposed in (False, True):
        assert bool(torch.isnan(L.measureEPE(flat, 0.5, tail, PS, exposed=exposed, searchRange=32.0)).all())


def test_seventy_thousand_sites(L, dev):
    """The site index exceeds a 16-bit grid dimension: sites ride on blockIdx.x."""
    gen = torch.Generator().manual_seed(29)
    img = torch.rand(64, 64, generator=gen).to(dev)
    S = 70000
    rng = np.random.default_rng(31)
    ang = rng.uniform(0, 2 * np.pi, S)
    sites = np.concatenate([rng.uniform(-1.0, 64.0, (S, 2)), np.cos(ang)[:, None], np.sin(ang)[:, None]], axis=1).astype(np.float32)
    got = L.measureEPE(img, 0.5, sites, PS, searchRange=2.0)
    table = compare(got, img, sites, [1.0], 0.5, True, 2.0)
    assert np.isfinite(table[0, 0, 65536:, 0]).sum() > 1000 and np.isnan(table[0, 0, 65536:, 0]).sum() > 10
    # the last site alone gives its row of the big call
    alone = L.measureEPE(img, 0.5, sites[-1:], PS, searchRange=2.0)
    assert torch.equal(torch.nan_to_num(alone[0, 0, 0], nan=-1e9), torch.nan_to_num(got[0, 0, -1], nan=-1e9))


def test_argument_errors_through_the_c_entry_and_the_wrapper(L, dev):
    from lithographysimulator_amd import _native as nat
    from lithographysimulator_amd.imageformation import ShapeError
    import ctypes
    img = torch.rand(2, 32, 32, generator=torch.Generator().manual_seed(3)).to(dev)
    sites = torch.tensor([[10.0, 10.0, 1.0, 0.0], [12.0, 9.0, 0.0, 1.0]], device=dev)
    out = torch.full((1, 2, 2, 3), -7.0, device=dev)
    one = (ctypes.c_float * 1)(1.0)
    bad_gain = (ctypes.c_float * 1)(float("nan"))
    f = nat.lib().litho_measure_epe
    st = nat.stream_ptr(dev)
    i, s, o = nat.ptr(img), nat.ptr(sites), nat.ptr(out)
    with torch.cuda.device(dev):
        for args in ((None, 2, 32, s, 2, one, 1, 0.5, 1, 8.0, 25.0, o), (i, 2, 32, None, 2, one, 1, 0.5, 1, 8.0, 25.0, o),
                     (i, 2, 32, s, 2, None, 1, 0.5, 1, 8.0, 25.0, o), (i, 2, 32, s, 2, one, 1, 0.5, 1, 8.0, 25.0, None),
                     (i, 2, 32, s, 0, one, 1, 0.5, 1, 8.0, 25.0, o), (i, 0, 32, s, 2, one, 1, 0.5, 1, 8.0, 25.0, o),
                     (i, 2, 32, s, 2, one, 0, 0.5, 1, 8.0, 25.0, o), (i, 2, 32, s, 2, one, 65, 0.5, 1, 8.0, 25.0, o),
                     (i, 2, 32, s, 2, one, 1, 0.5, 1, 0.0, 25.0, o), (i, 2, 32, s, 2, one, 1, 0.5, 1, 32.5, 25.0, o),
                     (i, 2, 32, s, 2, one, 1, 0.5, 1, float("nan"), 25.0, o), (i, 2, 32, s, 2, one, 1, 0.5, 1, float("inf"), 25.0, o),
                     (i, 2, 32, s, 2, one, 1, 0.5, 1, -1.0, 25.0, o), (i, 2, 32, s, 2, one, 1, 0.5, 1, 8.0, 0.0, o),
                     (i, 2, 32, s, 2, one, 1, 0.5, 1, 8.0, -25.0, o), (i, 2, 32, s, 2, bad_gain, 1, 0.5, 1, 8.0, 25.0, o)):
            assert f(*args, st) == nat.E_ARG, args[1:11]
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())                                         # nothing was written
        assert f(i, 2, 32, s, 2, one, 1, 0.5, 1, 32.0, 25.0, o, st) == 0
        torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(out, nan=-1e9), torch.nan_to_num(L.measureEPE(img, 0.5, sites, 25.0, searchRange=32.0), nan=-1e9))
    with pytest.raises(ShapeError):
        L.measureEPE(img.double(), 0.5, sites, 25.0)
    with pytest.raises(ShapeError):
        L.measureEPE(img[:, :, :31], 0.5, sites, 25.0)
    with pytest.raises(ShapeError):
        L.measureEPE(img, 0.5, sites[:, :3], 25.0)
    with pytest.raises(ShapeError):
        L.measureEPE(img, 0.5, torch.zeros(2, 4, dtype=torch.int32, device=dev), 25.0)
    with pytest.raises(ShapeError):
        L.measureEPE(img, 0.5, sites.cpu(), 25.0)                                # a tensor on another device
    with pytest.raises(ShapeError):
        L.measureEPE(img, 0.5, sites, 25.0, doses=[1.0] * 65)
    with pytest.raises(ValueError):
        L.measureEPE(img, 0.5, sites, 0.0)
    with pytest.raises(ValueError):
        L.measureEPE(img, 0.5, sites, 25.0, searchRange=33.0)
    with pytest.raises(RuntimeError):
        L.measureEPE(img.cpu(), 0.5, sites.cpu(), 25.0)                          # no CPU fallback
