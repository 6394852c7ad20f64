"""GPU parity of the diffused aerial image (litho_postprocess_resist_diffused) and the sub-pixel edge finder
(litho_measure_cd) against the CPU restatement tests/resist_oracle.py (pinned by closed forms in test_resist_cpu.py).

Bounds are derived, not measured.  Diffused image: D is two passes of a (2R+1)-term fp32 sum of non-negative products --
2 (2R+2) roundings -- plus the fp32 rounding of the taps in either pass and of the product with the gain (+4 with
margin), each at most 2^-24 of the largest value: (2 (2R+2) + 4) 2^-24 max D.  The loader of the fused kernel evaluates
the same bilinear_at as postProcess (same file, no contraction), so its input IS postProcess's image, which earlier tests
pin against the reference; only the diffusion is under test here."""
import math

import numpy as np
import pytest
import torch

import resist_oracle as RO
from helpers import NA, PS, TOL_IMAGE_MAX, WL, f16

pytestmark = pytest.mark.gpu

SIGMAS_NM = (0.0, 10.0, 30.0, 75.0, 200.0)            # R = 0, 2, 5, 12, 32 at 25 nm pixels
U = 2.0 ** -24


def bound_factor(R):
    return (2 * (2 * R + 2) + 4) * U


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    import lithographysimulator_amd as L
    return L


def _eps(pn):
    from oracle import abbe_oracle as O
    return O.calculate_epsilon_n(4 / pn, PS, WL)[0]


def _raw_cases(golden, dev):
    g = golden("g5_images.npz")
    cases = {tag: torch.from_numpy(g[f"{tag}_raw"]).to(dev) for tag in ("demo64", "cfg1_lines", "cfg1_bern")}
    gen = torch.Generator().manual_seed(11)
    cases["random_stack"] = (torch.rand(3, 256, 256, generator=gen) * 4.0).to(dev)
    return cases


@pytest.mark.parametrize("tag", ["demo64", "cfg1_lines", "cfg1_bern", "random_stack"])
def test_diffused_image_and_contour_against_the_restatement(golden, L, dev, tag):
    raw = _raw_cases(golden, dev)[tag]
    eps = _eps(raw.shape[-1])
    plain = L.postProcess(raw, eps)
    I64 = plain.cpu().numpy().astype(np.float64)
    for sigma_nm in SIGMAS_NM:
        R = RO.radius(sigma_nm / PS)
        assert R == {0.0: 0, 10.0: 2, 30.0: 5, 75.0: 12, 200.0: 32}[sigma_nm]
        D64 = RO.diffuse(I64, sigma_nm / PS)
        for dose, frac in ((1.0, 0.3), (0.7, 0.25), (1.3, 0.5)):
            thr = frac * float(D64.max())
            D, resist = L.resistContour(raw, eps, thr, dose=dose, return_image=True, diffusionLength=sigma_nm, pixelSize=PS)
            assert D.shape == plain.shape and resist.shape == plain.shape and resist.dtype == torch.uint8
            if sigma_nm == 0.0:
                img0, res0 = L.resistContour(raw, eps, thr, dose=dose, return_image=True)
                assert torch.equal(D, plain) and torch.equal(D, img0) and torch.equal(resist, res0)
            err = float(np.abs(D.cpu().numpy().astype(np.float64) - D64).max())
            bound = bound_factor(R) * float(D64.max())
            print(f"{tag} sigma {sigma_nm} nm R={R} dose {dose}: max|D_gpu - D_f64| = {err:.3e} = {err / bound:.3f} of the bound")
            assert err <= bound, f"{tag} sigma {sigma_nm} nm (R={R}): max|D_gpu - D_f64| = {err:.3e} = {err / bound:.3f} of the bound {bound:.3e}"
            # the contour is exactly the threshold on the image of the same pass ...
            expect = (D * torch.tensor(dose, dtype=torch.float32, device=dev) >= torch.tensor(thr, dtype=torch.float32, device=dev)).to(torch.uint8)
            assert torch.equal(resist, expect)
            only = L.resistContour(raw, eps, thr, dose=dose, diffusionLength=sigma_nm, pixelSize=PS)     # out = NULL
            assert torch.equal(only, resist)
            # ... and the restatement's, except where the derived bound straddles the threshold
            ref = RO.contour(D64.astype(np.float32), dose, thr)
            assert 0 < int(ref.sum()) < ref.size
            differ = resist.cpu().numpy() != ref
            u64 = D64 * float(np.float32(dose))
            band = bound_factor(R) * float(u64.max())
            assert (np.abs(u64[differ] - float(np.float32(thr))) <= band).all(), (tag, sigma_nm, dose, int(differ.sum()))
            assert int(differ.sum()) <= 1e-4 * ref.size, (tag, sigma_nm, dose, int(differ.sum()))


@pytest.mark.parametrize("sigma_nm", [30.0, 200.0])
def test_diffused_4094_grid_on_sampled_rows_and_columns(L, dev, sigma_nm):
    """pn = 4096 post-processes to n = 4094, a multiple of no tile: the last tile row and column are partial, and the loader
    resamples (the sizes differ) instead of copying.  R = 5, and the widest support R = 32."""
    pn = 4096
    R = RO.radius(sigma_nm / PS)
    eps = _eps(pn)
    gen = torch.Generator().manual_seed(7)
    raw = (torch.rand(pn, pn, generator=gen) * 3.0).to(dev)
    plain = L.postProcess(raw, eps)
    n = plain.shape[-1]
    assert n == 4094
    thr = 1.5
    D, resist = L.resistContour(raw, eps, thr, return_image=True, diffusionLength=sigma_nm, pixelSize=PS)
    assert torch.equal(resist, (D >= thr).to(torch.uint8))
    assert torch.equal(L.resistContour(raw, eps, thr, diffusionLength=sigma_nm, pixelSize=PS), resist)
    D64 = RO.diffuse(plain.cpu().numpy(), sigma_nm / PS)
    Dh = D.cpu().numpy()
    rng = np.random.default_rng(3)
    picks = sorted(set([0, 1, 31, 32, 63, 64, n - 31, n - 30, n - 2, n - 1] + [int(v) for v in rng.integers(0, n, 6)]))
    bound = bound_factor(R) * float(D64.max())
    worst = max(float(np.abs(Dh[picks, :] - D64[picks, :]).max()), float(np.abs(Dh[:, picks] - D64[:, picks]).max()))
    print(f"4094 grid R={R}: max|D_gpu - D_f64| on {len(picks)} rows and columns = {worst:.3e} = {worst / bound:.3f} of the bound")
    assert worst <= bound, f"4094 grid, R={R}: {worst:.3e} = {worst / bound:.3f} of the bound {bound:.3e}"


def test_diffused_entry_limits_and_null_outputs(L, dev):
    """Through the C entry itself: image only (resist = NULL); R = 33, a negative or NaN sigma and two NULL outputs are
    argument errors that write nothing."""
    from lithographysimulator_amd import _native as nat
    pn = 256
    eps = _eps(pn)
    gen = torch.Generator().manual_seed(5)
    raw = (torch.rand(2, pn, pn, generator=gen) * 2.0).to(dev)
    D, resist = L.resistContour(raw, eps, 1.0, return_image=True, diffusionLength=30.0, pixelSize=PS)
    f = nat.lib().litho_postprocess_resist_diffused
    out = torch.full_like(D, -7.0)
    res = torch.full_like(resist, 9)
    st = nat.stream_ptr(dev)
    with torch.cuda.device(dev):
        assert f(nat.ptr(raw), 2, pn, eps, 1.0, 1.0, 30.0 / PS, nat.ptr(out), None, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, D)
        out.fill_(-7.0)
        for sigma in (8.01, -1.0, float("nan"), float("inf")):
            assert f(nat.ptr(raw), 2, pn, eps, 1.0, 1.0, sigma, nat.ptr(out), nat.ptr(res), st) == nat.E_ARG
        assert f(nat.ptr(raw), 2, pn, eps, 1.0, 1.0, 1.2, None, None, st) == nat.E_ARG
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((res == 9).all())
        # sigma = 0 through the new entry: bit for bit the existing pass
        assert f(nat.ptr(raw), 2, pn, eps, 0.7, 1.0, 0.0, nat.ptr(out), nat.ptr(res), st) == 0
        torch.cuda.synchronize()
    img0, res0 = L.resistContour(raw, eps, 1.0, dose=0.7, return_image=True)
    assert torch.equal(out, img0) and torch.equal(res, res0)
    # the widest support (R = 32, more than 64 KiB of LDS) on a stack, after the small launches and before them again
    D32 = L.resistContour(raw, eps, 1.0, return_image=True, diffusionLength=200.0, pixelSize=PS)[0]
    again = L.resistContour(raw, eps, 1.0, return_image=True, diffusionLength=30.0, pixelSize=PS)[0]
    assert torch.equal(again, D) and float(D32.max()) < float(D.max())


@pytest.fixture(scope="module")
def focus_stack(L, dev):
    """The setup of test_bossung_curves_of_a_through_focus_stack: lines_mask(256), circular sigma 0.5 source, five
    aberration-free focal planes -120 .. +120 nm."""
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
    return dict(raw=raw, eps=eps, img=img, n=n, r=r, c_dark=c_dark, c_bright=c_bright, thr=thr)


def _compare_with_oracle(got, image, gauges, doses, thr, exposed, n):
    table, runs, tols = RO.measure_cd(image.cpu().numpy(), gauges, [float(np.float32(d)) for d in doses], thr, exposed, PS)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == table.shape
    assert np.array_equal(np.isnan(got), np.isnan(table))                      # the classification is exact fp32 on both sides
    assert np.array_equal(got[..., 0] == 0.0, table[..., 0] == 0.0)
    pos_tol = 2.0 ** -22 * (n + tols)                                            # pixels: fp32 position + the division's condition
    for k, name in ((1, "x_lo"), (2, "x_hi")):
        fin = ~np.isnan(table[..., k])
        d = np.abs(got[..., k] - table[..., k])[fin]
        print(f"{name}: {int(fin.sum())} finite entries, worst |x_gpu - x_f64| = {float(d.max()):.3e} px = {float((d / pos_tol[..., k - 1][fin]).max()):.3f} of its bound")
        assert (d <= pos_tol[..., k - 1][fin]).all(), (name, float(d.max()), float((d / pos_tol[..., k - 1][fin]).max()))
        assert float(pos_tol[..., k - 1][fin].max()) < 0.01                     # far below a pixel: pins the run [lo, hi] too
        border = fin & (runs[..., k - 1] == (0 if k == 1 else n - 1))
        assert np.array_equal(got[..., k][border], table[..., k][border])       # -0.5 / n - 0.5 exactly
    fin = ~np.isnan(table[..., 1])
    cd_tol = (pos_tol.sum(-1) + 2.0 ** -22 * n) * PS                            # the two positions, the fp32 difference and product
    assert (np.abs(got[..., 0] - table[..., 0])[fin] <= cd_tol[fin]).all()
    for k in (3, 4):                                                            # |b - a|, T * ps, the division: three fp32 roundings
        fin = np.isfinite(table[..., k])
        assert (np.abs(got[..., k] - table[..., k])[fin] <= 4 * U * np.abs(table[..., k])[fin]).all()
    return table, runs


@pytest.mark.parametrize("sigma_nm", [0.0, 30.0])
def test_edge_finder_against_the_restatement_on_the_focus_stack(L, dev, focus_stack, sigma_nm):
    s = focus_stack
    n, r = s["n"], s["r"]
    image = s["img"] if sigma_nm == 0.0 else L.resistContour(s["raw"], s["eps"], s["thr"], return_image=True,
                                                             diffusionLength=sigma_nm, pixelSize=PS)[0]
    gauges = [(r, s["c_dark"], 0), (r, s["c_bright"], 0), (r, s["c_dark"], 1), (r, s["c_bright"], 1),      # lines and spaces,
              (r - 40, s["c_dark"] + 1, 0), (r + 33, s["c_bright"] - 1, 1), (2, n // 2, 0), (n // 2, 1, 1),  # along rows and columns
              (0, 0, 0), (n - 1, n - 1, 1), (r, n - 1, 0),
              (n, 5, 0), (5, -1, 1), (-3, 5, 0), (5, n, 1), (5, 5, 2)]                                        # outside the grid
    doses = [0.8, 1.0, 1.25]
    seen_zero = seen_run = seen_border = 0
    for exposed in (False, True):
        got = L.measureCD(image, s["thr"], gauges, PS, doses=doses, exposed=exposed)
        assert tuple(got.shape) == (3, 5, len(gauges), 5) and got.dtype == torch.float32
        table, runs = _compare_with_oracle(got, image, gauges, doses, s["thr"], exposed, n)
        assert np.isnan(table[:, :, 11:]).all() and bool(torch.isnan(got[:, :, 11:]).all())
        seen_zero += int((table[..., 0] == 0).sum())
        seen_run += int((np.isfinite(table[..., 3]) & np.isfinite(table[..., 4])).sum())
        seen_border += int(((runs[..., 0] == 0) & (runs[..., 1] == n - 1)).sum())
        full = (runs[..., 0] == 0) & (runs[..., 1] == n - 1)
        assert (got.cpu().numpy()[..., 0][full] == np.float32(n * PS)).all()
        # a tensor of gauges on the device, and one 2-D plane, give the same rows
        g_dev = torch.tensor(gauges, dtype=torch.int64, device=dev)
        assert torch.equal(torch.nan_to_num(L.measureCD(image[1], s["thr"], g_dev, PS, doses=doses, exposed=exposed), nan=-1.0),
                           torch.nan_to_num(got[:, 1:2], nan=-1.0))
    assert seen_zero > 20 and seen_run > 20 and seen_border > 5               # every branch of the definition was exercised


def test_measure_cd_on_the_synthetic_v_profile(L, dev):
    n, a, x0, T = 200, 0.5, 120.25, 3.0
    v = (a * (torch.arange(n, dtype=torch.float64) - x0).abs()).to(torch.float32)       # multiples of 1/8: exact
    img = torch.stack([v[None, :].expand(n, n), v[:, None].expand(n, n)]).contiguous().to(dev)
    out = L.measureCD(img, T, [(5, 121, 0), (118, 9, 1), (5, 3, 0), (100, 199, 1)], PS, doses=(1.0, 2.0)).cpu()
    want = torch.tensor([12.0 * PS, x0 - T / a, x0 + T / a, a / (T * PS), a / (T * PS)])
    assert torch.equal(out[0, 0, 0], want) and torch.equal(out[0, 1, 1], want)
    half = torch.tensor([6.0 * PS, x0 - 0.5 * T / a, x0 + 0.5 * T / a, 2 * a / (T * PS), 2 * a / (T * PS)])
    assert torch.equal(out[1, 0, 0], half) and torch.equal(out[1, 1, 1], half)
    assert float(out[0, 0, 2, 0]) == 0.0 and bool(torch.isnan(out[0, 0, 2, 1:]).all())   # u = 58.6 >= T: not an unexposed sample
    assert float(out[0, 0, 1, 0]) == 0.0                                                   # plane 0 is constant along a column
    # the exposed side runs from the crossing to the border
    ex = L.measureCD(img, T, [(7, 150, 0)], PS, exposed=True).cpu()[0, 0, 0]
    assert float(ex[1]) == x0 + T / a and float(ex[2]) == n - 0.5 and math.isnan(float(ex[4])) and float(ex[3]) == float(np.float32(a / (T * PS)))
    assert float(ex[0]) == (n - 0.5 - (x0 + T / a)) * PS


def test_subpixel_bossung_curves_are_consistent_with_the_pixel_table(L, dev, focus_stack):
    s = focus_stack
    raw, eps, thr, r, n = s["raw"], s["eps"], s["thr"], s["r"], s["n"]
    doses = [0.8, 1.0, 1.25]
    for sigma_nm in (0.0, 30.0):
        image = s["img"] if sigma_nm == 0.0 else L.resistContour(raw, eps, thr, return_image=True, diffusionLength=sigma_nm,
                                                                 pixelSize=PS)[0]
        for col, exposed in ((s["c_dark"], False), (s["c_bright"], True)):
            pix = L.bossungCurves(raw, eps, thr, doses, PS, row=r, column=col, exposed=exposed, diffusionLength=sigma_nm).cpu()
            sub = L.bossungCurves(raw, eps, thr, doses, PS, row=r, column=col, exposed=exposed, subpixel=True,
                                  diffusionLength=sigma_nm).cpu()
            assert tuple(sub.shape) == tuple(pix.shape) == (3, 5) and sub.dtype == torch.float32
            full = L.measureCD(image, thr, [(r, col, 0)], PS, doses=doses, exposed=exposed).cpu()
            assert torch.equal(sub, full[:, :, 0, 0])
            assert bool(((sub - pix).abs() <= PS).all()), (sigma_nm, exposed, sub, pix)
            assert bool(((sub == 0) == (pix == 0)).all())
            if sigma_nm == 0.0:
                assert torch.equal(pix, L.bossungCurves(raw, eps, thr, doses, PS, row=r, column=col, exposed=exposed).cpu())
            # symmetric in focus (I(+z) = I(-z) for a real mask and an aberration-free pupil): the two planes are each within
            # TOL_IMAGE_MAX * max of the exact image, an edge moves by du / |du/dx| = du / (ils * T) nm, two edges per CD
            peak = float(image.max())
            for di, dose in enumerate(doses):
                for pa, pb in ((0, 4), (1, 3)):
                    if float(sub[di, pa]) == 0.0 or float(sub[di, pb]) == 0.0:
                        assert float(sub[di, pa]) == float(sub[di, pb])
                        continue
                    ils = min(float(full[di, p, 0, k]) for p in (pa, pb) for k in (3, 4))
                    tol = 2 * 2 * TOL_IMAGE_MAX * peak * dose / (ils * thr)
                    assert abs(float(sub[di, pa]) - float(sub[di, pb])) <= tol, (sigma_nm, dose, pa, pb, sub, tol)
    # the point of the feature: at nominal dose the pixel table cannot tell the focal planes of the line apart, the
    # sub-pixel table orders them as the restatement does -- 0 < +-60 < +-120 nm
    col = s["c_dark"]
    pix = L.bossungCurves(raw, eps, thr, [1.0], PS, row=r, column=col).cpu()[0]
    sub = L.bossungCurves(raw, eps, thr, [1.0], PS, row=r, column=col, subpixel=True).cpu()[0]
    ref = RO.measure_cd(s["img"].cpu().numpy(), [(r, col, 0)], [1.0], thr, False, PS)[0][0, :, 0, 0]
    assert float(pix[2]) == float(pix[3]) == float(pix[4]) > 0
    assert ref[2] < ref[3] < ref[4] and float(sub[2]) < float(sub[3]) < float(sub[4])
    assert ref[2] < ref[1] < ref[0] and float(sub[2]) < float(sub[1]) < float(sub[0])
    print("pixel CD", pix.tolist(), "sub-pixel CD", sub.tolist(), "restatement", ref.tolist())
