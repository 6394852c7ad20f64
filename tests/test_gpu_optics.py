"""GPU parity for the source-sampling, pupil, post-process and mask-spectrum kernels."""
import hashlib
import math

import numpy as np
import pytest
import torch

from helpers import (NA, PS, PUPIL_CASES, SOURCE_CASES, TOL_IMAGE_MAX, TOL_PHI, WL, f16, g18_focus_cases, g18_large_source_cases,
                     g18_pupil_cases, g18_source_cases, g18_support, rel_max, sha256_packed, unpack_bitmap)

pytestmark = pytest.mark.gpu

# fp16 wavefront: the HIP kernel evaluates atan2/cos/sin/pow correctly rounded in fp32, torch-CPU uses SLEEF
# (<= 1 ulp), so a flipped fp16 rounding was budgeted for (<= 1e-5 of pixels).  OBSERVED on MI355X
# (scripts/parity_probe.py, profiles/r02_parity_probe.txt): 0 mismatching pixels in all 14 pupil cases, 0 flipped
# source pixels in all 10 large bitmaps -- so the tests assert exact equality.


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    import lithographysimulator_amd as L
    return L


def _source(L, dev, pn, kind, sin, sout, sx=0.0, sy=0.0, count=4, rot=-math.pi / 8):
    ls = L.LightSource(sin, sout, pn, NA, sx, sy, dev)
    return ls.generateAnnular() if kind == "annular" else ls.generateQuasar(count, rot)


@pytest.mark.parametrize("pn", [64, 256])
@pytest.mark.parametrize("name", list(SOURCE_CASES))
def test_source_lists_exact(golden, L, dev, pn, name):
    g = golden("g1_sources.npz")
    bm = _source(L, dev, pn, **SOURCE_CASES[name])
    assert bm.dtype == torch.int64 and tuple(bm.shape) == (pn, pn)
    got = L.sourceShifts(bm, pn).cpu().numpy()
    assert got.dtype == np.int32
    assert np.array_equal(got, g[f"shifts_{name}_{pn}"])


@pytest.mark.parametrize("pn", [1024, 2048])
@pytest.mark.parametrize("name", list(SOURCE_CASES))
def test_source_bitmaps_large(golden, L, dev, pn, name):
    g = golden("g1_sources.npz")
    bm = _source(L, dev, pn, **SOURCE_CASES[name]).cpu().numpy()
    ref = unpack_bitmap(g[f"packed_{name}_{pn}"], pn)
    # bit exact, quasar wedges (fp16 angle from atan2) included: 0 flips observed, 0 allowed
    flips = int((bm != ref).sum())
    assert flips == 0, f"{flips} source pixels differ from the reference"
    assert np.array_equal(sha256_packed(bm), g[f"sha256_{name}_{pn}"])


def test_source_4096_counts(golden, L, dev):
    g = golden("g1_sources.npz")
    bm = _source(L, dev, 4096, **SOURCE_CASES["annular"])
    assert int(bm.sum()) == 1581616
    assert np.array_equal(sha256_packed(bm.cpu().numpy()), g["sha256_annular_4096"])
    assert L.sourceShifts(bm, 4096).shape == (1581616, 2)


def test_source_compaction_edge_cases(L, dev):
    pn = 64
    empty = torch.zeros((pn, pn), dtype=torch.int64, device=dev)
    assert L.sourceShifts(empty, pn).shape == (0, 2)
    full = torch.ones((pn, pn), dtype=torch.int64, device=dev)
    sh = L.sourceShifts(full, pn).cpu()
    assert torch.equal(sh, (torch.argwhere(full.cpu()) - pn // 2).to(torch.int32))
    with pytest.raises(ValueError):
        L.sourceShifts(torch.ones((32, 32), dtype=torch.int64, device=dev), pn)


@pytest.mark.parametrize("pn", [2, 62, 1000, 4096, 4098, 8192])
def test_source_compaction_on_both_sides_of_the_fused_scan(L, dev, pn):
    """litho_source_compact runs two launches up to pn = 4096 (the row-offset scan folded into the write, round 6) and three
    above: random sparse bitmaps (empty rows, full rows, first / last pixel lit) against torch.argwhere (imageformation.py:59) on
    both sides of the switch, with the device-side count of the asynchronous form."""
    gen = torch.Generator().manual_seed(pn)
    bm = (torch.rand(pn, pn, generator=gen) < (0.3 if pn <= 1000 else 0.002)).to(torch.int64)
    bm[0, 0] = 1; bm[pn - 1, pn - 1] = 1
    if pn >= 62:
        bm[5] = 0; bm[7] = 1; bm[pn - 2] = 0
    want = (torch.argwhere(bm) - pn // 2).to(torch.int32)
    got = L.sourceShifts(bm.to(dev), pn)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    from lithographysimulator_amd.lightsource import sourceShiftsAsync
    sh, count = sourceShiftsAsync(bm.to(dev), pn)
    assert int(count.item()) == want.shape[0] and torch.equal(sh[:want.shape[0]].cpu(), want)


@pytest.mark.parametrize("pn", [64, 256])
@pytest.mark.parametrize("name", list(PUPIL_CASES))
def test_pupils(golden, L, dev, pn, name):
    g = golden("g2_pupils.npz")
    ab = PUPIL_CASES[name]
    p = L.Pupil(pn, WL, NA, None if ab is None else f16(ab), dev)
    W = p.generateWavefrontError().real.to(torch.float16).cpu()
    Wref = torch.from_numpy(g[f"W_{name}_{pn}"]).view(torch.float16)
    mism = int((W != Wref).sum())
    assert mism == 0, f"{mism} of {pn * pn} fp16 wavefront values differ from the reference"
    p2 = L.Pupil(pn, WL, NA, None if ab is None else f16(ab), dev)
    phi = p2.generatePupilFunction().cpu()
    ref = torch.from_numpy(g[f"phi_{name}_{pn}"])
    assert torch.equal(phi != 0, ref != 0)
    assert float((phi - ref).abs().max()) < TOL_PHI               # EVERY pixel (observed: <= 6e-8)


def test_pupil_mutates_callers_coefficients_like_reference(L, dev):
    ab = f16([0, 0, 0.01, 0, 100, 0.01, 0, 0.01, 0.01, 0.01])
    L.Pupil(64, WL, NA, ab, dev).generatePupilFunction()
    assert abs(float(ab[4]) - 0.0635) < 1e-4                     # 100 -> 0.0635


def test_pupil_length4_raises(L, dev):
    with pytest.raises(IndexError):
        L.Pupil(64, WL, NA, f16([0, 0, 0, 1]), dev).generatePupilFunction()


@pytest.mark.parametrize("pn", [1024, 2048])
def test_pupil_large(golden, L, dev, pn):
    g = golden("g2_pupils.npz")
    for name in ("ideal", "defocus_p100", "demo"):
        ab = PUPIL_CASES[name]
        phi = L.Pupil(pn, WL, NA, None if ab is None else f16(ab), dev).generatePupilFunction().cpu()
        assert int((phi != 0).sum()) == int(g[f"nz_{name}_{pn}"])
        sub = phi[::16, ::16]
        ref = torch.from_numpy(g[f"phisub_{name}_{pn}"])
        assert float((sub - ref).abs().max()) < TOL_PHI           # every sample (0 outliers observed)


@pytest.mark.parametrize("pn", [64, 256])
def test_pupil_stack_vs_golden(golden, L, dev, pn):
    """litho_pupil_stack: the planes of ONE launch against the reference-made single pupils of g2 -- the
    defocus-only vectors [0,0,0,0,d] as three planes of one stack, and the demo vector as a one-plane stack: fp16 W
    bit-exact, phi on every pixel."""
    g = golden("g2_pupils.npz")
    W, phi = L.throughFocusPupils(pn, WL, NA, f16([0, 0, 0, 0, 7]), [100.0, -200.0, 30.0], dev, wavefront=True)
    assert tuple(phi.shape) == (3, pn, pn) and phi.dtype == torch.complex64 and W.dtype == torch.float16
    for p, name in enumerate(("defocus_p100", "defocus_m200", "defocus_p30")):
        Wref = torch.from_numpy(g[f"W_{name}_{pn}"]).view(torch.float16)
        assert int((W[p].cpu() != Wref).sum()) == 0, name
        ref = torch.from_numpy(g[f"phi_{name}_{pn}"])
        assert torch.equal(phi[p].cpu() != 0, ref != 0) and float((phi[p].cpu() - ref).abs().max()) < TOL_PHI
    ab = f16(PUPIL_CASES["demo"])
    before = ab.clone()
    W, phi = L.throughFocusPupils(pn, WL, NA, ab, [float(PUPIL_CASES["demo"][4])], dev, wavefront=True)
    assert torch.equal(ab, before)                               # the reference's loop works on clones: caller's vector untouched
    assert int((W[0].cpu() != torch.from_numpy(g[f"W_demo_{pn}"]).view(torch.float16)).sum()) == 0
    assert float((phi[0].cpu() - torch.from_numpy(g[f"phi_demo_{pn}"])).abs().max()) < TOL_PHI


@pytest.mark.parametrize("pn,J,planes", [(64, 5, 1), (64, 10, 70), (256, 15, 9), (64, 40, 3), (2048, 10, 32)])
def test_pupil_stack_equals_single_plane_launches(L, dev, pn, J, planes):
    """One stacked launch (per 64 planes) = `planes` litho_pupil calls, bit for bit in W AND phi: every term count (5 = the
    defocus term is the last, 15, 40 = beyond the 32 terms that travel in the kernel arguments), more planes than one launch
    holds (70), and config 5 at its size (2048^2 x 32 planes, defocus -310 .. 310 nm, demo vector)."""
    gen = torch.Generator().manual_seed(100 * J + planes)
    ab = PUPIL_CASES["demo"] if J == 10 else [0.0, 0.0] + [float(v) for v in (torch.rand(J - 2, generator=gen) * 0.04 - 0.02)]
    defocus = [-310.0 + 20.0 * k for k in range(32)] if planes == 32 else [float(v) for v in (torch.rand(planes, generator=gen) * 600 - 300)]
    W, phi = L.throughFocusPupils(pn, WL, NA, f16(ab), defocus, dev, wavefront=True)
    assert tuple(W.shape) == tuple(phi.shape) == (planes, pn, pn)
    for p in (range(planes) if pn < 2048 else (0, 13, 31)):
        one = f16(ab).clone()
        one[4] = defocus[p]
        W1 = L.Pupil(pn, WL, NA, one.clone(), dev).generateWavefrontError().real.to(torch.float16)
        phi1 = L.Pupil(pn, WL, NA, one.clone(), dev).generatePupilFunction()
        assert torch.equal(W[p].view(torch.int16), W1.view(torch.int16)), p
        assert torch.equal(torch.view_as_real(phi[p]), torch.view_as_real(phi1)), p
    if pn == 2048:                                               # every plane of config 5's stack has the ideal pupil's support
        assert [int(v) for v in (phi != 0).flatten(1).sum(1).cpu()] == [int((phi[0] != 0).sum())] * planes


def test_pupil_stack_short_vector_raises(L, dev):
    with pytest.raises(IndexError):
        L.throughFocusPupils(64, WL, NA, f16([0, 0, 0, 1]), [10.0], dev)
    with pytest.raises(ValueError):
        L.throughFocusPupils(64, WL, NA, f16([0, 0, 0, 0, 1]), [], dev)


def test_generate_phi_and_z(L, dev):
    from oracle import abbe_oracle as O
    W = O.wavefront_error(f16(PUPIL_CASES["demo"]), 64, NA, WL)
    phi = L.generatePhi(W.to(torch.complex64).to(dev), 64, dev).cpu()
    assert float((phi - O.pupil_from_wavefront(W, 64)).abs().max()) < TOL_PHI
    Z = L.generateZ(1, 3, 64, 0.5, dev).cpu().float()
    Zref = O.zernike_term(1, 3, 64, torch.tensor(0.5))
    assert int((Z != Zref).sum()) == 0


@pytest.mark.parametrize("key", ["demo_64_ps25", "bern_64_ps25", "lines_64_ps25", "bern_256_ps25", "lines_256_ps25",
                                 "bern_64_ps48", "bern_64_ps10", "bern_128_ps25", "bern_96_ps25"])
def test_mask_spectrum_vs_golden(golden, L, dev, key):
    from lithographysimulator_amd.synthetic import bernoulli_mask, lines_mask
    g = golden("g3_mask_spectra.npz")
    kind, pn, ps = key.split("_"); pn = int(pn); ps = int(ps[2:])
    geo = None if kind == "demo" else (bernoulli_mask(pn) if kind == "bern" else lines_mask(pn))
    mask = L.Mask(geo, ps, dev)
    eps, N = mask.calculateEpsilonN(mask.deltaK, ps, WL)
    assert [eps, N] == list(g[f"epsN_{key}"])
    assert rel_max(mask.fraunhofer(WL, True).cpu(), torch.from_numpy(g[f"spec_{key}"])) < 2e-6


def test_mask_spectrum_scaled_mask_larger_than_n(L, dev):
    """pixelSize 64: epsilon = 1.33 and N = pn, the scaled mask is CROPPED to N (negative pad)."""
    from oracle import abbe_oracle as O
    from lithographysimulator_amd.synthetic import bernoulli_mask
    geo = bernoulli_mask(64)
    got = L.Mask(geo, 64, dev).fraunhofer(WL, True).cpu()
    assert rel_max(got, O.mask_spectrum(geo, 64, WL)) < 2e-6


def test_sizing_table(golden, L):
    for pn, ps, eps, N in golden("g3_mask_spectra.npz")["sizing_table"]:
        m = L.Mask.__new__(L.Mask)
        e, n = L.Mask.calculateEpsilonN(m, 4 / pn, ps, WL)
        assert n == int(N) and e == eps


@pytest.mark.parametrize("pn", [64, 256, 1024, 2048, 4096])
def test_postprocess_vs_oracle(L, dev, pn):
    from oracle import abbe_oracle as O
    eps, N = O.calculate_epsilon_n(4 / pn, PS, WL)
    gen = torch.Generator().manual_seed(pn)
    raw = torch.rand(pn, pn, generator=gen) * 1e12
    got = L.postProcess(raw.to(dev), eps).cpu()
    ref = O.post_process(raw, eps)
    assert got.shape == ref.shape
    assert rel_max(got, ref) < 1e-6


@pytest.mark.parametrize("ps", [48, 64, 10])
def test_postprocess_other_epsilons(L, dev, ps):
    from oracle import abbe_oracle as O
    eps, N = O.calculate_epsilon_n(4 / 64, ps, WL)
    raw = torch.rand(64, 64, generator=torch.Generator().manual_seed(ps))
    got = L.postProcess(-raw.to(dev), eps).cpu()            # abs() is part of the post-process
    ref = O.post_process(raw, eps)
    assert got.shape == ref.shape and rel_max(got, ref) < 1e-6


@pytest.mark.parametrize("pn", [4096, 8192])
def test_pupil_support_at_large_sizes(golden, L, dev, pn):
    """pn = 8192: the reference's fp16 sigma grid is coarser than its own step, its r <= 1 support is 4099 wide
    (golden g8); the HIP kernel's 16-lane arange recipe has to land on exactly the same pixels."""
    g = golden("g8_large_pupils.npz")
    for name, ab in (("ideal", None), ("defocus_p100", [0, 0, 0, 0, 100])):
        phi = L.Pupil(pn, WL, NA, None if ab is None else f16(ab), dev).generatePupilFunction()
        nz = phi != 0
        assert int(nz.sum()) == int(g[f"nz_{name}_{pn}"])
        assert np.array_equal(nz.sum(1).to(torch.int32).cpu().numpy(), g[f"rowcount_{name}_{pn}"])
        rows = torch.nonzero(nz.any(1)).flatten(); cols = torch.nonzero(nz.any(0)).flatten()
        assert [int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])] == list(g[f"box_{name}_{pn}"])
        sub = phi[::64, ::64].cpu()
        assert float((sub - torch.from_numpy(g[f"phisub_{name}_{pn}"])).abs().max()) < TOL_PHI


@pytest.mark.parametrize("tag", ["demo64", "cfg1_bern", "cfg1_lines"])
def test_resist_threshold_on_golden_images(golden, L, dev, tag):
    """The constant-threshold resist model fused into the post-process pass (the reference's README lists photoresist
    response as an open goal; the definition is ours): resist = (dose * image >= threshold) as uint8 -- a three-line
    torch expression on the image of the same pass (exact), and on the REFERENCE's own final image (identical except
    where an fp32 rounding of the resampling straddles the threshold)."""
    g = golden("g5_images.npz")
    raw = torch.from_numpy(g[f"{tag}_raw"]).to(dev)
    ref_final = torch.from_numpy(g[f"{tag}_final"])
    pn = raw.shape[0]
    from oracle import abbe_oracle as O
    eps, N = O.calculate_epsilon_n(4 / pn, PS, WL)
    S = {"demo64": 184, "cfg1_bern": 3233, "cfg1_lines": 3233}[tag]
    for dose, frac in ((1.0, 0.3), (0.7, 0.25), (1.0 / S, None)):
        thr = (0.3 if frac is None else frac) * float(ref_final.max()) * (dose if frac is None else 1.0)
        image, resist = L.resistContour(raw, eps, thr, dose=dose, return_image=True)
        assert resist.dtype == torch.uint8 and resist.shape == image.shape == ref_final.shape
        assert rel_max(image.cpu(), ref_final) < TOL_IMAGE_MAX                  # the image of the same pass is the post-processed one
        expect = (image * torch.tensor(dose, dtype=torch.float32, device=dev) >= torch.tensor(thr, dtype=torch.float32, device=dev)).to(torch.uint8)
        assert torch.equal(resist, expect)
        only = L.resistContour(raw, eps, thr, dose=dose)                       # contour only: no image written
        assert torch.equal(only, resist)
        ref_mask = (ref_final * np.float32(dose) >= np.float32(thr)).to(torch.uint8)
        flips = int((resist.cpu() != ref_mask).sum())
        assert 0 < int(ref_mask.sum()) < ref_mask.numel() and flips <= max(2, ref_mask.numel() // 20000), (flips, int(ref_mask.sum()))


def test_resist_threshold_stack_and_edges(L, dev):
    """A 3-plane stack; threshold 0 (everything prints, the zero-padded border included), an unreachable threshold
    (nothing prints), and a negative raw image (abs() is part of the post-process)."""
    from oracle import abbe_oracle as O
    pn = 256
    eps, N = O.calculate_epsilon_n(4 / pn, PS, WL)
    gen = torch.Generator().manual_seed(3)
    raw = (torch.rand(3, pn, pn, generator=gen) * 5.0).to(dev)
    img, res = L.resistContour(-raw, eps, 2.5, dose=1.0, return_image=True)
    assert res.shape == img.shape == (3, pn, pn)
    assert torch.equal(res, (img >= 2.5).to(torch.uint8)) and rel_max(img.cpu(), torch.stack([O.post_process(r.cpu(), eps) for r in raw])) < 1e-6
    assert int(L.resistContour(raw, eps, 0.0).sum()) == 3 * pn * pn
    assert int(L.resistContour(raw, eps, 1e30).sum()) == 0


def test_bossung_curves_of_a_through_focus_stack(L, dev):
    """Process-window table (no reference counterpart): a 5-plane stack of a line/space mask.  The CD table must equal a
    plain per-plane, per-dose measurement on resistContour, widen with... dose for an exposed feature and shrink for an
    unexposed one, and be symmetric in focus for an aberration-free pupil (I(+z) = I(-z) for a real mask)."""
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
    row = img[2, r]                                               # best focus, centre row
    c_dark = int(torch.argmin(row[n // 4: 3 * n // 4])) + n // 4    # the middle of a line (dark), of a space (bright)
    c_bright = int(torch.argmax(row[n // 4: 3 * n // 4])) + n // 4
    thr = 0.5 * float(row[c_dark] + row[c_bright])
    doses = [0.8, 1.0, 1.25]
    dark = L.bossungCurves(raw, eps, thr, doses, PS, row=r, column=c_dark).cpu()
    bright = L.bossungCurves(raw, eps, thr, doses, PS, row=r, column=c_bright, exposed=True).cpu()
    assert tuple(dark.shape) == (3, 5) == tuple(bright.shape)
    for di, dose in enumerate(doses):                             # the same numbers by hand
        con = L.resistContour(raw, eps, thr, dose=dose).cpu()
        for p in range(5):
            line = con[p, r].tolist()
            for col, want, table in ((c_dark, 0, dark), (c_bright, 1, bright)):
                if line[col] != want:
                    assert table[di, p] == 0
                    continue
                lo = col
                while lo > 0 and line[lo - 1] == want:
                    lo -= 1
                hi = col
                while hi < n - 1 and line[hi + 1] == want:
                    hi += 1
                assert float(table[di, p]) == (hi - lo + 1) * PS, (dose, p, col)
    assert float(dark[1, 2]) > 0 and float(bright[1, 2]) > 0      # both features print at best focus and nominal dose
    assert bool((dark[0] >= dark[1]).all()) and bool((dark[1] >= dark[2]).all())        # more dose: unexposed lines shrink
    assert bool((bright[0] <= bright[1]).all()) and bool((bright[1] <= bright[2]).all())  # ... exposed spaces widen
    assert torch.equal(dark[:, 0], dark[:, 4]) and torch.equal(dark[:, 1], dark[:, 3])  # symmetric through focus


# ---------------------------------------------------------------- golden g18: off the demo grids, fixture only
def _report(bad, total, what):
    assert not bad, f"{len(bad)} of {total} {what} differ from the reference:\n  " + "\n  ".join(bad[:40])


def _ordered(bits16):
    """fp16 bit patterns -> integers in value order (adjacent values differ by one)."""
    b = bits16.to(torch.int32) & 0xFFFF
    return torch.where(b < 0x8000, b, 0x8000 - b)


def _w_mismatches(W, Wref):
    """(values that differ bit for bit, those of them that are NOT exactly one fp16 ulp away)."""
    a, b = W.cpu().view(torch.int16), Wref.view(torch.int16)
    diff = a != b
    far = diff & ((_ordered(a) - _ordered(b)).abs() != 1)
    return int(diff.sum()), int(far.sum())


def _phi_f64(W16):
    """exp(i 2 pi W) with the exponential in float64.  Its ARGUMENT is the reference's: pupil.py:103 multiplies the
    complex64 W by the Python scalar 1j*2*pi, i.e. by fp32(2 pi) with one fp32 rounding of the product, and that rounding
    belongs to the operation, not to the kernel's error (for |W| = 5 it alone moves phi by 3e-6)."""
    ang = (torch.tensor(2 * math.pi, dtype=torch.float32) * W16.to(torch.float32)).double()
    return torch.complex(torch.cos(ang), torch.sin(ang))


@pytest.mark.parametrize("pn", [14, 30, 46, 62, 100, 118])
def test_g18_source_bitmaps_and_lists(golden, L, dev, pn):
    """k_source_bitmap and the compaction at sizes that are no multiple of 32 (the axis' scalar tail, lit at 30 and 62), four
    shifts of which three are not fp16 numbers, wedge counts 1 .. 64, rotations beyond +-2 pi: 264 bitmaps per size, every
    pixel, and sourceShifts = argwhere - pn // 2 of the golden bitmap."""
    g = golden("g18_optics_sweep.npz")
    bad, total = [], 0
    for label, sin, sout, sx, sy, count, rot, ref in g18_source_cases(g, pn):
        ls = L.LightSource(sin, sout, pn, NA, sx, sy, dev)
        bm = ls.generateAnnular() if count is None else ls.generateQuasar(count, rot)
        total += 1
        flips = int((bm.cpu().numpy() != ref).sum())
        want = np.argwhere(ref).astype(np.int32) - pn // 2
        lists_equal = np.array_equal(L.sourceShifts(bm, pn).cpu().numpy(), want)
        if flips or not lists_equal:
            bad.append(f"{label}: {flips} pixels{'' if lists_equal else ', source list differs'}")
    print(f"g18 sources pn {pn}: {len(bad)} of {total} differ")
    _report(bad, total, f"source cases at pn {pn}")


def test_g18_source_bitmaps_large(golden, L, dev):
    """200, 502, 1000 and 3000, centred and shifted by (-0.37, 0.41): lit count, every row count, sha256 of the packed bits;
    the source list against argwhere of the bitmap the hash has just identified with the reference's."""
    g = golden("g18_optics_sweep.npz")
    bad, total = [], 0
    for key, pn, kind, sx, sy in g18_large_source_cases(g):
        bm_dev = _source(L, dev, pn, kind, 0.4, 0.8, sx, sy)
        bm = bm_dev.cpu().numpy()
        total += 1
        rows = int((bm.sum(1).astype(np.int32) != g[f"{key}_rows"]).sum())
        same = np.array_equal(sha256_packed(bm), g[f"{key}_sha256"])
        lists_equal = np.array_equal(L.sourceShifts(bm_dev, pn).cpu().numpy(), np.argwhere(bm).astype(np.int32) - pn // 2)
        if int(bm.sum()) != int(g[f"{key}_count"]) or rows or not same or not lists_equal:
            bad.append(f"{key}: count {int(bm.sum())} vs {int(g[f'{key}_count'])}, {rows} row counts differ, "
                       f"sha256 {'equal' if same else 'differs'}, list {'equal' if lists_equal else 'differs'}")
    print(f"g18 large sources: {len(bad)} of {total} differ")
    _report(bad, total, "large source cases")


def test_g18_pupils(golden, L, dev):
    """k_pupil_packed (J <= 32) and k_pupil with its staged table (J = 36, 45, 66 -- that path's first comparison with the
    reference) at pn 14 .. 256, four (NA, wavelength) pairs, fp16-subnormal products, a 900 nm defocus and a vector too
    short for the defocus rescale: fp16 W, the r <= 1 support, and phi against exp(i 2 pi W_golden) in float64.

    W: the reference and the oracle agree on all of these on the CPU, so a difference is the kernel's.  The only legitimate
    one is a flipped fp16 rounding after atan2 / cos / sin / pow (correctly rounded here, SLEEF within 1 ulp there), budgeted
    in SURVEY 8c at 1e-5 of the pixels compared, each exactly one fp16 ulp away.  OBSERVED on MI355X: 0 of 531,468 values in
    153 cases -- so 0 is asserted."""
    g = golden("g18_optics_sweep.npz")
    bad, total, pixels, mism_total, worst = [], 0, 0, 0, 0.0
    for label, pn, na, lam, vec, Wref in g18_pupil_cases(g):
        W = L.Pupil(pn, lam, na, vec.clone(), dev).generateWavefrontError().real.to(torch.float16)
        phi = L.Pupil(pn, lam, na, vec.clone(), dev).generatePupilFunction().cpu()
        total += 1
        pixels += pn * pn
        mism, far = _w_mismatches(W, Wref)
        mism_total += mism
        support = torch.from_numpy(g18_support(g, pn))
        flips = int(((phi != 0) != support).sum())
        want = torch.where(support, _phi_f64(Wref), torch.zeros((), dtype=torch.complex128))
        err = float((phi.to(torch.complex128) - want).abs().max())
        worst = max(worst, err)
        if mism or flips or not err < TOL_PHI:
            bad.append(f"{label}: {mism} W values ({far} by more than one ulp), {flips} support pixels, phi error {err:.2e}")
    print(f"g18 pupils: {len(bad)} of {total} cases differ; {mism_total} of {pixels} fp16 W values; worst phi error {worst:.2e}")
    _report(bad, total, "pupil cases")
    assert mism_total == 0


def test_g18_through_focus(golden, L, dev):
    """throughFocusPupils at defocus -500, -33, 0.5 and 250 nm on a 28-term vector (k_pupil_stack) and a 36-term one (plane by
    plane through the staged table), at (NA, wavelength) = (0.33, 13.5) and (1.35, 193), pn 30 and 64: every plane bit-identical
    in W and phi to the single Pupil call with that defocus, whose W is the reference's (one golden W per plane)."""
    g = golden("g18_optics_sweep.npz")
    defocus = [float(d) for d in g["tf_defocus"]]
    bad, total = [], 0
    for label, pn, na, lam, vec, Wref in g18_focus_cases(g):
        before = vec.clone()
        W, phi = L.throughFocusPupils(pn, lam, na, vec, defocus, dev, wavefront=True)
        assert torch.equal(vec, before) and tuple(W.shape) == tuple(phi.shape) == (len(defocus), pn, pn)
        for p, d in enumerate(defocus):
            ab = vec.clone()
            ab[4] = d
            W1 = L.Pupil(pn, lam, na, ab.clone(), dev).generateWavefrontError().real.to(torch.float16)
            phi1 = L.Pupil(pn, lam, na, ab.clone(), dev).generatePupilFunction()
            total += 1
            mism, _ = _w_mismatches(W1, Wref[p])
            same_w = torch.equal(W[p].view(torch.int16), W1.view(torch.int16))
            same_phi = torch.equal(torch.view_as_real(phi[p]), torch.view_as_real(phi1))
            if mism or not same_w or not same_phi:
                bad.append(f"{label} defocus {d}: single call {mism} W values off the reference, stack W "
                           f"{'equal' if same_w else 'differs'}, stack phi {'equal' if same_phi else 'differs'}")
    print(f"g18 through focus: {len(bad)} of {total} planes differ")
    _report(bad, total, "through-focus planes")


@pytest.mark.parametrize("pn", [30, 100])
def test_g18_generate_phi_complex_wavefront(golden, L, dev, pn):
    """k_pupil_phase on a wavefront with a non-zero imaginary part (an absorbing pupil): exp(-2 pi Im) (cos, sin)(2 pi Re),
    evaluated in float64 on the golden support, zero outside.  The arguments are the reference's fp32 products with
    fp32(2 pi) (see _phi_f64); what remains is three fp32 roundings (magnitude, cos / sin, product) of 6e-8 relative each,
    inside TOL_PHI scaled by the magnitude."""
    g = golden("g18_optics_sweep.npz")
    gen = torch.Generator().manual_seed(pn)
    re = (torch.rand(pn, pn, generator=gen) - 0.5).to(torch.float32)
    im = ((torch.rand(pn, pn, generator=gen) - 0.5) * 0.6).to(torch.float32)
    phi = L.generatePhi(torch.complex(re, im).to(dev), pn, dev).cpu().to(torch.complex128)
    support = torch.from_numpy(g18_support(g, pn))
    twopi = torch.tensor(2 * math.pi, dtype=torch.float32)
    mag = torch.exp(-(twopi * im).double())
    ang = (twopi * re).double()
    want = torch.where(support, mag * torch.complex(torch.cos(ang), torch.sin(ang)), torch.zeros((), dtype=torch.complex128))
    assert torch.equal(phi != 0, support)
    rel = float(((phi - want).abs() / torch.where(support, mag, torch.ones_like(mag))).max())
    print(f"g18 generatePhi pn {pn}: worst error / magnitude {rel:.2e}, magnitudes {float(mag.min()):.2f} .. {float(mag.max()):.2f}")
    assert rel < TOL_PHI
