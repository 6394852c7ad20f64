"""GPU checks of the complex-transmission (phase-shift / grey) mask: litho_mask_spectrum_complex behind
`Mask(transmission=...)`, the two mask helpers, and the GDSII composition.

The reference has no complex mask, so the oracle is its own chain (oracle.abbe_oracle.mask_spectrum, mask.py:74-90) applied
to the real and to the imaginary part: every step of the chain is linear, spectrum(t) = S(Re t) + i S(Im t)."""
import math

import numpy as np
import pytest
import torch

from helpers import DEMO_AB, NA, PS, TOL_IMAGE_L2, TOL_IMAGE_MAX, WL, f16, rel_l2, rel_max, subsample_bitmap

pytestmark = pytest.mark.gpu

# (pn, pixelSize, wavelength): N = 128, up-scaled and padded | N = pn, the scaled mask cropped | epsilon = 1, the copy
# branch | N = 512
SIZES_IDENTITY = [(64, 25, 193.0), (64, 64, 193.0), (64, 25, 200.0), (256, 25, 193.0)]
# ... | pn no multiple of 64 (N = 256) | N = 2048
SIZES_ORACLE = SIZES_IDENTITY + [(96, 25, 193.0), (1024, 25, 193.0)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    import lithographysimulator_amd as L
    return L


def oracle_spectrum(t, ps, wl):
    """S(Re t) + i S(Im t) with the oracle's real chain."""
    from oracle import abbe_oracle as O
    t = t.cpu()
    return O.mask_spectrum(t.real.contiguous(), ps, wl) + 1j * O.mask_spectrum(t.imag.contiguous(), ps, wl)


def footprint(pn, kind):
    from lithographysimulator_amd.synthetic import bernoulli_mask, lines_mask
    return lines_mask(pn) if kind == "lines" else bernoulli_mask(pn)


def transmission(L, pn, kind):
    """The four transmissions of the oracle test.  lines_mask needs pn % 64 == 0: Bernoulli footprints at 96."""
    lines = "lines" if pn % 64 == 0 else "bern"
    if kind == "attenuated":                                   # 6 % / pi
        return L.attenuatedPSM(footprint(pn, lines))
    if kind == "alternating":                                  # every second line (Bernoulli: a second pattern) shifted
        geo = footprint(pn, lines)
        if lines == "lines":
            k = pn // 64
            sh = torch.zeros_like(geo)
            for c0 in (25, 43):
                sh[:, c0 * k:(c0 + 4) * k] = 1
        else:
            from lithographysimulator_amd.synthetic import bernoulli_mask
            sh = bernoulli_mask(pn, seed=99)
        return L.alternatingPSM(geo, sh)
    gen = torch.Generator().manual_seed(1000 + pn)
    if kind == "random":                                       # a seeded complex map on the Bernoulli footprint
        v = torch.complex(torch.randn(pn, pn, generator=gen), torch.randn(pn, pn, generator=gen))
        return v * footprint(pn, "bern").to(torch.complex64)
    if kind == "imaginary":                                    # purely imaginary grey levels
        return torch.complex(torch.zeros(pn, pn), torch.rand(pn, pn, generator=gen) * footprint(pn, "bern").float())
    raise KeyError(kind)


# ---- 1: bit identity with the binary path --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lines", "bern"])
@pytest.mark.parametrize("pn,ps,wl", SIZES_IDENTITY)
def test_zero_one_transmission_is_the_binary_path_bit_for_bit(L, dev, pn, ps, wl, kind):
    """Zeros contribute exactly nothing to every butterfly, and the scale kernel's real part runs the int16 kernel's
    arithmetic: the claim holds in exact arithmetic, not to a tolerance."""
    g = footprint(pn, kind)
    binary = L.Mask(g, ps, dev)
    cplx = L.Mask(pixelSize=ps, device=dev, transmission=g.to(torch.complex64))
    assert binary.calculateEpsilonN(binary.deltaK, ps, wl) == cplx.calculateEpsilonN(cplx.deltaK, ps, wl)
    a, b = binary.fraunhofer(wl, True), cplx.fraunhofer(wl, True)
    assert b.dtype == torch.complex64 and tuple(b.shape) == (pn, pn)
    assert torch.equal(a, b), f"max |diff| {float((a - b).abs().max()):.3e} of {float(a.abs().max()):.3e}"


# ---- 2: spectrum against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["attenuated", "alternating", "random", "imaginary"])
@pytest.mark.parametrize("pn,ps,wl", SIZES_ORACLE)
def test_complex_spectrum_vs_oracle(L, dev, pn, ps, wl, kind):
    """2e-6 relative to the largest order: the bound this kernel family meets for binary masks (test_gpu_optics.py)."""
    t = transmission(L, pn, kind)
    got = L.Mask(pixelSize=ps, device=dev, transmission=t).fraunhofer(wl, True).cpu()
    ref = oracle_spectrum(t, ps, wl)
    e = rel_max(got, ref)
    print(f"{kind} {pn}^2 ps {ps} wl {wl}: rel-to-max {e:.2e}")
    assert e < 2e-6


def test_real_grey_transmission_and_nan_propagation(L, dev):
    """A real floating tensor is a grey mask (imaginary part zero); values are not inspected: a NaN propagates."""
    gen = torch.Generator().manual_seed(7)
    grey = torch.rand(64, 64, generator=gen, dtype=torch.float64)
    got = L.Mask(pixelSize=PS, device=dev, transmission=grey).fraunhofer(WL, True).cpu()
    assert rel_max(got, oracle_spectrum(grey.to(torch.complex64), PS, WL)) < 2e-6
    bad = grey.to(torch.complex64)
    bad[10, 20] = float("nan")
    spec = L.Mask(pixelSize=PS, device=dev, transmission=bad).fraunhofer(WL, True)
    assert bool(torch.isnan(spec.abs()).any())


# ---- 3: end to end against the oracle ------------------------------------------------------------------------------------
def test_attenuated_mask_image_vs_oracle_64(L, dev):
    from oracle import abbe_oracle as O
    from lithographysimulator_amd.synthetic import lines_mask
    pn = 64
    t = L.attenuatedPSM(lines_mask(pn))
    mask = L.Mask(pixelSize=PS, device=dev, transmission=t)
    mft = mask.fraunhofer(WL, True)
    bm = L.LightSource(0.4, 0.8, pn, NA, device=dev).generateQuasar(4, -math.pi / 8)
    pf = L.Pupil(pn, WL, NA, f16(DEMO_AB), dev).generatePupilFunction()
    img = L.abbeImage(mask, mft, pf, bm, PS, mask.deltaK, WL, True, dev).cpu()
    ref = O.abbe_image(oracle_spectrum(t, PS, WL), O.pupil_function(f16(DEMO_AB), pn, NA, WL),
                       O.source_quasar(0.4, 0.8, pn, 4, -math.pi / 8), PS, 4 / pn, WL)
    e_max, e_l2 = rel_max(img, ref), rel_l2(img, ref)
    print(f"attenuated 64^2 image: rel-to-max {e_max:.2e}, rel-L2 {e_l2:.2e}")
    assert img.shape == ref.shape and e_max < TOL_IMAGE_MAX and e_l2 < TOL_IMAGE_L2


@pytest.fixture(scope="module")
def case256(L, dev):
    """Attenuated mask at 256^2, 64 points of the annular source: the operands and the oracle's raw intensity, once."""
    from oracle import abbe_oracle as O
    from lithographysimulator_amd.synthetic import lines_mask
    pn = 256
    t = L.attenuatedPSM(lines_mask(pn))
    mask = L.Mask(pixelSize=PS, device=dev, transmission=t)
    eps, N = mask.calculateEpsilonN(mask.deltaK, PS, WL)
    bm = subsample_bitmap(O.source_annular(0.4, 0.8, pn), 64)
    shifts = O.source_shifts(bm, pn)
    ref = O.abbe_raw(oracle_spectrum(t, PS, WL), O.pupil_function(f16(DEMO_AB), pn, NA, WL), shifts, N)
    pf = L.Pupil(pn, WL, NA, f16(DEMO_AB), dev).generatePupilFunction()
    return mask, pf, shifts.to(dev), N, ref


@pytest.mark.parametrize("coarse", [0, 2])
def test_attenuated_mask_intensity_vs_oracle_256(L, dev, case256, coarse):
    """The direct path and the coarse-grid path (with its Nyquist-line correction) with a non-Hermitian M from a real use."""
    from lithographysimulator_amd import _native as nat
    mask, pf, shifts, N, ref = case256
    raw = L.abbeIntensity(mask.fraunhofer(WL, True), pf, shifts, N, options={"coarse": coarse}).cpu()
    assert nat.last_plan()["coarse_grid"] == (1 if coarse else 0), nat.last_plan()
    e_max, e_l2 = rel_max(raw, ref), rel_l2(raw, ref)
    print(f"attenuated 256^2 raw intensity, coarse={coarse}: rel-to-max {e_max:.2e}, rel-L2 {e_l2:.2e}")
    assert e_max < TOL_IMAGE_MAX and e_l2 < TOL_IMAGE_L2


# ---- 4: physics ----------------------------------------------------------------------------------------------------------
def _grating(pn=64):
    """Full-height vertical lines 3 px wide on a 6 px pitch; the shifter covers every second line."""
    cols = torch.arange(pn)
    clear = cols % 6 < 3
    geo = clear[None, :].expand(pn, pn).to(torch.int16).contiguous()
    sh = (clear & ((cols // 6) % 2 == 1))[None, :].expand(pn, pn).to(torch.int16).contiguous()
    return geo, sh


@pytest.mark.parametrize("kind", ["binary", "alternating"])
def test_alternating_mask_resolves_what_the_binary_mask_cannot(L, dev, kind):
    """150 nm pitch at 193 nm, NA 0.7, sigma <= 0.3: the binary mask's first orders lie outside the pupil (oracle
    contrast 0.042), the alternating mask's orders lie at half that frequency (oracle contrast 0.997)."""
    pn = 64
    geo, sh = _grating(pn)
    mask = L.Mask(geo, PS, dev) if kind == "binary" else L.Mask(pixelSize=PS, device=dev, transmission=L.alternatingPSM(geo, sh))
    bm = L.LightSource(0.0, 0.3, pn, NA, device=dev).generateAnnular()
    assert int(bm.sum()) == 69
    pf = L.Pupil(pn, WL, NA, None, dev).generatePupilFunction()
    img = L.abbeImage(mask, mask.fraunhofer(WL, True), pf, bm, PS, mask.deltaK, WL, True, dev).cpu()
    n = img.shape[0]
    row = img[n // 2, n // 2 - 12:n // 2 + 12]
    contrast = float((row.max() - row.min()) / (row.max() + row.min()))
    print(f"{kind}: contrast {contrast:.4f}")
    if kind == "binary":
        assert contrast < 0.1
    else:
        assert contrast > 0.9


# ---- 5: GDSII ------------------------------------------------------------------------------------------------------------
def _two_layer_library():
    from lithographysimulator_amd import layout as LY

    def rect(x0, y0, x1, y1):
        return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1], [x0, y0]])
    lib = LY.GdsLibrary("PSM", 1e-3, 1e-9)
    top = LY.GdsStructure("TOP")
    for i in range(4):                                          # clear apertures: 100 nm lines on a 200 nm pitch
        top.elements.append(LY.GdsElement("boundary", layer=1, datatype=0, xy=rect(300 + 200 * i, 200, 400 + 200 * i, 1400)))
    for i in (1, 3):                                            # shifters: wider than every second aperture, and shorter
        top.elements.append(LY.GdsElement("boundary", layer=2, datatype=0, xy=rect(270 + 200 * i, 400, 430 + 200 * i, 1200)))
    top.elements.append(LY.GdsElement("boundary", layer=3, datatype=0, xy=rect(0, 0, 1600, 100)))     # not listed: ignored
    lib.structures["TOP"] = top
    return lib


def test_gdsii_layers_compose_into_a_transmission(L, dev):
    from lithographysimulator_amd import layout as LY
    pn, ps = 64, 25
    lib = LY.readGDSII(LY.writeGDSII(_two_layer_library()))
    bg = complex(-0.245, 0)
    mask = L.maskFromGDSII(lib, pn, ps, top="TOP", origin=(0.0, 0.0), device=dev,
                           transmissions={(1, 0): 1, (2, 0): -1}, background=bg)
    r1 = L.rasterizeLayout(L.flattenLayout(lib, "TOP", [(1, 0)]), pn, ps, (0.0, 0.0), dev)
    r2 = L.rasterizeLayout(L.flattenLayout(lib, "TOP", [(2, 0)]), pn, ps, (0.0, 0.0), dev)
    assert int(r1.sum()) > 0 and int(r2.sum()) > 0 and int((r1 * r2).sum()) > 0 and int((r1 * (1 - r2)).sum()) > 0
    want = torch.full((pn, pn), bg, dtype=torch.complex64, device=dev)
    want[r1 != 0] = 1
    want[r2 != 0] = -1                                          # the later layer wins where both cover a pixel
    assert mask.transmission.dtype == torch.complex64 and torch.equal(mask.transmission, want)
    assert mask.pixelSize == ps and mask.pixelNumber == pn and mask.device == r1.device
    # the mapping's order decides: apertures listed last override the shifters
    swapped = L.maskFromGDSII(lib, pn, ps, top="TOP", origin=(0.0, 0.0), device=dev,
                              transmissions={(2, 0): -1, (1, 0): 1}, background=bg)
    want2 = torch.full((pn, pn), bg, dtype=torch.complex64, device=dev)
    want2[r2 != 0] = -1
    want2[r1 != 0] = 1
    assert torch.equal(swapped.transmission, want2) and not torch.equal(want, want2)
    # origin=None: one window, centred on the listed layers together
    auto = L.maskFromGDSII(lib, pn, ps, top="TOP", device=dev, transmissions={(1, 0): 1, (2, 0): -1}, background=bg)
    both = L.flattenLayout(lib, "TOP", [(1, 0), (2, 0)])
    lo, hi = np.min([q.min(axis=0) for q in both], axis=0), np.max([q.max(axis=0) for q in both], axis=0)
    org = (float((lo[0] + hi[0]) / 2) - pn * ps / 2.0, float((lo[1] + hi[1]) / 2) - pn * ps / 2.0)
    a1 = L.rasterizeLayout(L.flattenLayout(lib, "TOP", [(1, 0)]), pn, ps, org, dev)
    a2 = L.rasterizeLayout(L.flattenLayout(lib, "TOP", [(2, 0)]), pn, ps, org, dev)
    want3 = torch.full((pn, pn), bg, dtype=torch.complex64, device=dev)
    want3[a1 != 0] = 1
    want3[a2 != 0] = -1
    assert torch.equal(auto.transmission, want3)
    # transmissions=None: what it returns today -- a binary Mask of the chosen layers
    plain = L.maskFromGDSII(lib, pn, ps, top="TOP", layers=[(1, 0)], origin=(0.0, 0.0), device=dev)
    assert plain.transmission is None and plain.geometry.dtype == torch.int16 and torch.equal(plain.geometry, r1)
    # and the composed mask images: its spectrum is the oracle's
    assert rel_max(mask.fraunhofer(WL, True).cpu(), oracle_spectrum(want, ps, WL)) < 2e-6


# ---- 6: graph capture ----------------------------------------------------------------------------------------------------
def test_complex_spectrum_is_capturable_in_a_hip_graph(L, dev):
    """The call is asynchronous, allocates nothing and never waits on the host: one capture, one replay."""
    from lithographysimulator_amd.synthetic import lines_mask
    mask = L.Mask(pixelSize=PS, device=dev, transmission=L.attenuatedPSM(lines_mask(64)))
    eager = mask.fraunhofer(WL, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mask.fraunhofer(WL, True)                               # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mask.fraunhofer(WL, True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
