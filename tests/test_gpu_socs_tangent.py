"""Forward-mode Hopkins imaging on the GPU: litho_socs_jvp (csrc/socs_grad.hip), litho_measure_epe_jvp / litho_measure_cd_jvp
(csrc/metrology.hip) and lithographysimulator_amd/sensitivity.py against the float64 definitions of tests/socs_tangent_oracle.py,
against the engine itself and against hopkinsGradient; then the whole chain (maskErrorFactor, epeJacobian) against central
differences of the EXISTING device chain, and correctLayout(step="meef") against the damped loop.

Bounds.  The image tangent: helpers.TOL_IMAGE_MAX / TOL_IMAGE_L2 relative to the oracle's max|dI| and ||dI|| -- the formula has the
fields' own rounding, and its complex64 floor is under a quarter of them (test_socs_tangent_cpu.py measures it on these cases).
The size regimes are those of test_gpu_socs_grad.py: m = N / pn = 1, 1 < m <= pn, m > pn; several lines per workgroup and one.
Every test prints what it observed (-s)."""
import ctypes

import numpy as np
import pytest
import torch

import epe_oracle as EO
import opc_case as C
import resist_oracle as RO
import socs_grad_oracle as GO
import socs_tangent_oracle as TO
from helpers import TOL_IMAGE_L2, TOL_IMAGE_MAX
from oracle import abbe_oracle as O

pytestmark = pytest.mark.gpu

SIZES = GO.GRAD_SIZES + GO.EXTRA_SIZES


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat
    assert nat.lib().litho_target_arch() == b"gfx950"
    return L


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    return _native


def _check(tag, got, want):
    got, want = got.cpu().double(), want.double()
    e_max = float((got - want).abs().max() / want.abs().max())
    e_l2 = float(torch.linalg.norm(got - want) / torch.linalg.norm(want))
    print(f"{tag}: max {e_max:.2e} (bound {TOL_IMAGE_MAX:.0e}), l2 {e_l2:.2e} (bound {TOL_IMAGE_L2:.0e})")
    assert e_max < TOL_IMAGE_MAX and e_l2 < TOL_IMAGE_L2, (tag, e_max, e_l2)


# ---- 1, 2: against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,N", SIZES)
def test_tangent_against_the_oracle(L, dev, pn, N):
    """K = 5, one plane and two, three complex directions; the last direction is M itself and its tangent is 2 I."""
    for planes in (1, 2):
        k, M, _ = GO.sized_case(pn, N, 5, planes)
        dM = TO.directions(M, 3, 100 + pn + N)
        socs = GO.socs_around(k, dev)
        got = L.hopkinsTangent(M.to(dev), socs, N, dM.to(dev))
        want = TO.tangent(k, M, dM, N)
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
        for p in range(3):
            _check(f"tangent pn {pn} N {N} planes {planes} direction {p}", got[p], want[p])
        _check("  direction M against 2 I of the engine", got[2], 2.0 * L.hopkinsIntensity(M.to(dev), socs, N).cpu())


@pytest.mark.parametrize("pn,N", [(1024, 1024), (2048, 4096)])
def test_tangent_with_one_line_per_workgroup(L, dev, pn, N):
    """K = 2, P = 2: the truth on the 40 x 40 sub-grid of test_fields_with_one_line_per_workgroup."""
    k, M, _ = GO.sized_case(pn, N, 2, 1)
    dM = TO.directions(M, 2, pn)
    got = L.hopkinsTangent(M.to(dev), GO.socs_around(k, dev), N, dM.to(dev)).cpu()
    c = pn // 2
    idx = torch.tensor(sorted(set([0, 1, 2, c - 2, c - 1, c, c + 1, pn - 2, pn - 1] + list(range(5, pn, pn // 31)))))[:40]
    F = O.centred_dft_matrix(pn, N)[idx]
    E = F @ (k.to(TO.C128) * M.to(TO.C128)) @ F.T
    for p in range(2):
        dE = F @ (k.to(TO.C128) * dM[p].to(TO.C128)) @ F.T
        want = 2.0 * (E.real * dE.real + E.imag * dE.imag).sum(dim=0)
        _check(f"tangent pn {pn} N {N} direction {p} on {len(idx)} x {len(idx)} outputs", got[p][idx][:, idx], want)


# ---- 3, 4: against the engine and against the gradient ---------------------------------------------------------------------------
def test_tangent_against_differences_of_the_engine(L, dev):
    """(hopkinsIntensity(M + dM) - hopkinsIntensity(M - dM)) / 2 is the tangent exactly (the image is quadratic); both sides come
    from K fp32 fields, so the bound is the image's -- relative to the images the difference is formed from, which is where its
    rounding comes from."""
    pn, N = 64, 128
    for planes in (1, 2):
        k, M, _ = GO.sized_case(pn, N, 5, planes)
        dM = TO.directions(M, 2, 7)[:1]
        socs, Md, dMd = GO.socs_around(k, dev), M.to(dev), dM.to(dev)
        up = L.hopkinsIntensity(Md + dMd[0], socs, N).double()
        fd = (up - L.hopkinsIntensity(Md - dMd[0], socs, N).double()) / 2
        got = L.hopkinsTangent(Md, socs, N, dMd)[0]
        scale = up.cpu()
        e_max = float((got.cpu().double() - fd.cpu()).abs().max() / scale.abs().max())
        e_l2 = float(torch.linalg.norm(got.cpu().double() - fd.cpu()) / torch.linalg.norm(scale))
        print(f"planes {planes}: tangent vs engine difference, relative to the image: max {e_max:.2e}, l2 {e_l2:.2e}")
        assert e_max < TOL_IMAGE_MAX and e_l2 < TOL_IMAGE_L2


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("pn,N", [(32, 64), (128, 256)])
def test_dot_product_with_the_gradient(L, dev, pn, N, planes):
    k, M, G = GO.sized_case(pn, N, 5, planes)
    dM = TO.directions(M, 2, 3)
    socs, Md = GO.socs_around(k, dev), M.to(dev)
    J = L.hopkinsTangent(Md, socs, N, dM.to(dev)).cpu().double()
    g = L.hopkinsGradient(Md, socs, N, G.to(dev)).cpu()
    for p in range(2):
        lhs, rhs = float((G.double() * J[p]).sum()), GO.inner(g, dM[p])
        bound = GO.TOL_ADJOINT * float(torch.linalg.norm(J[p]) * torch.linalg.norm(G.double()))
        print(f"pn {pn} planes {planes} direction {p}: <G, J dM> {lhs:.8e}, Re <g, dM> {rhs:.8e}, difference {lhs - rhs:.2e} (bound {bound:.2e})")
        assert abs(lhs - rhs) <= bound


# ---- 5: bits -----------------------------------------------------------------------------------------------------------------------
def test_a_directions_bits_do_not_depend_on_its_neighbours(L, dev):
    pn, N = 64, 128
    for planes in (1, 2):
        k, M, _ = GO.sized_case(pn, N, 5, planes)
        socs, Md = GO.socs_around(k, dev), M.to(dev)
        dM = TO.directions(M, 17, 21).to(dev)
        alone = L.hopkinsTangent(Md, socs, N, dM[16])                              # a single [pn,pn] counts as P = 1
        among = L.hopkinsTangent(Md, socs, N, torch.cat([dM[:5], dM[16:], dM[5:15]]))      # 16 directions, this one the sixth
        chunked = L.hopkinsTangent(Md, socs, N, dM)                                # the 17th: the wrapper's second chunk
        assert tuple(alone.shape[:1]) == (1,) and tuple(chunked.shape[:1]) == (17,)
        assert torch.equal(alone[0], among[5]) and torch.equal(alone[0], chunked[16])
        assert torch.equal(chunked[:16], L.hopkinsTangent(Md, socs, N, dM[:16]))
        assert torch.equal(chunked, L.hopkinsTangent(Md, socs, N, dM))             # two calls


def test_chunks_and_out(L, dev):
    pn, N = 64, 128
    for planes in (1, 2):
        k, M, _ = GO.sized_case(pn, N, 5, planes)
        socs, Md = GO.socs_around(k, dev), M.to(dev)
        dM = TO.directions(M, 3, 22).to(dev)
        want = TO.tangent(k, M, dM.cpu(), N)
        default = L.hopkinsTangent(Md, socs, N, dM)
        by_two = L.hopkinsTangent(Md, socs, N, dM, kernelChunk=2)
        assert torch.equal(L.hopkinsTangent(Md, socs, N, dM, kernelChunk=5), default)
        _check(f"planes {planes} kernelChunk 2", by_two, want)
        k4 = k if planes == 2 else k[None]
        built = None
        for c0 in (0, 2, 4):
            part = GO.socs_around(k4[:, c0:c0 + 2] if planes == 2 else k4[0, c0:c0 + 2], dev)
            built = L.hopkinsTangent(Md, part, N, dM, out=built)
        assert torch.equal(by_two, built)
        start = torch.randn(tuple(default.shape), generator=torch.Generator().manual_seed(4)).to(dev)
        acc = start.clone()
        assert L.hopkinsTangent(Md, socs, N, dM, out=acc) is acc
        _check(f"planes {planes} accumulated into out", acc - start, want)
    with pytest.raises(ValueError):
        L.hopkinsTangent(Md, socs, N, dM, kernelChunk=0)
    for bad in (dM.real, dM[:, :-1], dM.cpu(), dM[None]):
        with pytest.raises(ValueError):
            L.hopkinsTangent(Md, socs, N, bad)


# ---- 6: the metrology tangents -----------------------------------------------------------------------------------------------------
MIN_SLOPE = 1.0 / 32     # of the threshold, per interval


def _device_opc_image(L, dev, golden):
    """(image fp32 [128,128] on the device, threshold, socs): tests/opc_case.py through 32 SOCS kernels."""
    pupil = L.Pupil(C.PN, C.WAVELENGTH, C.NA, None, device=dev).generatePupilFunction()
    source = L.LightSource(C.SIGMA_IN, C.SIGMA_OUT, C.PN, C.NA, device=dev).generateAnnular()
    socs = L.socsKernels(pupil, source, kernels=32)
    eps, N = O.calculate_epsilon_n(4 / C.PN, C.PIXEL, C.WAVELENGTH)
    raster = L.rasterizeLayout(C.layout(), C.PN, C.PIXEL, C.ORIGIN, dev, antialias=16)
    mft = L.Mask(pixelSize=C.PIXEL, device=dev, transmission=raster).fraunhofer(C.WAVELENGTH, True)
    return L.postProcess(L.hopkinsIntensity(mft, socs, N), eps), float(golden("g19_opc_loop.npz")["threshold"]), socs


@pytest.fixture(scope="module")
def opc(L, dev, golden):
    return _device_opc_image(L, dev, golden)


def _metrology_cases(opc):
    """(name, image [2,n,n] fp32 numpy, threshold, pixel): the smooth synthetic pair and the device's opc_case image with a dimmer,
    shifted second plane."""
    smooth = TO.smooth_pair(64, 9, planes=2)[0]
    image, threshold, _ = opc
    img = image.cpu().numpy()
    return [("smooth 64", smooth, 0.5, 25.0), ("opc 128", np.stack([img, 0.85 * np.roll(img, 3, axis=1)]).astype(np.float32), threshold, C.PIXEL)]


@pytest.mark.parametrize("exposed", [True, False])
@pytest.mark.parametrize("P", [1, 16])
def test_epe_tangent_against_the_oracle(L, dev, opc, P, exposed):
    """Bound 1e-4 max|d epe|.  d epe = ps h (-du_k w - (T - u_k)(du_{k+1} - du_k)) / w^2 with w = u_{k+1} - u_k formed in fp32 from
    two bilinear samples, each good to about 3 eps32 |u|: w carries 6 eps32 |u| and enters (to first order) squared, the numerator
    carries as much again, so |error| <= about 24 eps32 (|u| / |w|) |d epe|.  With |u| about T at a crossing and the sites of this
    test chosen FROM THE ORACLE to have |w| >= T / 32, that is 24 * 32 * 6e-8 = 4.6e-5 of |d epe|, under the bound of 1e-4 of the
    largest.  The sites the oracle finds no crossing for are kept: the NaN patterns must be identical."""
    gains = [0.8, 1.0, 1.25]
    for name, image, T, ps in _metrology_cases(opc):
        n = image.shape[-1]
        rng = np.random.default_rng(n + P)
        ang = rng.uniform(0, 2 * np.pi, 600)
        sites = np.stack([rng.uniform(2, n - 3, 600), rng.uniform(2, n - 3, 600), np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
        sites[0] = (np.nan, 5.0, 1.0, 0.0)                                         # a NaN site
        sites[1] = (1.0, 1.0, -1.0, -1.0)                                          # leaves the grid after two samples
        table, _ = EO.measure_epe(image, sites, gains, T, exposed, 6.0, ps)
        slope = table[..., 1] * (0.5 * ps) * T                                     # |u_{k+1} - u_k|
        ok = (np.isnan(slope) | (slope >= MIN_SLOPE * T)).all(axis=(0, 1))
        sites = sites[ok]
        dimage = (TO.smooth_pair(n, 10 + P, planes=2, P=P)[1] * (20 * float(np.abs(image).max()))).astype(np.float32)
        want, table = TO.epe_tangent(image, dimage, sites, gains, T, exposed, 6.0, ps)
        found = ~np.isnan(table[..., 0])
        assert (~found).any() and (table[..., 2][found] < 0).any() and found.sum() > 300 and np.isnan(table[:, :, 0]).all()
        img, dimg, st = torch.from_numpy(image).to(dev), torch.from_numpy(dimage).to(dev), torch.from_numpy(sites).to(dev)
        got = L.measureEPETangent(img, dimg, T, st, ps, doses=gains, exposed=exposed, searchRange=6.0).cpu().numpy().astype(np.float64)
        assert got.shape == want.shape == (P, 3, 2, len(sites))
        assert np.array_equal(np.isnan(got), np.isnan(want))
        e = float(np.nanmax(np.abs(got - want)) / np.nanmax(np.abs(want)))
        print(f"{name} P {P} exposed {exposed}: {len(sites)} sites, {int(found.sum())} crossings, max |d epe| {np.nanmax(np.abs(want)):.3g} nm, "
              f"error {e:.2e} of it (bound 1e-4)")
        assert e < 1e-4
        # and the primal kept its bits: the existing parity with the oracle, interval for interval
        prim = L.measureEPE(img, T, st, ps, doses=gains, exposed=exposed, searchRange=6.0).cpu().numpy()
        assert np.array_equal(np.isnan(prim[..., 0]), ~found) and np.array_equal(prim[..., 2][found], table[..., 2][found].astype(np.float32))
        one = L.measureEPETangent(img[0], dimg[:, 0], T, st, ps, doses=gains, exposed=exposed, searchRange=6.0)
        assert torch.equal(torch.nan_to_num(one[:, :, 0]), torch.nan_to_num(torch.from_numpy(got.astype(np.float32))[:, :, 0].to(dev)))


@pytest.mark.parametrize("exposed", [True, False])
@pytest.mark.parametrize("P", [1, 16])
def test_cd_tangent_against_the_oracle(L, dev, opc, P, exposed):
    """The same bound by the same derivation, per crossing; dcd is the difference of two such terms times the pixel.  Gauges whose
    crossings the oracle finds flatter than T / 32 per pixel are not among the chosen ones; border gauges, gauges on the other
    tone and gauges outside the grid are."""
    gains = [0.8, 1.0, 1.25]
    border_runs = 0
    for name, image, T, ps in _metrology_cases(opc):
        n = image.shape[-1]
        rng = np.random.default_rng(2 * n + P)
        gauges = [(int(r), int(c), int(a)) for r, c, a in zip(rng.integers(0, n, 400), rng.integers(0, n, 400), rng.integers(0, 2, 400))]
        table, runs, _ = RO.measure_cd(image, gauges, gains, T, exposed, ps)
        slopes = np.stack([table[..., 3], table[..., 4]]) * (T * ps)
        ok = (np.isnan(slopes) | (slopes >= MIN_SLOPE * T)).all(axis=(0, 1, 2))
        # and gauges on the first and last samples of a few lines: where those are inside, the run ends at the border
        gauges = [g for g, keep in zip(gauges, ok) if keep] + [(n + 5, 3, 0), (3, 3, 2)]
        gauges += [(r, 0, 0) for r in range(0, n, n // 8)] + [(n - 1, c, 1) for c in range(0, n, n // 8)]
        table, _, _ = RO.measure_cd(image, gauges, gains, T, exposed, ps)
        slopes = np.stack([table[..., 3], table[..., 4]]) * (T * ps)
        gauges = [g for g, keep in zip(gauges, (np.isnan(slopes) | (slopes >= MIN_SLOPE * T)).all(axis=(0, 1, 2))) if keep]
        dimage = (TO.smooth_pair(n, 30 + P, planes=2, P=P)[1] * (20 * float(np.abs(image).max()))).astype(np.float32)
        want, table = TO.cd_tangent(image, dimage, gauges, gains, T, exposed, ps)
        _, runs, _ = RO.measure_cd(image, gauges, gains, T, exposed, ps)
        inside = runs[..., 0] >= 0
        assert inside.any() and (~inside).any()
        border_runs += int(((runs[..., 0] == 0) | (runs[..., 1] == n - 1))[inside].sum())
        img, dimg = torch.from_numpy(image).to(dev), torch.from_numpy(dimage).to(dev)
        got = L.measureCDTangent(img, dimg, gauges, T, ps, doses=gains, exposed=exposed).cpu().numpy().astype(np.float64)
        assert got.shape == want.shape == (P, 3, 2, len(gauges), 3)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        e = [float(np.nanmax(np.abs(got[..., j] - want[..., j])) / np.nanmax(np.abs(want[..., j]))) for j in range(3)]
        print(f"{name} P {P} exposed {exposed}: {len(gauges)} gauges, {int(inside.sum())} inside; errors (dcd, dx_lo, dx_hi) "
              f"{e[0]:.2e} {e[1]:.2e} {e[2]:.2e} of the largest (bound 1e-4)")
        assert max(e) < 1e-4
        prim = L.measureCD(img, T, gauges, ps, doses=gains, exposed=exposed).cpu().numpy()
        assert np.array_equal(np.isnan(prim), np.isnan(table))
        assert float(np.nanmax(np.abs(prim[..., 0] - table[..., 0]))) <= 1e-3 * ps
    assert border_runs > 0


# ---- 7: the whole chain ------------------------------------------------------------------------------------------------------------
# The window of the whole-chain test: every edge of the lattice layout lies 5 (x) or 3 (y) lattice steps inside a pixel, so a move
# of up to 2 steps either way stays inside that pixel and the raster is affine in the bias PIXEL BY PIXEL.  With edges ON pixel
# borders (origin (0, 0)) the coverage of a pixel has a kink at zero bias -- an outward move fills the pixel outside, an inward one
# empties the pixel inside -- and the image gets an h |h| term that a central difference does not cancel (measured: 1 % of the
# MEEF per 1.56 nm); the tangent there is the symmetric derivative.
LATTICE_ORIGIN = (-5 * C.PIXEL / 16, -3 * C.PIXEL / 16)


def _device_chain(L, dev, socs, polys, sites, bias, threshold, gauges, fields=False):
    """The EXISTING chain: biasLayout -> rasterizeLayout(16) -> spectrum -> hopkinsIntensity (`fields`: hopkinsFields, squared and
    summed in float64) -> postProcess -> measureEPE and measureCD, as float64 numpy: (epe_nm [S], cd_nm [G], the EPE's interval t_k [S], the CD's run (first, last inside sample) [G,2])."""
    eps, N = O.calculate_epsilon_n(4 / C.PN, C.PIXEL, C.WAVELENGTH)
    raster = L.rasterizeLayout(L.biasLayout(polys, sites, bias), C.PN, C.PIXEL, LATTICE_ORIGIN, dev, antialias=16)
    mft = L.Mask(pixelSize=C.PIXEL, device=dev, transmission=raster).fraunhofer(C.WAVELENGTH, True)
    if fields:                                                  # the same image from the code the tangent runs on: sum_k |E_k|^2
        E = L.hopkinsFields(mft, socs, N)
        raw = (E.real.double() ** 2 + E.imag.double() ** 2).sum(dim=0).float()
    else:
        raw = L.hopkinsIntensity(mft, socs, N)
    image = L.postProcess(raw, eps)
    e = L.measureEPE(image, threshold, sites, C.PIXEL, searchRange=C.RANGE)[0, 0].double().cpu().numpy()
    c = L.measureCD(image, threshold, gauges, C.PIXEL, exposed=True)[0, 0].double().cpu().numpy()
    run = np.nan_to_num(np.stack([np.ceil(c[:, 1]), np.floor(c[:, 2])], axis=1), nan=-1.0)
    return e[:, 0], c[:, 0], np.nan_to_num(e[:, 2], nan=-99.0), run


def test_meef_and_jacobian_against_differences_of_the_device_chain(L, dev, opc):
    """The lattice layout in a window that keeps its edges inside pixels (the raster is affine in the bias, pixel by pixel, for the
    steps used), K = 32.  |tan - FD(d/2)| <= |FD(d) - FD(d/2)| + r at d = pixel / 8: the truncation term is c d^2, so the
    derivative sits three times inside; r = 2 rho / d is the fp32 noise of the difference, rho the largest change of an EPE (a
    CD) between the two chains' images of the SAME layout -- the engine's (hopkinsIntensity, what the differences run on) and
    the one of the line transforms the tangent runs on (sum_k |hopkinsFields|^2): measured here, from the primal alone.  As in the CPU test of the metrology tangents, the criterion is for the
    sites and gauges whose chosen interval (run) is the primal's at all four moved layouts: both formulas are piecewise, a
    crossing that passes a sample changes the piece, and a difference across two pieces is no estimate of either's derivative.
    An edge moves by up to MEEF d = 4 nm = 0.16 pixel here, so a good part of them do; their share is printed and bounded."""
    _, threshold, socs = opc
    polys = TO.lattice_layout()
    sites = L.layoutSites(polys, TO.LATTICE_SPACING, C.PIXEL, LATTICE_ORIGIN, C.PN, C.WAVELENGTH)
    S = len(sites)
    # across the dense lines, along one (its ends), across the isolated line (two cuts), the contact both ways, the L's arms (two cuts each)
    gauges = [(48, 19, 0), (48, 35, 0), (40, 51, 0), (48, 35, 1), (44, 85, 0), (30, 85, 0), (96, 32, 0), (96, 32, 1), (83, 90, 1),
              (83, 100, 1), (100, 78, 0), (108, 78, 0)]
    zero = np.zeros(S)
    e0, cd0, tk0, run0 = _device_chain(L, dev, socs, polys, sites, zero, threshold, gauges)
    e1, cd1, _, _ = _device_chain(L, dev, socs, polys, sites, zero, threshold, gauges, fields=True)
    rho_epe = float(np.nanmax(np.abs(e0 - e1)))
    rho_cd = float(np.nanmax(np.abs(cd0 - cd1)))
    d = C.PIXEL / 8
    print(f"{S} sites; repeatability between the two chains' images: EPE {rho_epe:.2e} nm, CD {rho_cd:.2e} nm")

    def fd(direction, step):
        """(dEPE/dh [S], dCD/dh [G], the sites whose interval is the primal's at both moves, the gauges whose run is)."""
        up, dn = (_device_chain(L, dev, socs, polys, sites, s * step * direction, threshold, gauges) for s in (1.0, -1.0))
        same_site = (up[2] == tk0) & (dn[2] == tk0)
        same_gauge = (up[3] == run0).all(axis=1) & (dn[3] == run0).all(axis=1)
        return (up[0] - dn[0]) / (2 * step), (up[1] - dn[1]) / (2 * step), same_site, same_gauge

    cd, meef = L.maskErrorFactor(polys, gauges, socs, C.PN, C.PIXEL, LATTICE_ORIGIN, C.WAVELENGTH, threshold)
    cd, meef = cd[0].double().cpu().numpy(), meef[0].double().cpu().numpy()
    assert np.array_equal(cd, cd0) and (cd > 0).all()
    (_, c1, _, g1), (_, c2, _, g2) = fd(np.ones(S), d), fd(np.ones(S), d / 2)
    keep = g1 & g2
    err, bound = np.abs(meef - c2 / 2), np.abs(c1 - c2) / 2 + 2 * rho_cd / d / 2
    print("gauge CD nm", np.round(cd, 2), "\nMEEF", np.round(meef, 3), "\nrun kept", keep, "\n|tan - FD(d/2)|", err, "\nbound", bound)
    assert keep.sum() >= len(gauges) // 2 and (err <= bound)[keep].all() and (meef > 0.5).all()

    columns = [0, S // 3, S - 5]
    dirs = np.zeros((3, S))
    dirs[np.arange(3), columns] = 1.0
    epe, J = L.epeJacobian(polys, sites, zero, socs, C.PN, C.PIXEL, LATTICE_ORIGIN, C.WAVELENGTH, threshold, searchRange=C.RANGE, directions=dirs)
    assert np.array_equal(np.nan_to_num(epe), np.nan_to_num(e0)) and J.shape == (S, 3)
    for j, col in enumerate(columns):
        (f1, _, s1, _), (f2, _, s2, _) = fd(dirs[j], d), fd(dirs[j], d / 2)
        keep = s1 & s2 & ~np.isnan(J[:, j])
        err, bound = np.abs(J[:, j] - f2)[keep], np.abs(f1 - f2)[keep] + 2 * rho_epe / d
        off = np.delete(J[:, j], col)
        print(f"column {col}: J[{col},{col}] = {J[col, j]:.4f}, largest |J| off the diagonal {np.nanmax(np.abs(off)):.4f}; {int(keep.sum())} of {S} "
              f"sites keep their interval; max |tan - FD(d/2)| {err.max():.2e}, its bound {bound[np.argmax(err)]:.2e}")
        assert keep.sum() >= 0.9 * S and (err <= bound).all() and abs(J[col, j]) > 0.3


# ---- 8: the loop -------------------------------------------------------------------------------------------------------------------
def test_meef_loop_against_the_damped_loop(L, dev, opc):
    _, threshold, socs = opc
    kw = dict(spacing=C.SPACING, iterations=4, maxBias=C.MAX_BIAS, antialias=C.ANTIALIAS, searchRange=C.RANGE, model="socs", socs=socs)
    pupil = L.Pupil(C.PN, C.WAVELENGTH, C.NA, None, device=dev).generatePupilFunction()
    source = L.LightSource(C.SIGMA_IN, C.SIGMA_OUT, C.PN, C.NA, device=dev).generateAnnular()
    args = (C.layout(), C.PN, C.PIXEL, C.ORIGIN, C.WAVELENGTH, pupil, source, threshold)
    damped = L.correctLayout(*args, gain=C.GAIN, **kw)
    same = L.correctLayout(*args, gain=C.GAIN, step="damped", **kw)
    meef = L.correctLayout(*args, step="meef", **kw)
    print("damped history (rms nm, max nm, lost):", [(round(a, 4), round(b, 4), c) for a, b, c in damped.history])
    print("meef   history (rms nm, max nm, lost):", [(round(a, 4), round(b, 4), c) for a, b, c in meef.history])
    assert same.history == damped.history and damped.jacobian is None
    assert meef.jacobian is not None and meef.jacobian.shape == (len(meef.sites), len(meef.sites))
    best = lambda r: r.history[r.best_iteration]                                   # noqa: E731
    assert best(meef)[2] <= best(damped)[2] and best(meef)[0] <= best(damped)[0]
    with pytest.raises(ValueError):
        L.correctLayout(*args, step="meef", **{**kw, "model": "abbe", "socs": None})


# ---- 9: arguments ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_come_back_as_codes_and_launch_nothing(nat, dev):
    lib = nat.lib()
    poison = lambda n: torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)       # noqa: E731
    pn, K, groups, P = 16, 2, 2, 2
    cells = pn * pn
    kern, m, dm = poison(groups * K * cells * 8), poison(cells * 8), poison(P * cells * 8)
    out = poison(P * groups * cells * 4)
    need = int(lib.litho_socs_jvp_work_bytes(groups, K, P, pn))
    assert need == 2 * groups * K * cells * 8 + groups * cells * 4
    work = poison(need)
    st = nat.stream_ptr(dev)
    p = nat.ptr

    def jvp(kernels=kern, mask=m, dmask=dm, P=P, groups=groups, K=K, pn=pn, N=32, dI=out, work=work, nbytes=need):
        return lib.litho_socs_jvp(p(kernels) if kernels is not None else None, p(mask) if mask is not None else None,
                                  p(dmask) if dmask is not None else None, P, groups, K, pn, N, p(dI) if dI is not None else None, 0,
                                  p(work) if work is not None else None, nbytes, st)
    for kw in (dict(pn=24), dict(pn=8), dict(N=48), dict(N=8192), dict(P=0), dict(P=17), dict(groups=0), dict(K=0), dict(kernels=None),
               dict(mask=None), dict(dmask=None), dict(dI=None), dict(work=None)):
        assert jvp(**kw) == nat.E_ARG, kw
    assert jvp(pn=32, N=16) == nat.E_NSMALL
    assert jvp(nbytes=need - 1) == nat.E_WORKSPACE
    for bad in ((0, K, P, pn), (groups, 0, P, pn), (groups, K, 0, pn), (groups, K, 17, pn), (groups, K, P, 24), (groups, K, P, 8192)):
        assert int(lib.litho_socs_jvp_work_bytes(*bad)) == 0, bad
    # metrology
    n, S, G = 16, 3, 2
    img, dimg = poison(n * n * 4), poison(P * n * n * 4)
    sites, gauges = poison(S * 16), poison(G * 12)
    eout, cout = poison(P * S * 4), poison(P * G * 12)
    one = (ctypes.c_float * 1)(1.0)
    nan = (ctypes.c_float * 1)(float("nan"))

    def epe(image=img, dimage=dimg, P=P, planes=1, n=n, sites=sites, S=S, gains=one, n_gains=1, rng=8.0, ps=25.0, o=eout):
        q = lambda t: p(t) if t is not None else None                              # noqa: E731
        return lib.litho_measure_epe_jvp(q(image), q(dimage), P, planes, n, q(sites), S, gains, n_gains, 0.5, 1, rng, ps, q(o), st)

    def cd(image=img, dimage=dimg, P=P, planes=1, n=n, gauges=gauges, G=G, gains=one, n_gains=1, T=0.5, ps=25.0, o=cout):
        q = lambda t: p(t) if t is not None else None                              # noqa: E731
        return lib.litho_measure_cd_jvp(q(image), q(dimage), P, planes, n, q(gauges), G, gains, n_gains, T, 1, ps, q(o), st)
    for kw in (dict(image=None), dict(dimage=None), dict(sites=None), dict(gains=None), dict(o=None), dict(P=0), dict(P=17), dict(planes=0),
               dict(planes=65536), dict(n=0), dict(S=0), dict(n_gains=0), dict(n_gains=65), dict(gains=nan), dict(rng=0.0), dict(rng=33.0),
               dict(ps=0.0), dict(ps=float("inf"))):
        assert epe(**kw) == nat.E_ARG, kw
    for kw in (dict(image=None), dict(dimage=None), dict(gauges=None), dict(gains=None), dict(o=None), dict(P=0), dict(P=17), dict(planes=0),
               dict(planes=65536), dict(n=0), dict(G=0), dict(n_gains=0), dict(n_gains=65), dict(gains=nan), dict(T=float("nan")),
               dict(ps=0.0), dict(ps=float("inf"))):
        assert cd(**kw) == nat.E_ARG, kw
    torch.cuda.synchronize(dev)
    for name, t in (("dI", out), ("work", work), ("epe out", eout), ("cd out", cout)):
        assert bool((t == 0xFF).all()), f"{name} was written by a refused call"
