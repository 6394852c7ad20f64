"""The resist film stack on the GPU: litho_film_pupils (csrc/film.hip), filmPupils and vectorSocsKernels(film=, depths=,
depthWeights=) (lithographysimulator_amd/film.py, vector.py) and the unchanged consumers of what they return.

Truth is tests/film_oracle.py in float64 (pinned to closed forms in test_film_cpu.py).  Bounds: the planes, per element,
|got - want| <= 2^-22 |want| + 1e-12 max |want| -- the first term is test_gpu_vector.py's (one fp32 rounding per component), the
second covers cells where the s- and p-terms cancel in double; it is four orders above 2^-52 and five below fp32's 2^-24, so it
cannot hide an fp32-level error.  The homogeneous stack against vectorPupils 2 . 2^-22 |want| (two independent roundings).
Images helpers.TOL_IMAGE_MAX / TOL_IMAGE_L2 at full rank, `captured` within 1e-5 of 1, traces 1e-6 relative, the closed-form
intensity ratios 1e-5.  Every test prints what it observed (-s).

Measured on an MI355X: planes 5.8e-8 ... 5.9e-8 worst relative error at pn 16, 30 and 64, for L = 1, 3 and 16 with the resist
first, middle and last (bound 2.4e-7 + 1e-12 max), the same with cells exactly on alpha^2 + beta^2 = 1 (exact zeros, everything
finite), on a pupil stack and at 17 depths, which equal 17 single-depth calls bit for bit, as does a second call; the
homogeneous stack 9.6e-8 ... 1.1e-7 from vectorPupils (bound 4.8e-7); full-rank images per (focus, depth) plane max
3.4e-7 ... 7.6e-7, l2 1.7e-7 ... 4.6e-7 against vectorAbbeIntensity (bounds 2e-5, 5e-6), that against the float64 truth 2.6e-7 max,
captured within 3.4e-7 of 1; the bulk image from one kernel set max 5.1e-7 ... 8.1e-7, its trace equal to the weighted sum to nine
digits; intensity ratios 3.1e-7 (standing wave) and 9.2e-8 (absorption) from the closed forms (bound 1e-5); film=None equal bit
for bit.  The whole file takes five seconds."""
import ctypes

import numpy as np
import pytest
import torch

import film_oracle as FO
import vector_oracle as VO
from helpers import DEMO_AB, NA, PS, TOL_IMAGE_L2, TOL_IMAGE_MAX, f16, rel_l2, rel_max
from oracle import abbe_oracle as O

pytestmark = pytest.mark.gpu
WL = FO.WL
WATER = (1.35, FO.WATER)


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
    e_max, e_l2 = rel_max(got.cpu(), want), rel_l2(got.cpu(), want)
    print(f"{tag}: max {e_max:.2e} (bound {TOL_IMAGE_MAX:.0e}), l2 {e_l2:.2e} (bound {TOL_IMAGE_L2:.0e})")
    assert e_max < TOL_IMAGE_MAX and e_l2 < TOL_IMAGE_L2, (tag, e_max, e_l2)


def _planes_check(tag, got, want, first=2.0 ** -22, second=1e-12):
    """Returns the worst relative error over the non-zero elements."""
    got, want = got.cpu().numpy().astype(np.complex128), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all(), tag
    excess = np.abs(got - want) - first * np.abs(want) - second * np.abs(want).max()
    worst = float((np.abs(got - want)[want != 0] / np.abs(want)[want != 0]).max())
    assert (excess <= 0).all(), (tag, worst, float(excess.max()))
    assert not got[want == 0].any(), tag
    return worst


def _pupils(pn):
    g = torch.Generator().manual_seed(pn)
    return {"demo": O.pupil_function(f16(DEMO_AB), pn, NA, WL).to(torch.complex64),
            "random": torch.view_as_complex(torch.randn((pn, pn, 2), generator=g, dtype=torch.float32) + 0.1)}


def _stacks():
    """L = 1, 3 and 16 with the resist first, in the middle and last."""
    l3 = FO.STACKS["L3"][0]
    return [("L1", FO.STACKS["L1"])] + [(f"L3 resist {r}", (l3, FO.SILICON, r)) for r in (0, 1, 2)] + \
           [(f"L16 resist {r}", FO.stack16(r)) for r in (0, 8, 15)]


def _depths(layers, resist, D):
    d = layers[resist][2]
    return [0.37 * d] if D == 1 else [0.0, 0.37 * d, d]


# ---- 1. litho_film_pupils --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", [16, 30, 64])
def test_film_pupils_against_the_oracle(L, dev, pn):
    """One workgroup (16), an even size that is no multiple of the block or of anything else (30), 64; L = 1, 3, 16 with the
    resist first, middle and last; one depth without defocus (the NULL path) and three depths with a defocus list; demo
    aberrations and a random pupil that is non-zero everywhere; with and without gamma^(-1/2); dry and water.  Worst relative
    error seen on an MI355X: LABNOTES.md."""
    zs = (-100.0, 0.0, 100.0)
    worst = 0.0
    for tag, (layers, sub, res) in _stacks():
        stack = L.FilmStack(layers, sub, res)
        for name, P in _pupils(pn).items():
            p = P.numpy().astype(np.complex128)
            for na, n in VO.OPTICS:
                for rad in (False, True):
                    one = _depths(layers, res, 1)
                    got = L.filmPupils(P.to(dev), na, stack, one, WL, n, rad)
                    assert got.dtype == torch.complex64 and tuple(got.shape) == (1, 6, pn, pn)
                    e = _planes_check(f"pn {pn} {tag} {name} NA {na} rad {rad} D 1", got,
                                      FO.film_pupils(p, na, n, layers, sub, res, one, WL, rad))
                    three = _depths(layers, res, 3)
                    got = L.filmPupils(P.to(dev), na, stack, three, WL, n, rad, defocus=list(zs))
                    assert tuple(got.shape) == (3, 3, 6, pn, pn)
                    for i, z in enumerate(zs):
                        e = max(e, _planes_check(f"pn {pn} {tag} {name} NA {na} rad {rad} D 3 z {z:+.0f}", got[i],
                                                 FO.film_pupils(p, na, n, layers, sub, res, three, WL, rad, z)))
                    worst = max(worst, e)
        print(f"pn {pn} {tag}: worst relative error so far {worst:.2e} (bound {2.0 ** -22:.2e} + 1e-12 max)")
    if pn == 64:
        assert (~VO.cosines(pn, 0.7, 1.0)[3]).any()


def test_film_pupils_stack_second_call_and_many_depths(L, dev):
    """A pupil stack with one defocus value per plane; a second call gives the same bits; 17 depths take two launches per plane
    (16 depths travel with one launch) and equal the oracle and, depth by depth, the single-depth calls bit for bit."""
    pn = 30
    layers, sub, res = FO.STACKS["L3"]
    stack = L.FilmStack(layers, sub, res)
    pupils = _pupils(pn)
    two = torch.stack([pupils["demo"], pupils["random"]]).to(dev)
    depths = _depths(layers, res, 3)
    got = L.filmPupils(two, *WATER[:1], stack, depths, WL, WATER[1], True, defocus=[50.0, -30.0])
    assert tuple(got.shape) == (2, 3, 6, pn, pn)
    for i, (name, z) in enumerate((("demo", 50.0), ("random", -30.0))):
        e = _planes_check(f"stack plane {i}", got[i],
                          FO.film_pupils(pupils[name].numpy().astype(np.complex128), *WATER, layers, sub, res, depths, WL, True, z))
        print(f"pupil stack plane {i} ({name}, z {z:+.0f}): worst relative error {e:.2e}")
    again = L.filmPupils(two, WATER[0], stack, depths, WL, WATER[1], True, defocus=[50.0, -30.0])
    assert torch.equal(torch.view_as_real(again).view(torch.int32), torch.view_as_real(got).view(torch.int32))     # as bit patterns
    many = stack.depths(17)
    P = pupils["random"]
    got = L.filmPupils(P.to(dev), WATER[0], stack, many, WL, WATER[1])
    assert tuple(got.shape) == (17, 6, pn, pn)
    e = _planes_check("17 depths", got, FO.film_pupils(P.numpy().astype(np.complex128), *WATER, layers, sub, res, many, WL))
    single = torch.cat([L.filmPupils(P.to(dev), WATER[0], stack, z, WL, WATER[1]) for z in many])
    same = torch.equal(torch.view_as_real(single), torch.view_as_real(got))
    print(f"17 depths in two launches: worst relative error {e:.2e}, {'==' if same else '!='} 17 single-depth calls")
    assert same


@pytest.mark.parametrize("na,n,pn", [(0.72, 1.44, 64), (0.5, 1.0, 32)])
def test_film_pupils_on_the_evanescent_boundary(L, dev, na, n, pn):
    """The two exactly representable cases of test_gpu_vector.py: alpha^2 + beta^2 == 1.0 exactly at cells (pn/2, 0) and
    (0, pn/2).  Those are exact zeros in all six planes at every depth, and everything is finite."""
    a, b, gamma, inside = VO.cosines(pn, na, n)
    on = (a * a + b * b) == 1.0
    assert int(on.sum()) == 2 and not inside[on].any()
    P = _pupils(pn)["random"]
    assert bool((P != 0).all())
    layers, sub, res = FO.STACKS["L3"]
    stack, depths = L.FilmStack(layers, sub, res), _depths(layers, res, 3)
    for rad in (False, True):
        got = L.filmPupils(P.to(dev), na, stack, depths, WL, n, rad, defocus=[-100.0, 100.0])
        assert bool(torch.isfinite(torch.view_as_real(got)).all()) and not got.cpu()[:, :, :, torch.from_numpy(on)].any()
        for i, z in enumerate((-100.0, 100.0)):
            e = _planes_check(f"boundary NA {na} rad {rad} z {z:+.0f}", got[i],
                              FO.film_pupils(P.numpy().astype(np.complex128), na, n, layers, sub, res, depths, WL, rad, z))
            print(f"NA {na} n {n} pn {pn} radiometric {rad} z {z:+.0f}: worst relative error {e:.2e}, 2 boundary cells exact zeros")


@pytest.mark.parametrize("na,n", VO.OPTICS)
def test_homogeneous_stack_on_the_device_is_vector_pupils(L, dev, na, n):
    """Every index equal to the incident one: filmPupils at depth z equals vectorPupils(defocus = z from the top of the stack)
    times exp(-2 pi i n z / lambda), applied in complex128; two independent fp32 roundings, 2 . 2^-22 |want|."""
    pn = 64
    P = _pupils(pn)["random"].to(dev)
    stack = L.FilmStack([(n, 0.0, 50.0), (n, 0.0, 80.0), (n, 0.0, 20.0)], (n, 0.0), 1)
    depths = [0.0, 25.0, 80.0]
    for rad in (False, True):
        got = L.filmPupils(P, na, stack, depths, WL, n, rad)
        ref = L.vectorPupils(P, na, n, rad, defocus=[50.0 + z for z in depths], wavelength=WL)
        for i, z in enumerate(depths):
            want = ref[i].cpu().numpy().astype(np.complex128) * np.exp(-2j * np.pi * n * (50.0 + z) / WL)
            e = _planes_check(f"homogeneous NA {na} rad {rad} z {z}", got[i], want, first=2.0 * 2.0 ** -22, second=0.0)
            print(f"NA {na} n {n} radiometric {rad} z {50.0 + z:.0f}: worst relative difference {e:.2e} (bound {2.0 ** -21:.2e})")


def test_film_pupils_argument_errors(nat, dev):
    pn = 16
    P = torch.ones((pn, pn), dtype=torch.complex64, device=dev)
    out = torch.full((2, 6, pn, pn), 7.0, dtype=torch.complex64, device=dev)
    f, st = nat.lib().litho_film_pupils, nat.stream_ptr(dev)
    nan, inf = float("nan"), float("inf")

    def call(planes=1, size=pn, na=1.35, index=1.44, layers=((1.7, 0.02, 100.0), (1.8, 0.3, 40.0)), L_=None, sub=(0.88, 2.78),
             resist=0, depths=(10.0, 90.0), D=None, defocus=None, wl=WL, pupil=P, dst=out):
        flat = [v for layer in layers for v in layer]
        lay = (ctypes.c_double * max(1, len(flat)))(*flat)
        zd = (ctypes.c_double * max(1, len(depths)))(*depths)
        zf = (ctypes.c_double * len(defocus))(*defocus) if defocus is not None else None
        return f(nat.ptr(pupil) if pupil is not None else None, planes, size, na, index, 0, lay, len(layers) if L_ is None else L_,
                 sub[0], sub[1], resist, zd, len(depths) if D is None else D, zf, wl, nat.ptr(dst) if dst is not None else None, st)

    thick = ((1.7, 0.0, 10.0),) * 17
    bad = [dict(L_=0), dict(layers=thick), dict(resist=2), dict(resist=-1), dict(D=0), dict(planes=0), dict(planes=32768),
           dict(layers=((1.7, nan, 100.0),)), dict(layers=((inf, 0.0, 100.0),)), dict(layers=((1.7, 0.0, inf),)),
           dict(sub=(nan, 0.0)), dict(sub=(0.88, inf)), dict(depths=(nan,)), dict(defocus=(nan,)), dict(defocus=(inf,)),
           dict(wl=nan), dict(wl=0.0), dict(na=nan), dict(index=nan),
           dict(layers=((1.7, -0.01, 100.0),)), dict(sub=(0.88, -1.0)), dict(layers=((0.0, 0.0, 100.0),)), dict(sub=(0.0, 1.0)),
           dict(layers=((1.7, 0.0, 0.0),)), dict(layers=((1.7, 0.0, -5.0),)),
           dict(depths=(-0.1,)), dict(depths=(100.1,)), dict(resist=1, depths=(40.1,)),
           dict(na=1.44), dict(na=1.5), dict(size=15), dict(size=14), dict(pupil=None), dict(dst=None)]
    for kw in bad:
        assert call(**kw) == nat.E_ARG, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                             # a refused call writes nothing
    assert call() == 0 and call(resist=1, depths=(0.0, 40.0)) == 0                               # and the good ones run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.view_as_real(out)).all()) and not bool((out == 7.0).any())


# ---- 2. end to end ----------------------------------------------------------------------------------------------------------------
_e2e = {}


def _end_to_end(L, dev):
    """pn 32, N 64: demo pupil, five lit points of the annular 0.3-0.9 source (weight 1), the Bernoulli mask's spectrum, the L3
    stack at three depths, two focus planes."""
    if not _e2e:
        from lithographysimulator_amd.synthetic import bernoulli_mask
        import socs_oracle as SO
        pn = 32
        W = SO.strided_points(O.source_annular(0.3, 0.9, pn), 5).to(torch.float32)
        layers, sub, res = FO.STACKS["L3"]
        _e2e.update(pn=pn, N=64, W=W, S=int((W > 0).sum()), P=O.pupil_function(f16(DEMO_AB), pn, NA, WL).to(torch.complex64).to(dev),
                    M=O.mask_spectrum(bernoulli_mask(pn), PS, WL).to(torch.complex64).to(dev), stack=L.FilmStack(layers, sub, res),
                    depths=[10.0, 45.0, 100.0], zs=[-60.0, 40.0], shifts=L.sourceShifts((W > 0).to(dev), pn))
        _e2e["Q"] = L.filmPupils(_e2e["P"], WATER[0], _e2e["stack"], _e2e["depths"], WL, WATER[1], True, defocus=_e2e["zs"])
    return _e2e


@pytest.mark.parametrize("mode", ["x", "unpolarized"])
def test_end_to_end_per_depth_and_bulk(L, dev, mode):
    c = _end_to_end(L, dev)
    pn, N, S, D, F = c["pn"], c["N"], c["S"], 3, 2
    assert S <= 5 and tuple(c["Q"].shape) == (F, D, 6, pn, pn)
    abbe = L.vectorAbbeIntensity(c["M"], c["Q"].reshape(F * D, 6, pn, pn), c["shifts"], N, polarization=mode)
    assert tuple(abbe.shape) == (F * D, pn, pn)
    # the on-device truth itself against the float64 vector Abbe sum of the oracle's planes, at one (f, d)
    Q64 = FO.film_pupils(c["P"].cpu().numpy(), *WATER, *FO.STACKS["L3"], c["depths"], WL, True, c["zs"][1])
    _check(f"{mode}: vectorAbbeIntensity on the film planes vs float64 truth, plane (1, 2)", abbe[5],
           VO.abbe_truth(Q64[2], c["M"].cpu(), c["W"].numpy().astype(np.float64), mode, 1.0, N))
    rank = (3 if mode == "x" else 5) * S
    common = dict(polarization=mode, mediumIndex=WATER[1], radiometric=True, defocus=c["zs"], wavelength=WL, oversample=0,
                  film=c["stack"], depths=c["depths"])
    k = L.vectorSocsKernels(c["P"], c["W"].to(dev), WATER[0], kernels=rank, **common)
    assert k.stacked and k.planes == F * D and k.K == rank and tuple(k.kernels.shape) == (F * D, rank, pn, pn)
    got = L.hopkinsIntensity(c["M"], k, N)
    for f in range(F):
        for d in range(D):
            _check(f"{mode} plane f {f} d {d}: hopkins vs vectorAbbeIntensity", got[f * D + d], abbe[f * D + d].cpu().double())
    print(f"{mode}: K {rank}, captured {k.captured.tolist()}")
    assert float((k.captured - 1.0).abs().max()) < 1e-5
    # bulk: one kernel set per focus plane
    omega = [0.2, 0.5, 0.3]
    kb = L.vectorSocsKernels(c["P"], c["W"].to(dev), WATER[0], kernels=rank * D, depthWeights=omega, **common)
    assert kb.stacked and kb.planes == F and kb.K == rank * D
    bulk = L.hopkinsIntensity(c["M"], kb, N)
    for f in range(F):
        want = sum(o * abbe[f * D + d].cpu().double() for d, o in enumerate(omega))
        _check(f"{mode} bulk focus plane {f}: one kernel set (K {kb.K}) vs sum_d w_d Abbe_d", bulk[f], want)
        tr = sum(o * float(k.trace[f * D + d]) for d, o in enumerate(omega))
        print(f"  trace {float(kb.trace[f]):.6f}, weighted sum {tr:.6f}, captured {float(kb.captured[f]):.8f}")
        assert abs(float(kb.trace[f]) - tr) <= 1e-6 * tr
    assert float((kb.captured - 1.0).abs().max()) < 1e-5


# ---- 3. physics on the device -----------------------------------------------------------------------------------------------------
def _constant_images(L, dev, stack, depths):
    """A clear mask (its spectrum is one at the grid centre, zero elsewhere), one on-axis source point, "x" polarisation: the
    image at every depth is a constant; returns the D constants in float64."""
    pn, N = 32, 64
    P = torch.ones((pn, pn), dtype=torch.complex64, device=dev)
    W = torch.zeros((pn, pn), dtype=torch.float32, device=dev)
    W[pn // 2, pn // 2] = 1.0
    M = torch.zeros((pn, pn), dtype=torch.complex64, device=dev)
    M[pn // 2, pn // 2] = 1.0
    k = L.vectorSocsKernels(P, W, WATER[0], polarization="x", mediumIndex=WATER[1], wavelength=WL, kernels=3, oversample=0,
                            film=stack, depths=depths)
    img = L.hopkinsIntensity(M, k, N).cpu().double()
    flat = float(((img.amax(dim=(1, 2)) - img.amin(dim=(1, 2))) / img.mean(dim=(1, 2))).max())
    assert flat < 1e-5, flat
    return img.mean(dim=(1, 2)).numpy()


def test_standing_wave_and_absorption_on_the_device(L, dev):
    """Normal incidence, closed forms written out here.  A lossless resist n_r of thickness d on silicon: with
    r = (n_r - n_s) / (n_r + n_s), |u(z)|^2 is proportional to |1 + r exp(-4 pi i n_r (d - z) / lambda)|^2.  An absorbing resist on
    a substrate of its own index: exp(-4 pi k z / lambda).  Ratios of the images to 1e-5."""
    n_r, d = 1.7, 120.0
    depths = [7.0, 40.0, 95.0]
    I = _constant_images(L, dev, L.FilmStack([(n_r, 0.0, d)], FO.SILICON, 0), depths)
    r = (n_r - complex(FO.SILICON[0], -FO.SILICON[1])) / (n_r + complex(FO.SILICON[0], -FO.SILICON[1]))
    u2 = np.abs(1.0 + r * np.exp(-4j * np.pi * n_r * (d - np.array(depths)) / WL)) ** 2
    for i in (1, 2):
        got, want = I[0] / I[i], u2[0] / u2[i]
        print(f"standing wave: I({depths[0]}) / I({depths[i]}) = {got:.7f}, closed form {want:.7f}, off by {abs(got / want - 1):.1e}")
        assert abs(got / want - 1.0) <= 1e-5
    assert u2.max() / u2.min() > 2.0                                              # a real standing wave
    k = 0.08
    I = _constant_images(L, dev, L.FilmStack([(n_r, k, d)], (n_r, k), 0), depths)
    for i in (1, 2):
        got, want = I[0] / I[i], np.exp(-4.0 * np.pi * k * (depths[0] - depths[i]) / WL)
        print(f"absorption: I({depths[0]}) / I({depths[i]}) = {got:.7f}, closed form {want:.7f}, off by {abs(got / want - 1):.1e}")
        assert abs(got / want - 1.0) <= 1e-5


# ---- 4. film=None is the code path of before ---------------------------------------------------------------------------------------
def test_without_a_film_nothing_moved(L, dev):
    """vectorSocsKernels without the new keywords against the path it ran before they existed, restated here from vectorPupils,
    vector._VectorOperator and socs._factorise: the same bits."""
    from functools import partial
    from lithographysimulator_amd import socs as S, vector as V
    P, W, M, N = VO.six_points()
    P, W = P.to(torch.complex64).to(dev), W.to(dev)
    zs = [-80.0, 30.0]
    k = L.vectorSocsKernels(P, W, WATER[0], polarization="te", degree=0.6, mediumIndex=WATER[1], radiometric=True, defocus=zs,
                            wavelength=WL, kernels=20, oversample=6)

    def planes_of(Wm, d):
        pol = L.sourcePolarization(W, "te", 0.6)
        Q = L.vectorPupils(P.reshape(1, 32, 32), WATER[0], WATER[1], True, np.array(zs), WL)
        wsh = torch.fft.ifftshift(pol, dim=(-2, -1)).to(d).contiguous()
        sxx, syy, sxy = pol.to(torch.float64).sum(dim=(1, 2)).tolist()
        for Qp in Q:
            Qp = Qp.contiguous()
            q = Qp.to(torch.complex128)
            gxx, gyy = float((q[0::2].abs() ** 2).sum()), float((q[1::2].abs() ** 2).sum())
            gxy = float((q[0::2] * q[1::2].conj()).sum().real)
            yield (Qp != 0).any(dim=0), sxx * gxx + syy * gyy + 2.0 * sxy * gxy, partial(V._VectorOperator, Qp, wsh, 8 << 30)

    ref = S._factorise("vectorSocsKernels", P.device, 32, 2, True, W, 5, planes_of, kernels=20, oversample=6, iterations=2, seed=0,
                       applier=None)
    assert torch.equal(torch.view_as_real(k.kernels), torch.view_as_real(ref.kernels))
    assert torch.equal(k.eigenvalues, ref.eigenvalues) and torch.equal(k.trace, ref.trace) and k.boxes == ref.boxes
    print(f"film=None: {tuple(k.kernels.shape)} kernels, eigenvalues and traces equal bit for bit; captured {k.captured.tolist()}")
