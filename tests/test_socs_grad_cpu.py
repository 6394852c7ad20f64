"""Mask gradients on the CPU: the float64 definitions of tests/socs_grad_oracle.py against finite differences and against the
yardsticks of oracle/abbe_oracle.py, and the host pieces of lithographysimulator_amd/ilt.py that need no GPU (the resize matrix,
the argument checks, the descent loop on injected callables).  Every test prints what it observed (-s)."""
import math

import numpy as np
import pytest
import torch

import socs_grad_oracle as GO
import socs_oracle as SO
from helpers import NA, PS, TOL_IMAGE_L2, TOL_IMAGE_MAX, WL
from oracle import abbe_oracle as O

REGIME_CASES = [(pn, name) for pn in (32, 64) for name in ("shrink", "crop", "copy")]


def _complex_randn(shape, gen):
    return torch.view_as_complex(torch.randn(tuple(shape) + (2,), generator=gen, dtype=torch.float64))


# ---- the gradient formula --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain32", "wrap32", "focus64"])
@pytest.mark.parametrize("K", [3, None])
def test_gradient_against_central_differences(name, K):
    """l = sum G . I is exactly quadratic in M, so a central difference with h = 1e-6 ||M|| leaves float64 rounding only
    (~ eps64 / h = 1e-10); the directional derivative along 4 random complex dM equals Re <g, dM> to 1e-7 relative."""
    P, W, M, N = SO.problem(name)
    phi = torch.from_numpy(SO.exact_kernels(P.numpy(), W.numpy(), K)[0])
    Mc = M.to(torch.complex128)
    G = GO.random_G(tuple(M.shape), 3).double()
    assert bool((G < 0).any()) and bool((G > 0).any()) and bool((G == 0).any())
    g = GO.gradient(phi, Mc, N, G)
    gen = torch.Generator().manual_seed(17)
    for d in range(4):
        dM = _complex_randn(M.shape, gen)
        dM = dM / torch.linalg.norm(dM)
        h = 1e-6 * float(torch.linalg.norm(Mc))
        fd = (float((G * GO.intensity(phi, Mc + h * dM, N)).sum()) - float((G * GO.intensity(phi, Mc - h * dM, N)).sum())) / (2 * h)
        an = GO.inner(g, dM)
        rel = abs(fd - an) / abs(an)
        print(f"{name} K {phi.shape[0]} direction {d}: central difference {fd:.12e}, Re<g,dM> {an:.12e}, relative {rel:.2e}")
        assert rel < 1e-7


def test_gradient_sums_over_the_planes_of_a_stack():
    """Two planes (the kernels of a pupil and of its conjugate), a G per plane: g is the sum of the planes' own gradients, and
    finite differences of sum_p sum G_p . I_p agree with it."""
    P, W, M, N = SO.problem("plain32")
    phi = torch.stack([torch.from_numpy(SO.exact_kernels(p.numpy(), W.numpy(), 3)[0]) for p in (P, P.conj().resolve_conj())])
    Mc = M.to(torch.complex128)
    G = GO.random_G((2,) + tuple(M.shape), 4).double()
    g = GO.gradient(phi, Mc, N, G)
    assert tuple(GO.intensity(phi, Mc, N).shape) == (2, 32, 32) and tuple(g.shape) == (32, 32)
    per_plane = GO.gradient(phi[0], Mc, N, G[0]) + GO.gradient(phi[1], Mc, N, G[1])
    assert float((g - per_plane).abs().max() / g.abs().max()) < 1e-14
    gen = torch.Generator().manual_seed(18)
    for d in range(4):
        # a random direction plus the unit gradient: the derivative is then of the size of ||g||, so the central difference's
        # rounding (eps64 |l| / h) stays as far below it as the 1e-7 assumes; a wrong g gives another number than the difference
        dM = _complex_randn(M.shape, gen)
        dM = dM / torch.linalg.norm(dM) + g / torch.linalg.norm(g)
        h = 1e-6 * float(torch.linalg.norm(Mc))
        fd = (float((G * GO.intensity(phi, Mc + h * dM, N)).sum()) - float((G * GO.intensity(phi, Mc - h * dM, N)).sum())) / (2 * h)
        rel = abs(fd - GO.inner(g, dM)) / abs(fd)
        print(f"two planes, direction {d}: relative {rel:.2e}")
        assert rel < 1e-7


def test_fp32_floor_of_the_gradient_formula():
    """The fp32 floor the device bound is derived from (socs_grad_oracle.py, "Gradient tolerance"): the same formula in torch's CPU
    complex64 against float64 on the GPU tests' cases.  Both figures lie below a quarter of the project's image tolerances, so
    those are the gradient's bounds; the constants in socs_grad_oracle.py are what this printed when they were chosen."""
    worst_max = worst_l2 = 0.0
    cases = [GO.sized_case(pn, N, K, planes) + (N,) for pn, N in GO.GRAD_SIZES + GO.EXTRA_SIZES for K in (1, 2, 5) for planes in (1, 2)]
    cases += [GO.sized_case(pn, N, 2, 1) + (N,) for pn, N in GO.LARGE_GRAD_SIZES]
    for name in ("plain32", "wrap32"):
        P, W, M, N = SO.problem(name)
        phi = torch.from_numpy(SO.exact_kernels(P.numpy(), W.numpy(), None)[0]).to(torch.complex64)
        cases.append((phi, M, GO.random_G(tuple(M.shape), 9), N))
    for k, M, G, N in cases:
        g64, g32 = GO.gradient(k, M, N, G), GO.gradient(k, M, N, G, dtype=torch.complex64)
        d = g32.to(torch.complex128) - g64
        worst_max = max(worst_max, float(d.abs().max() / g64.abs().max()))
        worst_l2 = max(worst_l2, float(torch.linalg.norm(d) / torch.linalg.norm(g64)))
    print(f"complex64 formula vs float64 over {len(cases)} cases: max {worst_max:.2e} (recorded {GO.FP32_FLOOR_MAX:.1e}, a quarter "
          f"of the image bound {TOL_IMAGE_MAX / 4:.1e}), l2 {worst_l2:.2e} (recorded {GO.FP32_FLOOR_L2:.1e}, a quarter "
          f"{TOL_IMAGE_L2 / 4:.2e})")
    assert worst_max < TOL_IMAGE_MAX / 4 and worst_l2 < TOL_IMAGE_L2 / 4
    assert GO.FP32_FLOOR_MAX < TOL_IMAGE_MAX / 4 and GO.FP32_FLOOR_L2 < TOL_IMAGE_L2 / 4
    assert (GO.TOL_GRAD_MAX, GO.TOL_GRAD_L2) == (TOL_IMAGE_MAX, TOL_IMAGE_L2)


# ---- the bookends ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", [32, 64])
def test_the_epsilon_cases_land_in_their_regimes(pn):
    r = GO.epsilon_regimes(pn)
    for name, (ps, eps, N) in r.items():
        print(f"pn {pn} {name}: pixelSize {ps:.6f}, epsilon {eps:.6f}, N {N}, resized {math.floor(pn * eps)}, pad {(N - math.floor(pn * eps)) // 2}")
        assert N >= pn
    assert r["shrink"][1] < 1 and math.floor(pn * r["shrink"][1]) < pn
    assert r["crop"][1] > 1 and (r["crop"][2] - math.floor(pn * r["crop"][1])) // 2 < 0
    assert math.floor(pn * r["copy"][1]) == pn and r["copy"][1] != 1.0


@pytest.mark.parametrize("pn,name", REGIME_CASES)
def test_oracle_adjoints_by_the_dot_product_test(pn, name):
    """<A x, y> = <x, A^H y> for the oracle's dense-matrix adjoints against the op-for-op chains: the mask spectrum restated for
    a complex transmission (float64 on the yardstick's fp32 weights: 1e-12) and O.post_process itself (fp32: GO.TOL_ADJOINT)."""
    ps, eps, N = GO.epsilon_regimes(pn)[name]
    gen = torch.Generator().manual_seed(pn + len(name))
    t, y = _complex_randn((pn, pn), gen), _complex_randn((pn, pn), gen)
    St = GO.spectrum_complex(t, eps, N)
    gap = abs(complex((St.conj() * y).sum()) - complex((t.conj() * GO.spectrum_adjoint(y, pn, eps, N)).sum()))
    rel_s = gap / float(torch.linalg.norm(St) * torch.linalg.norm(y))
    also = float((GO.spectrum_matrix(pn, eps, N) @ t @ GO.spectrum_matrix(pn, eps, N).T - St).abs().max() / St.abs().max())
    raw = torch.rand((pn, pn), generator=gen, dtype=torch.float64).to(torch.float32)
    img = O.post_process(raw, eps)
    gy = torch.randn(tuple(img.shape), generator=gen, dtype=torch.float64)
    gap_p = abs(float((img.double() * gy).sum()) - float((raw.double() * GO.postprocess_adjoint(gy, pn, eps)).sum()))
    rel_p = gap_p / float(torch.linalg.norm(img.double()) * torch.linalg.norm(gy))
    print(f"pn {pn} {name}: spectrum {rel_s:.2e} (B t B^T vs the chain {also:.2e}), post-process {rel_p:.2e}, image {tuple(img.shape)}")
    assert rel_s < 1e-12 and also < 1e-12 and rel_p < GO.TOL_ADJOINT


@pytest.mark.parametrize("pn", [32, 64])
def test_the_complex_chain_is_the_yardsticks_on_a_binary_mask(pn):
    from lithographysimulator_amd.synthetic import bernoulli_mask
    geo = bernoulli_mask(pn)
    eps, N = O.calculate_epsilon_n(4 / pn, PS, WL)
    want = O.mask_spectrum(geo, PS, WL)
    got = GO.spectrum_complex(geo.to(torch.complex128), eps, N)
    e = float((got - want.to(torch.complex128)).abs().max() / want.abs().max())
    print(f"pn {pn}: restated chain vs O.mask_spectrum {e:.2e}")
    assert e < 2e-6


@pytest.mark.parametrize("pn,name", REGIME_CASES)
def test_resize_matrix_is_the_yardsticks_bit_for_bit(pn, name):
    """The package's R against O.bilinear_resize applied to probe images, for the spectrum's scale and the post-process's."""
    from lithographysimulator_amd.ilt import resizeMatrix
    ps, eps, N = GO.epsilon_regimes(pn)[name]
    for scale in (eps, 1.0 / eps):
        R, n = resizeMatrix(pn, scale)
        want = GO.resize_matrix(pn, scale)
        assert n == want.shape[0] == math.floor(pn * scale)
        if R is None:
            assert n == pn and torch.equal(want, torch.eye(pn, dtype=torch.float64))
        else:
            assert R.dtype == torch.float32 and torch.equal(R.double(), want)
            assert int((R != 0).sum(dim=1).max()) <= 2
    assert (resizeMatrix(pn, eps)[0] is None) == (name == "copy")


@pytest.mark.parametrize("pn,name", REGIME_CASES)
def test_package_adjoints_on_the_host(pn, name):
    """maskSpectrumAdjoint with torch's inverse DFT in place of the device's, and postProcessAdjoint (torch alone), against the
    oracle's dense matrices."""
    from lithographysimulator_amd.ilt import maskSpectrumAdjoint, postProcessAdjoint
    ps, eps, N = GO.epsilon_regimes(pn)[name]
    gen = torch.Generator().manual_seed(5)
    y = _complex_randn((pn, pn), gen).to(torch.complex64)
    got = maskSpectrumAdjoint(y, pn, eps, N, transform=lambda x: torch.fft.ifft2(x, norm="forward"))
    want = GO.spectrum_adjoint(y, pn, eps, N)
    e_s = float((got - want).abs().max() / want.abs().max())
    n_out = GO.postprocess_matrix(pn, eps).shape[0]
    gy = torch.randn((2, n_out, n_out), generator=gen, dtype=torch.float64).to(torch.float32)
    back = postProcessAdjoint(gy, pn, eps)
    want_p = torch.stack([GO.postprocess_adjoint(gy[i], pn, eps) for i in range(2)])
    e_p = float((back - want_p).abs().max() / want_p.abs().max())
    print(f"pn {pn} {name}: S^H {e_s:.2e}, post-process adjoint {e_p:.2e}")
    assert got.dtype == torch.complex64 and tuple(got.shape) == (pn, pn) and e_s < 2e-6
    assert back.dtype == torch.float32 and tuple(back.shape) == (2, pn, pn) and e_p < 2e-6
    assert tuple(postProcessAdjoint(gy[0], pn, eps).shape) == (pn, pn)


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def _cpu_socs(pn=32, K=3, planes=1):
    return GO.socs_around(torch.zeros((planes, K, pn, pn) if planes > 1 else (K, pn, pn), dtype=torch.complex64), "cpu")


def test_gradient_argument_errors():
    import lithographysimulator_amd as L
    from lithographysimulator_amd.imageformation import ShapeError
    s = _cpu_socs()
    M, G = torch.zeros((32, 32), dtype=torch.complex64), torch.zeros((32, 32))
    for fn in (lambda: L.hopkinsGradient(M, "kernels", 64, G), lambda: L.hopkinsFields(M, None, 64)):
        with pytest.raises(TypeError):
            fn()
    for fn in (lambda: L.hopkinsGradient(M[:16], s, 64, G), lambda: L.hopkinsFields(M[None], s, 64),
               lambda: L.hopkinsIntensityAD(M[:, :16], s, 64)):
        with pytest.raises(ShapeError):
            fn()
    with pytest.raises(ShapeError, match="complex64"):                           # a complex128 leaf would be imaged in fp32 silently
        L.hopkinsIntensityAD(M.to(torch.complex128), s, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # a CPU tensor: there is no fall-back
        L.hopkinsGradient(M, s, 64, G)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.hopkinsFields(M, s, 64)
    for bad in (4097, 8192, 48, 8):
        with pytest.raises(ValueError):
            L.maskSpectrumAdjoint(M, 32, 1.0, bad)
    with pytest.raises(ValueError):
        L.maskSpectrumAdjoint(M, 32, 1.0, 16)                                    # N < pn
    with pytest.raises(ShapeError):
        L.maskSpectrumAdjoint(M[:16], 32, 1.0, 64, transform=lambda x: x)
    with pytest.raises(ShapeError):
        L.postProcessAdjoint(torch.zeros((31, 31)), 32, 1.0)


def test_the_abi_refuses_bad_sizes_without_a_device():
    """Every check of litho_socs_fields / litho_socs_vjp is made before any launch, so the codes come back on a machine without a
    GPU too (the pointers are never dereferenced on the host)."""
    from lithographysimulator_amd import _native as nat
    lib = nat.lib()
    buf = torch.zeros(64, dtype=torch.complex64)
    p = nat.ptr(buf)
    assert lib.litho_socs_vjp_work_bytes(2, 3, 32) == 2 * 3 * 32 * 32 * 8
    for bad in ((0, 3, 32), (2, 0, 32), (2, 3, 33), (2, 3, 8), (2, 3, 8192), (2, 3, 48)):
        assert lib.litho_socs_vjp_work_bytes(*bad) == 0
    for pn, N, rc in ((33, 64, nat.E_ARG), (8, 64, nat.E_ARG), (8192, 8192, nat.E_ARG), (48, 64, nat.E_ARG), (32, 48, nat.E_ARG),
                      (32, 8192, nat.E_ARG), (64, 32, nat.E_NSMALL), (4096, 2048, nat.E_NSMALL)):
        assert lib.litho_socs_fields(p, p, 1, pn, N, p, None) == rc, (pn, N)
        assert lib.litho_socs_vjp(p, p, p, 1, 1, pn, N, p, 0, p, 1 << 40, None) == rc, (pn, N)
    assert lib.litho_socs_fields(p, p, 0, 32, 64, p, None) == nat.E_ARG
    for null in range(3):
        args = [p, p, 1, 32, 64, p, None]
        args[(0, 1, 5)[null]] = None
        assert lib.litho_socs_fields(*args) == nat.E_ARG
    for null in (0, 1, 2, 7, 9):
        args = [p, p, p, 1, 1, 32, 64, p, 0, p, 1 << 40, None]
        args[null] = None
        assert lib.litho_socs_vjp(*args) == nat.E_ARG
    assert lib.litho_socs_vjp(p, p, p, 0, 1, 32, 64, p, 0, p, 1 << 40, None) == nat.E_ARG
    assert lib.litho_socs_vjp(p, p, p, 1, 0, 32, 64, p, 0, p, 1 << 40, None) == nat.E_ARG
    assert lib.litho_socs_vjp(p, p, p, 2, 3, 32, 64, p, 0, p, 2 * 3 * 32 * 32 * 8 - 1, None) == nat.E_WORKSPACE


# ---- the loop --------------------------------------------------------------------------------------------------------------------
class _Grid:
    def __init__(self, pn):
        self.pn = pn


def _oracle_loop_setting(pn, contacts):
    """Ideal pupil, 40 strided points of the annular 0.4-0.8 source at full rank, helpers' pixel and wavelength; the threshold is
    0.3 of the clear field.  Returns (target, imager, adjoint, threshold)."""
    P = O.pupil_function(None, pn, NA, WL)
    W = SO.strided_points(O.source_annular(0.4, 0.8, pn), 40).to(torch.float32)
    phi = torch.from_numpy(SO.exact_kernels(P.numpy(), W.numpy(), None)[0])
    eps, N = O.calculate_epsilon_n(4 / pn, PS, WL)
    imager, adjoint = GO.model(phi, pn, eps, N, gain=1.0 / float(W.sum()))
    n_out = GO.postprocess_matrix(pn, eps).shape[0]
    target = torch.zeros((n_out, n_out))
    for r, c, s in contacts:
        target[r:r + s, c:c + s] = 1.0
    clear = imager(torch.ones((pn, pn), dtype=torch.complex64))
    return target, imager, adjoint, 0.3 * float(clear[n_out // 2, n_out // 2])


def test_optimize_mask_descends_on_the_oracle_chain():
    import lithographysimulator_amd as L
    target, imager, adjoint, threshold = _oracle_loop_setting(32, [(10, 10, 5), (18, 20, 5)])
    res = L.optimizeMask(target, _Grid(32), PS, 4 / 32, WL, threshold, iterations=10, imager=imager, adjoint=adjoint)
    print(f"pn 32, 10 iterations: losses {['%.5f' % v for v in res.losses]}, best {res.best}")
    assert len(res.losses) == 11 and all(math.isfinite(v) for v in res.losses)
    assert res.losses[10] < res.losses[0]
    assert res.best == int(np.argmin(res.losses)) and res.losses[res.best] < res.losses[0]
    assert res.mask.dtype == torch.bool and tuple(res.mask.shape) == (32, 32) and torch.equal(res.mask, res.theta > 0)
    assert res.transmission.dtype == torch.complex64 and tuple(res.transmission.shape) == (32, 32)
    # the returned iterate is the best one: imaging its transmission gives that loss again
    resist = torch.sigmoid((25.0 / threshold) * (imager(res.transmission) - threshold))
    again = float(((resist - target) ** 2).mean())
    assert abs(again - res.losses[res.best]) < 1e-6 * res.losses[res.best]


def test_optimize_mask_the_setting_of_the_device_test():
    """pn 64, two isolated contacts, 12 iterations, the defaults: the reference chain alone meets the device test's condition."""
    import lithographysimulator_amd as L
    target, imager, adjoint, threshold = _oracle_loop_setting(64, [(20, 20, 6), (38, 40, 6)])
    res = L.optimizeMask(target, _Grid(64), PS, 4 / 64, WL, threshold, iterations=12, imager=imager, adjoint=adjoint)
    print(f"pn 64, 12 iterations: losses {['%.6f' % v for v in res.losses]}, best {res.best}")
    assert res.losses[res.best] < res.losses[0] and res.best == int(np.argmin(res.losses))
    # an attenuated phase-shift mask: complex background, an `initial` of its own
    res2 = L.optimizeMask(target, _Grid(64), PS, 4 / 64, WL, threshold, iterations=4, background=-math.sqrt(0.06), imager=imager,
                          adjoint=adjoint, initial=res.theta)
    assert bool((res2.transmission.real < 0).any()) and all(math.isfinite(v) for v in res2.losses)


# ---- the loop against the derivative of its own loss -------------------------------------------------------------------------
LOOP_CASES = [(pn, regime, planes, bg) for pn in (16, 32) for regime in ("shrink", "crop", "copy") for planes in (1, 2)
              for bg in GO.ILT_BACKGROUNDS]
# eps32 = 2^-24, the relative rounding of one fp32 operation.  The loop forms s = sigmoid(a_m theta) in fp32 and, on the device's
# types, theta1 = fl(theta0 - fl(step . fl(g / peak))) with |g / peak| <= 1.  Against g / peak in float64 that leaves, in units of
# eps32: max(|theta0|, |theta1|) / step from the subtraction (the division by step, a power of two, is exact), 2 from the product
# and the quotient, a_m max|theta0| from the rounding of a_m theta carried through s (1 - s) (|d log(s (1 - s)) / dx| = |1 - 2 s|
# <= 1), and 4 from the sigmoid, 1 - s and the two products
EPS32 = 2.0 ** -24


def _update_bound(case, theta1):
    top = max(float(case.theta0.abs().max()), float(theta1.abs().max()))
    return EPS32 * (top / GO.ILT_STEP + 2.0 + GO.ILT_MASK_STEEPNESS * float(case.theta0.abs().max()) + 4.0)

# the measured worst of |fd - <g, d>| / (||g|| ||d||) at h = 3e-3 over LOOP_CASES, 1.27e-4 (see the test's docstring), and the
# bound, 4 times it
FD_WORST_3E3 = 1.3e-4
TOL_FD_3E3 = 4 * FD_WORST_3E3
_runs = {}


def _recorded_run(pn, regime, planes, bg):
    """One optimizeMask(initial=theta0, iterations=1) on the float64 chain with hooks that record what crosses them; made once per
    case and shared by the tests below: (case, result, {"t": transmissions imaged, "grad_image", "grad_t"})."""
    key = (pn, regime, planes, bg)
    if key not in _runs:
        case = GO.ilt_case(pn, regime, planes, GO.ILT_BACKGROUNDS[bg], gain=1.0 / GO.ILT_WEIGHT_SUM)
        imager, adjoint = case.model()
        rec = {"t": [], "grad_image": [], "grad_t": []}

        def rec_imager(t):
            rec["t"].append(t.clone())
            return imager(t)

        def rec_adjoint(g):
            rec["grad_image"].append(g.clone())
            rec["grad_t"].append(adjoint(g))
            return rec["grad_t"][-1]

        _runs[key] = (case, case.loop(rec_imager, rec_adjoint), rec)
    return _runs[key]


@pytest.mark.parametrize("pn,regime,planes,bg", LOOP_CASES)
def test_loop_loss_and_image_gradient_against_the_closed_form(pn, regime, planes, bg):
    """losses[0] is GO.ilt_loss of the oracle image of t(theta0) computed here in float64.  The loop forms t in fp32 / complex64:
    a_m theta rounds at eps32 . 8 under a slope of |span| / 4, the sigmoid, the product and the sum at eps32 |t| each, 5e-7 in
    all (measured 1.4e-7), and the loss follows to 1e-6 relative, the bound of test_optimize_mask_descends_on_the_oracle_chain
    (measured 1.4e-8).  The gradient the loop hands to the adjoint has the image's shape and is 2 a_r dose / numel . diff . r (1 - r)
    with numel over pixels AND planes.  The loop forms it in float64 from the hook's float64 image, so only the rounded t separates
    the two: 5e-7 on t is at most that, relatively, on the image, times the sigmoid's a_r . threshold = 25 on the slope, times 2 for
    the two factors that move with it (diff and r (1 - r)): 2.5e-5 of the maximum (measured 1.7e-6); a count over one plane of
    two is a factor 2."""
    case, res, rec = _recorded_run(pn, regime, planes, bg)
    assert len(res.losses) == 2 and len(rec["t"]) == 2 and len(rec["grad_image"]) == 1
    assert rec["t"][0].dtype == torch.complex64 and tuple(rec["t"][0].shape) == (pn, pn)
    e_t = float((rec["t"][0].to(torch.complex128) - case.t0).abs().max())
    want = GO.ilt_loss(case.image0, case.target, case.threshold, GO.ILT_DOSE, case.a_r)
    e_l = abs(res.losses[0] - want) / want
    G = rec["grad_image"][0]
    shape = (planes, case.n_out, case.n_out) if planes > 1 else (case.n_out, case.n_out)
    assert tuple(G.shape) == shape and not G.is_complex()
    G_want = GO.ilt_grad_image(case.image0, case.target, case.threshold, GO.ILT_DOSE, case.a_r)
    e_g = float((G.double() - G_want).abs().max() / G_want.abs().max())
    print(f"pn {pn} {regime} planes {planes} {bg}: loss {res.losses[0]:.9f} vs {want:.9f} ({e_l:.1e}, bound 1e-6), t {e_t:.1e} (bound 5e-7), "
          f"grad_image {e_g:.1e} (bound 2.5e-5), signs {int((G_want < 0).sum())} / {int((G_want > 0).sum())}")
    assert e_t < 5e-7 and e_l < 1e-6 and e_g < 2.5e-5
    assert bool((G_want < 0).any()) and bool((G_want > 0).any())


@pytest.mark.parametrize("pn,regime,planes,bg", LOOP_CASES)
def test_loop_gradient_is_the_derivative_of_its_loss(pn, regime, planes, bg):
    """g_theta = a_m s (1 - s) Re(grad_t conj(span)) from the recorded adjoint output against the central difference of the loop's
    own loss, read through the public call (initial = theta0 +- h d, iterations = 1, losses[0]) along a seeded random d, at
    h = 1e-2 and 3e-3; the error is |fd - <g, d>| / (||g||_2 ||d||_2).  Measured over the 36 cases:
        h = 1e-2: worst 1.38e-3, median 6.9e-5;  h = 3e-3: worst 1.27e-4 (pn 32, crop, two planes, complex), median 5.7e-6,
        smallest 3.8e-7
    The worst cases fall as h^2 (1.38e-3 -> 1.27e-4); the small ones sit on the floor of the quotient, theta and t being rounded
    to fp32 inside the call, so no convergence ratio between the two steps is asserted.  The bound at h = 3e-3 is 4 times that
    worst, 5.2e-4.  Along a random d a gradient wrong by its own size shows at about 1 / pn of ||g|| ||d||, 0.03 ... 0.06, and a
    count over one plane of two doubles <g, d>; the update test below sees a wrong direction element by element."""
    case, res, rec = _recorded_run(pn, regime, planes, bg)
    g = GO.ilt_grad_theta(case.theta0, rec["grad_t"][0], case.background, 1, GO.ILT_MASK_STEEPNESS)
    d = torch.randn((pn, pn), generator=torch.Generator().manual_seed(pn + planes), dtype=torch.float64)
    dd = float((g * d).sum())
    scale = float(torch.linalg.norm(g) * torch.linalg.norm(d))
    errs = {}
    for h in (1e-2, 3e-3):
        imager, adjoint = case.model()
        lp = case.loop(imager, adjoint, theta=(case.theta0.double() + h * d).to(torch.float32)).losses[0]
        lm = case.loop(imager, adjoint, theta=(case.theta0.double() - h * d).to(torch.float32)).losses[0]
        errs[h] = abs((lp - lm) / (2 * h) - dd) / scale
    print(f"pn {pn} {regime} planes {planes} {bg}: <g,d> {dd:+.6e}, ||g|| ||d|| {scale:.3e}, error {errs[1e-2]:.2e} at h 1e-2, "
          f"{errs[3e-3]:.2e} at h 3e-3 (bound {TOL_FD_3E3:.1e})")
    assert errs[3e-3] < TOL_FD_3E3


@pytest.mark.parametrize("pn,regime,planes,bg", LOOP_CASES)
def test_first_update_is_the_peak_normalised_gradient(pn, regime, planes, bg):
    """Every case descends in its first step on the float64 chain (asserted: best == 1), so the returned theta is theta1 and
    (theta0 - theta1) / step must be g_theta / max|g_theta| of the recorded adjoint output, to the fp32 rounding of the update
    (EPS32 above; the float64 hooks make the loop's theta1 float64, which only lowers the error).  This is the one place where the
    loop's own grad_theta shows: its conjugate on span, its a_m s (1 - s), the peak normalisation and the sign."""
    case, res, rec = _recorded_run(pn, regime, planes, bg)
    assert res.best == 1 and res.losses[1] < res.losses[0], res.losses
    g = GO.ilt_grad_theta(case.theta0, rec["grad_t"][0], case.background, 1, GO.ILT_MASK_STEEPNESS)
    got, want = GO.update_of(case, res), g / g.abs().max()
    bound = _update_bound(case, res.theta)
    e = float((got - want).abs().max())
    print(f"pn {pn} {regime} planes {planes} {bg}: losses {res.losses[0]:.6f} -> {res.losses[1]:.6f}, update error {e:.2e} "
          f"(bound {bound:.2e}), peak {float(got.abs().max()):.7f}")
    assert e < bound
    assert torch.equal(res.mask, res.theta > 0) and res.transmission.dtype == torch.complex64


def _within(measured, recorded):
    """The recorded floor is what this machine printed when the bound was chosen; another host BLAS sums in another order and
    moves it by its own rounding, so the re-check allows a factor 2 -- a floor that has really moved (a changed case, another
    chain) is caught before the device bound built on it means something else."""
    return measured <= 2.0 * recorded


def test_fp32_floor_of_the_loop_chain():
    """The fp32 floors the bounds of tests/test_gpu_ilt.py are derived from (socs_grad_oracle.py, "Loop tolerances"): GO.model in
    torch's CPU complex64 against float64 on exactly the device tests' cases -- the image and the adjoint over
    GO.ILT_DEVICE_CASES, the one-iteration loop (both losses and the update) over GO.ILT_LOOP_CASES."""
    im_max = im_l2 = ad_max = ad_l2 = 0.0
    for key in GO.ILT_DEVICE_CASES:
        case = GO.device_case(*key)
        imager, adjoint = case.model(torch.complex64)
        image = imager(case.t0.to(torch.complex64))
        assert image.dtype == torch.float32
        im_max, im_l2 = max(im_max, GO.rel_max(image, case.image0)), max(im_l2, GO.rel_l2(image, case.image0))
        G = case.grad_image0.to(torch.float32)
        imager64, adjoint64 = case.model()
        imager64(case.t0.to(torch.complex64))
        got, want = adjoint(G), adjoint64(G)
        assert got.dtype == torch.complex64
        ad_max, ad_l2 = max(ad_max, GO.rel_max(got, want)), max(ad_l2, GO.rel_l2(got, want))
    loss = update = 0.0
    for key in GO.ILT_LOOP_CASES:
        case = GO.loop_case(*key)
        ref, got = case.reference(), case.loop(*case.model(torch.complex64))
        assert got.theta.dtype == torch.float32
        loss = max(loss, abs(got.losses[0] - ref.losses[0]) / ref.losses[0], abs(got.losses[1] - ref.losses[1]) / ref.losses[1])
        update = max(update, float((GO.update_of(case, got) - GO.update_of(case, ref)).abs().max()))
    print(f"complex64 chain vs float64: image max {im_max:.2e} (recorded {GO.ILT_FLOOR_IMAGE_MAX:.1e}), l2 {im_l2:.2e} "
          f"({GO.ILT_FLOOR_IMAGE_L2:.1e}); adjoint max {ad_max:.2e} ({GO.ILT_FLOOR_ADJOINT_MAX:.1e}), l2 {ad_l2:.2e} "
          f"({GO.ILT_FLOOR_ADJOINT_L2:.1e}) over {len(GO.ILT_DEVICE_CASES)} cases; loss {loss:.2e} ({GO.ILT_FLOOR_LOSS:.1e}), update "
          f"{update:.2e} ({GO.ILT_FLOOR_UPDATE:.1e}) over {len(GO.ILT_LOOP_CASES)} cases")
    print(f"bounds: image {GO.TOL_ILT_IMAGE_MAX:.1e} / {GO.TOL_ILT_IMAGE_L2:.1e}, adjoint {GO.TOL_ILT_ADJOINT_MAX:.1e} / "
          f"{GO.TOL_ILT_ADJOINT_L2:.1e}, loss {GO.TOL_ILT_LOSS:.1e}, update {GO.TOL_ILT_UPDATE:.1e}")
    assert _within(im_max, GO.ILT_FLOOR_IMAGE_MAX) and _within(im_l2, GO.ILT_FLOOR_IMAGE_L2)
    assert _within(ad_max, GO.ILT_FLOOR_ADJOINT_MAX) and _within(ad_l2, GO.ILT_FLOOR_ADJOINT_L2)
    assert _within(loss, GO.ILT_FLOOR_LOSS) and _within(update, GO.ILT_FLOOR_UPDATE)
    # the project's rule: the image tolerances where the floor is under a quarter of them, four times the floor otherwise
    for floor, tol, bound in ((GO.ILT_FLOOR_IMAGE_MAX, TOL_IMAGE_MAX, GO.TOL_ILT_IMAGE_MAX), (GO.ILT_FLOOR_IMAGE_L2, TOL_IMAGE_L2, GO.TOL_ILT_IMAGE_L2),
                              (GO.ILT_FLOOR_ADJOINT_MAX, TOL_IMAGE_MAX, GO.TOL_ILT_ADJOINT_MAX),
                              (GO.ILT_FLOOR_ADJOINT_L2, TOL_IMAGE_L2, GO.TOL_ILT_ADJOINT_L2)):
        assert bound == (tol if floor < tol / 4 else 4 * floor)
    assert (GO.TOL_ILT_LOSS, GO.TOL_ILT_UPDATE) == (4 * GO.ILT_FLOOR_LOSS, 4 * GO.ILT_FLOOR_UPDATE)


def test_optimize_mask_argument_errors():
    import lithographysimulator_amd as L
    target, imager, adjoint, threshold = _oracle_loop_setting(32, [(10, 10, 5)])
    ok = dict(imager=imager, adjoint=adjoint)
    with pytest.raises(ValueError, match="together"):
        L.optimizeMask(target, _Grid(32), PS, 4 / 32, WL, threshold, imager=imager)
    for kw in (dict(iterations=0), dict(step=0.0), dict(maskSteepness=-1.0), dict(resistSteepness=0.0), dict(feature=0.5, background=0.5),
               dict(initial=torch.zeros((16, 16)))):
        with pytest.raises(ValueError):
            L.optimizeMask(target, _Grid(32), PS, 4 / 32, WL, threshold, **ok, **kw)
    with pytest.raises(ValueError):
        L.optimizeMask(target[:, :5], _Grid(32), PS, 4 / 32, WL, threshold, **ok)
    with pytest.raises(TypeError):                                               # the device model needs real kernels
        L.optimizeMask(target, _Grid(32), PS, 4 / 32, WL, threshold)
