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
    import lithographysimulator_amd as L
    k = torch.zeros((planes, K, pn, pn) if planes > 1 else (K, pn, pn), dtype=torch.complex64)
    return L.SOCSKernels(k, torch.ones(K, dtype=torch.float64), 1.0, 1.0, 1.0, K, [None] * planes)


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
