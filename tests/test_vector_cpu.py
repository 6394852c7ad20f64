"""Vector (polarised, high-NA) imaging on the CPU: the identities behind the vector transmission cross coefficient
(tests/vector_oracle.py, float64), the oracle pinned to physics (two-beam closed form) and to the scalar Abbe sum (low-NA limit),
and the host side of lithographysimulator_amd/vector.py -- sourcePolarization, the J clamp, box, trace and captured fraction of
vectorSocsKernels run with `applier=` set to the oracle's operator, the refusals of vectorAbbeIntensity and
correctLayout(socs=).  No GPU is involved.  Every test prints what it observed (-s)."""
import numpy as np
import pytest
import torch

import socs_oracle as SO
import vector_oracle as VO
from helpers import DEMO_AB, NA, TOL_IMAGE_L2, TOL_IMAGE_MAX, WL, f16, rel_l2, rel_max
from oracle import abbe_oracle as O

MODES = [("x", 1.0), ("te", 1.0), ("tm", 1.0), ("unpolarized", 1.0), ("te", 0.5)]


def small():
    """pn 16, the demo pupil, 5 source points with grey weights (one of them at the centre, where TE / TM fall back to y / x)."""
    P = O.pupil_function(f16(DEMO_AB), 16, NA, WL).numpy().astype(np.complex128)
    W = np.zeros((16, 16))
    for (r, c), w in zip([(8, 8), (8, 11), (5, 8), (10, 6), (6, 10)], [1.0, 0.5, 1.5, 0.8, 1.2]):
        W[r, c] = w
    return P, W


@pytest.mark.parametrize("NA_,n", VO.OPTICS)
def test_factor_columns_are_orthonormal(NA_, n):
    for pn in (16, 30, 64):
        M = VO.factors(pn, NA_, n).reshape(3, 2, pn, pn)
        a, b, g, inside = VO.cosines(pn, NA_, n)
        nxx, nyy, nxy = (M[:, 0] ** 2).sum(0), (M[:, 1] ** 2).sum(0), (M[:, 0] * M[:, 1]).sum(0)
        e = max(np.abs(nxx - 1)[inside].max(), np.abs(nyy - 1)[inside].max(), np.abs(nxy)[inside].max())
        R = VO.factors(pn, NA_, n, radiometric=True).reshape(3, 2, pn, pn)
        e_r = max(np.abs((R[:, j] ** 2).sum(0) * g - 1)[inside].max() for j in (0, 1))
        print(f"NA {NA_} n {n} pn {pn}: {int(inside.sum())} cells inside, orthonormality {e:.1e}, radiometric norms g {e_r:.1e}")
        assert e <= 1e-14 and e_r <= 1e-13
        assert not M[:, :, ~inside].any() and ((~inside).any() == (NA_ / n * 2 * np.sqrt(2) >= 1))


@pytest.mark.parametrize("radiometric", [False, True])
@pytest.mark.parametrize("NA_,n", VO.OPTICS)
def test_operator_formula_rank_and_trace(NA_, n, radiometric):
    P, W = small()
    S = int((W > 0).sum())
    Q = VO.vector_pupils(P, NA_, n, radiometric)
    X = np.random.default_rng(3).standard_normal((2, 16, 16)) + 1j * np.random.default_rng(4).standard_normal((2, 16, 16))
    for mode, degree in MODES:
        A = VO.explicit_rows(Q, W, mode, degree)
        T = SO.tcc(A)
        want = (T @ X.reshape(2, -1).T).T.reshape(2, 16, 16)
        maps = VO.weight_maps(W, mode, degree)
        got = VO.fft_apply(Q, maps, X)
        e = np.abs(got - want).max() / np.abs(want).max()
        rank = int(np.linalg.matrix_rank(A))
        pure = mode != "unpolarized" and degree == 1.0
        tr, tr_formula = float(np.trace(T).real), VO.trace(Q, maps)
        scalar = float(W.sum()) * float((np.abs(P) ** 2)[VO.cosines(16, NA_, n)[3]].sum())
        print(f"NA {NA_} n {n} radiometric {radiometric} {mode} degree {degree}: formula vs explicit {e:.1e}, rank {rank} "
              f"({3 if pure else 5} S = {(3 if pure else 5) * S}), trace {tr:.6f}, formula {tr_formula:.6f}, scalar {scalar:.6f}")
        assert e <= 1e-12
        assert rank == (3 if pure else 5) * S
        assert abs(tr - tr_formula) <= 1e-12 * tr
        if not radiometric:
            assert abs(tr - scalar) <= 1e-12 * scalar
        else:
            assert tr > scalar


def test_low_na_limit_is_the_scalar_abbe_sum():
    P, W, M, N = SO.problem("wrap32")
    na, n = 0.01, 1.0
    img = VO.abbe_truth(VO.vector_pupils(P.numpy(), na, n), M, W.numpy(), "unpolarized", 1.0, N)
    scalar = SO.truth("wrap32")
    e = float((img - scalar).abs().max() / scalar.max())
    print(f"NA {na}: unpolarised vector image vs scalar Abbe sum {e:.2e} of the maximum (bound {2 * (na / n) ** 2:.1e})")
    assert e <= 2 * (na / n) ** 2


def test_two_beam_closed_form():
    """One on-axis source point, two equal orders at +-f on the x axis: y-polarised (TE) light keeps contrast 1, x-polarised (TM)
    light has contrast |cos 2 theta|, reversed beyond 45 degrees:  I = 2 + 2 C cos(2 . 2 pi k (q - c) / N) along x, C = 1 (TE),
    cos 2 theta (TM), sin theta = NA sigma_f / n."""
    pn, N, k = 32, 64, 7
    sx, sy = VO.sigma_grid(pn)
    P = (sx * sx + sy * sy <= 1.0).astype(np.complex128)
    W = np.zeros((pn, pn))
    W[pn // 2, pn // 2] = 1.0
    M = np.zeros((pn, pn), dtype=np.complex128)
    M[pn // 2, pn // 2 + k] = M[pn // 2, pn // 2 - k] = 1.0
    sigma_f = k * 4.0 / pn
    x = np.arange(pn) - pn // 2
    fringe = np.cos(2 * 2 * np.pi * k * x / N)
    for na, n in VO.OPTICS:
        sin_t = na * sigma_f / n
        c2 = 1 - 2 * sin_t ** 2
        Q = VO.vector_pupils(P, na, n)
        for mode, C in (("y", 1.0), ("x", c2), ("te", 1.0), ("tm", c2)):        # at d = 0 TE means y and TM means x
            img = VO.abbe_truth(Q, M, W, mode, 1.0, N).numpy()
            want = np.broadcast_to(2 + 2 * C * fringe[None, :], (pn, pn))
            e = np.abs(img - want).max()
            row = img[pn // 2]
            print(f"NA {na} n {n} theta {np.degrees(np.arcsin(sin_t)):.1f} deg, {mode}: contrast {C:+.4f} (|cos 2 theta| "
                  f"{abs(c2):.4f}), closed form {e:.1e}; centre {row[pn // 2]:.4f}, mean {row.mean():.4f}")
            assert e <= 1e-12
        if na / n > 0.9:
            assert sin_t > np.sin(np.pi / 4) and c2 < 0            # beyond 45 degrees: the TM fringes are reversed
            tm = VO.abbe_truth(Q, M, W, "x", 1.0, N).numpy()[pn // 2]
            assert tm[pn // 2] < 2.0 < VO.abbe_truth(Q, M, W, "y", 1.0, N).numpy()[pn // 2, pn // 2]


def test_defocus_phase_is_the_paraxial_one_to_fourth_order():
    pn, na, n, z = 64, 0.05, 1.0, 100.0
    sx, sy = VO.sigma_grid(pn)
    a, b, g, inside = VO.cosines(pn, na, n)
    assert inside.all()
    exact = np.angle(VO.defocus_phase(pn, na, n, z, WL))
    s = (na / n) ** 2 * (sx * sx + sy * sy)
    paraxial = 2 * np.pi * z * na ** 2 * (sx * sx + sy * sy) / (2 * n * WL)
    assert np.abs(paraxial).max() < np.pi                                         # no wrap of the angle
    ap = sx * sx + sy * sy <= 1.0                                                 # the aperture: where a pupil has light
    diff = exact - paraxial
    hi = 2 * np.pi * n * z / WL * s * s / (8 * (1 - s))                           # 1 - sqrt(1-s) - s/2 in [s^2/8, s^2/(8(1-s))]
    lo = 2 * np.pi * n * z / WL * s * s / 8
    assert hi[ap].max() < 1e-3 * np.abs(exact[ap]).max()
    print(f"defocus {z} nm at NA {na}: phase up to {np.abs(exact).max():.3e}, exact - paraxial up to {np.abs(diff).max():.3e} "
          f"(fourth-order bound {hi.max():.3e})")
    assert (diff >= lo - 1e-14).all() and (diff <= hi + 1e-14).all()
    assert (np.angle(VO.defocus_phase(pn, na, n, -z, WL)) == -exact).all()


# ---- the package's host side ----------------------------------------------------------------------------------------------------
def test_source_polarization_maps_and_errors():
    import lithographysimulator_amd as L
    P, W, M, N = VO.six_points()
    for mode, degree in MODES + [("y", 1.0), ("tm", 0.25)]:
        got = L.sourcePolarization(W, mode, degree)
        want = VO.weight_maps(W.numpy(), mode, degree)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 32, 32) and got.device.type == "cpu"
        assert np.abs(got.numpy() - want).max() <= 2.0 ** -24 * np.abs(want).max()
    ex, ey = VO.directions(32, "te")
    maps = L.sourcePolarization(W, (torch.from_numpy(3.0 * ex), torch.from_numpy(3.0 * ey)), 1.0)      # normalised per point
    assert float((maps - L.sourcePolarization(W, "te")).abs().max()) <= 2.0 ** -22 * float(W.max())
    bitmap = (W > 0).to(torch.uint8)
    assert torch.equal(L.sourcePolarization(bitmap, "x")[0], (W > 0).to(torch.float32))
    centre = torch.zeros((32, 32))
    centre[16, 16] = 2.0
    assert torch.equal(L.sourcePolarization(centre, "tm"), L.sourcePolarization(centre, "x"))
    assert torch.equal(L.sourcePolarization(centre, "te"), L.sourcePolarization(centre, "y"))
    for bad in (dict(mode="circular"), dict(mode="x", degree=1.5), dict(mode="te", degree=-0.1),
                dict(mode=(torch.zeros(32, 32), torch.zeros(32, 32))), dict(mode=(torch.ones(16, 16), torch.ones(16, 16)))):
        with pytest.raises(ValueError):
            L.sourcePolarization(W, **bad)
    for src in (-W, W.to(torch.complex64), W[:16], torch.full((32, 32), float("nan")), "annular"):
        with pytest.raises(ValueError):
            L.sourcePolarization(src, "x")


def test_host_planes_match_the_oracle():
    """The planes vectorSocsKernels(applier=) evaluates on the host for the box and the trace (a CPU pupil)."""
    from lithographysimulator_amd import vector as V
    P = VO.six_points()[0]
    for na, n in VO.OPTICS:
        for rad in (False, True):
            got = V._host_vector_pupils(P[None].expand(3, 32, 32), na, n, rad, np.array([-100.0, 0.0, 100.0]), WL).numpy()
            for p, z in enumerate((-100.0, 0.0, 100.0)):
                want = VO.vector_pupils(P.numpy(), na, n, rad, z, WL)
                assert np.abs(got[p] - want).max() <= 2.0 ** -22 * np.abs(want).max()
                assert not got[p][want == 0].any()
    # cells exactly on alpha^2 + beta^2 = 1 (test_gpu_vector.py, test_vector_pupils_on_the_evanescent_boundary): NA sigma / n is
    # exactly +-1 at the grid edge.  Only these exactly representable cases; a setting that puts cells within 1e-12 of the
    # boundary would test the rounding of a*a + b*b, not the branch.
    for na, n, pn in ((0.72, 1.44, 64), (0.5, 1.0, 32)):
        a, b, gamma, inside = VO.cosines(pn, na, n)
        on = (a * a + b * b) == 1.0
        assert int(on.sum()) == 2 and bool(on[pn // 2, 0]) and bool(on[0, pn // 2]) and not inside[on].any()
        g = torch.Generator().manual_seed(pn)
        R = torch.view_as_complex(torch.randn((pn, pn, 2), generator=g, dtype=torch.float32) + 0.1)
        assert bool((R != 0).all())
        for rad in (False, True):
            got = V._host_vector_pupils(R[None], na, n, rad, None, None).numpy()[0]
            want = VO.vector_pupils(R.numpy(), na, n, rad)
            print(f"NA {na} n {n} pn {pn} radiometric {rad}: 2 cells on the boundary, smallest gamma inside {gamma[inside].min():.3f}")
            assert np.isfinite(got).all() and not got[:, on].any()
            assert (np.abs(got - want) <= 2.0 ** -22 * np.abs(want)).all()
            assert not got[want == 0].any()


def test_direction_maps_reproduce_the_named_mode():
    """A pair of maps through VO.directions: the maps of "te" give what "te" gives, element for element."""
    P, W, M, N = VO.six_points()
    Q = VO.vector_pupils(P.numpy(), *VO.OPTICS[1])
    ex, ey = VO.directions(32, "te")
    for degree in (1.0, 0.5):
        assert np.array_equal(VO.weight_maps(W.numpy(), (ex, ey), degree), VO.weight_maps(W.numpy(), "te", degree))
        assert np.array_equal(VO.explicit_rows(Q, W.numpy(), (ex, ey), degree), VO.explicit_rows(Q, W.numpy(), "te", degree))
    gx, gy = VO.directions(32, VO.twisted_maps(32))
    lit = W.numpy() > 0
    lengths = np.hypot(*VO.twisted_maps(32))
    print(f"twisted maps: lengths {lengths.min():.3f} ... {lengths.max():.3f}, normalised to {np.hypot(gx, gy)[lit].min():.16f} ... "
          f"{np.hypot(gx, gy)[lit].max():.16f} at the lit points")
    assert lengths.min() > 0.5 and lengths.max() < 2.0 and np.abs(np.hypot(gx, gy) - 1.0).max() <= 4e-16
    zx, zy = VO.directions(32, (np.zeros((32, 32)), np.zeros((32, 32))))            # no direction: stays zero, no NaN
    assert not zx.any() and not zy.any()


@pytest.mark.parametrize("mode,degree", MODES + [pytest.param("maps", 0.7, id="maps-0.7")])
@pytest.mark.parametrize("NA_,n", VO.OPTICS)
def test_full_rank_factorisation_on_the_cpu(NA_, n, mode, degree):
    import lithographysimulator_amd as L
    P, W, M, N = VO.six_points()
    label = mode
    if mode == "maps":                                                          # angle 2 phi + 0.3, lengths in (0.5, 2)
        mode = VO.twisted_maps(32)
    Q = VO.vector_pupils(P.numpy(), NA_, n, True)
    maps = VO.weight_maps(W.numpy(), mode, degree)
    rank = VO.rank_of(Q, W.numpy(), mode, degree)
    k = L.vectorSocsKernels(P, W, NA_, polarization=mode, degree=degree, mediumIndex=n, radiometric=True, kernels=rank, oversample=0,
                            applier=VO.apply_as_applier(Q, maps))
    assert isinstance(k, L.SOCSKernels) and k.K == rank and k.lit_points == 6 and tuple(k.kernels.shape) == (rank, 32, 32)
    truth = VO.abbe_truth(Q, M, W.numpy(), mode, degree, N)
    img = SO.kernel_image(k.kernels, M, N)
    e_max, e_l2 = rel_max(img, truth), rel_l2(img, truth)
    tr = VO.trace(Q, maps)
    print(f"NA {NA_} n {n} {label} degree {degree}: rank {rank}, max {e_max:.2e} (bound {TOL_IMAGE_MAX:.0e}), l2 {e_l2:.2e} (bound "
          f"{TOL_IMAGE_L2:.0e}), captured {k.captured:.8f}, trace {k.trace:.6f} (oracle {tr:.6f}), box {k.boxes[0]}")
    assert e_max < TOL_IMAGE_MAX and e_l2 < TOL_IMAGE_L2
    assert abs(k.captured - 1.0) < 1e-5 and abs(k.trace - tr) < 1e-6 * tr and k.weight_sum == float(W.double().sum())
    assert (np.diff(k.eigenvalues.numpy()) <= 0).all()


def test_the_clamp_and_the_argument_errors():
    import lithographysimulator_amd as L
    P, W, M, N = VO.six_points()
    Q = VO.vector_pupils(P.numpy(), 1.35, 1.44)
    for mode, degree, bound in (("te", 1.0, 18), ("unpolarized", 1.0, 30), ("x", 0.5, 30)):
        k = L.vectorSocsKernels(P, W, 1.35, polarization=mode, degree=degree, mediumIndex=1.44, kernels=64, oversample=16,
                                applier=VO.apply_as_applier(Q, VO.weight_maps(W.numpy(), mode, degree)))
        assert k.K == bound, (mode, degree, k.K)
    ap = VO.apply_as_applier(Q, VO.weight_maps(W.numpy(), "x"))
    for kw in (dict(NA=1.5, mediumIndex=1.44), dict(NA=1.0), dict(NA=0.7, defocus=[0.0, 50.0]), dict(NA=0.7, kernels=0),
               dict(NA=0.7, polarization="circular"), dict(NA=0.7, polarization="y", degree=2.0)):
        with pytest.raises(ValueError):
            L.vectorSocsKernels(P, W, applier=ap, **kw)
    with pytest.raises(ValueError):
        L.vectorSocsKernels(P[:30, :30], W[:30, :30], 0.7, applier=ap)             # not a power of two
    with pytest.raises(ValueError):
        L.vectorSocsKernels(torch.stack([P, P]), W, 0.7, defocus=[0.0, 1.0, 2.0], wavelength=WL, applier=[ap, ap, ap])
    with pytest.raises(RuntimeError):
        L.vectorPupils(P, 0.7)                                                     # the kernel runs on a GPU only


def test_vector_abbe_intensity_refuses_per_point_polarisation():
    import lithographysimulator_amd as L
    Q = torch.zeros((6, 32, 32), dtype=torch.complex64)
    M = torch.zeros((32, 32), dtype=torch.complex64)
    sh = torch.zeros((1, 2), dtype=torch.int32)
    e = torch.ones((32, 32))
    for pol in ("te", "tm", (e, e)):
        with pytest.raises(ValueError, match="vectorSocsKernels"):
            L.vectorAbbeIntensity(M, Q, sh, 64, polarization=pol)
    with pytest.raises(ValueError):
        L.vectorAbbeIntensity(M, Q, sh, 64, polarization="x", degree=1.2)
    with pytest.raises(ValueError):
        L.vectorAbbeIntensity(M, Q, sh, 64, polarization="diagonal")


def test_correct_layout_refuses_kernels_of_another_grid():
    import lithographysimulator_amd as L
    import opc_case as C
    k = L.SOCSKernels(torch.zeros((2, 32, 32), dtype=torch.complex64), torch.ones(2, dtype=torch.float64), 1.0, 1.0, 1.0, 2, [None])
    assert C.PN != 32
    kw = dict(spacing=C.SPACING, maxBias=C.MAX_BIAS)
    with pytest.raises(ValueError, match="32 x 32"):
        L.correctLayout(C.layout(), C.PN, C.PIXEL, C.ORIGIN, C.WAVELENGTH, None, None, 0.3, model="socs", socs=k, **kw)
    with pytest.raises(ValueError):
        L.correctLayout(C.layout(), 32, C.PIXEL, C.ORIGIN, C.WAVELENGTH, None, None, 0.3, model="abbe", socs=k, **kw)
    with pytest.raises(TypeError):
        L.correctLayout(C.layout(), C.PN, C.PIXEL, C.ORIGIN, C.WAVELENGTH, None, None, 0.3, model="socs", socs="kernels", **kw)
