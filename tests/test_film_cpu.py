"""The resist film stack without a GPU: tests/film_oracle.py (both formulations) and the host path of
lithographysimulator_amd/film.py pinned by closed forms, FilmStack / filmPupils argument errors, and the bulk factorisation of
vectorSocsKernels(film=, depths=, depthWeights=) through `applier=` with the float64 host operator.

Tolerances: the closed forms and the two formulations against each other 1e-12 of the largest magnitude (double precision; the
phases reach a few hundred radians, so their rounding is a few 1e-14); the host planes, which are rounded to complex64,
2^-22 |want| + 1e-12 max |want| per element, the bound of tests/test_gpu_film.py; the factorisation helpers.TOL_IMAGE_MAX of
the operator's largest entry, what the CPU SOCS tests ask of an image.  Every test prints what it observed (-s)."""
import numpy as np
import pytest
import torch

import film_oracle as FO
import socs_oracle as SO
import vector_oracle as VO
from helpers import TOL_IMAGE_MAX

WL = FO.WL
TOL = 1e-12
METHODS = ("matrix", "stable")


def _close(tag, got, want, tol=TOL):
    scale = float(np.abs(want).max())
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max()) / scale
    print(f"{tag}: {err:.2e} of the largest magnitude (bound {tol:.0e})")
    assert np.isfinite(np.asarray(got)).all() and err <= tol, (tag, err)


def _random_pupil(pn, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.view_as_complex(torch.randn((pn, pn, 2), generator=g, dtype=torch.float32) + 0.1)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("NA_,n0", VO.OPTICS)
def test_homogeneous_stack_is_the_defocused_vector_pupil(NA_, n0, method):
    """Every index equal to n0, k = 0: the planes equal vector_pupils(defocus = z) . exp(-2 pi i n0 z / lambda), z measured from
    the top of the stack (50 nm of first layer + the depth in the second)."""
    P = _random_pupil(32, 3).numpy()
    layers, depths = [(n0, 0.0, 50.0), (n0, 0.0, 80.0), (n0, 0.0, 20.0)], [0.0, 25.0, 80.0]
    for rad in (False, True):
        got = FO.film_pupils(P, NA_, n0, layers, (n0, 0.0), 1, depths, WL, rad, None, method)
        for i, z in enumerate(depths):
            want = VO.vector_pupils(P, NA_, n0, rad, 50.0 + z, WL) * np.exp(-2j * np.pi * n0 * (50.0 + z) / WL)
            _close(f"{method} NA {NA_} radiometric {rad} z {z}", got[i], want)
    both = FO.film_pupils(P, NA_, n0, layers, (n0, 0.0), 1, [25.0], WL, True, -40.0, method)[0]
    want = VO.vector_pupils(P, NA_, n0, True, 75.0 - 40.0, WL) * np.exp(-2j * np.pi * n0 * 75.0 / WL)
    _close(f"{method} NA {NA_} with the pupil's own defocus riding on top", both, want)


@pytest.mark.parametrize("method", METHODS)
def test_one_interface_at_the_centre_cell(method):
    """A layer of the substrate's own index: one interface.  At s = 0, E_s = E_rad = t exp(-2 pi i nn z / lambda) with
    t = 2 n0 / (n0 + nn), E_z = 0, and the planes are P t on the diagonal and 0 elsewhere."""
    n0, nn = FO.WATER, complex(1.7, -0.05)
    layers, sub = [(1.7, 0.05, 90.0)], (1.7, 0.05)
    depths = np.array([0.0, 30.0, 90.0])
    Es, Erad, Ez = FO.film_fields(n0, layers, sub, 0, np.zeros(1), WL, depths, method)
    want = 2.0 * n0 / (n0 + nn) * np.exp(-2j * np.pi * nn * depths / WL)
    _close(f"{method} E_s", Es[:, 0], want)
    _close(f"{method} E_rad", Erad[:, 0], want)
    assert not Ez.any()
    pn = 16
    P = _random_pupil(pn, 4).numpy()
    Q = FO.film_pupils(P, 1.35, n0, layers, sub, 0, depths, WL, method=method)[:, :, pn // 2, pn // 2]
    _close(f"{method} planes at the centre cell", Q, np.outer(want, [1, 0, 0, 1, 0, 0]) * P[pn // 2, pn // 2])
    assert not Q[:, [1, 2, 4, 5]].any()


@pytest.mark.parametrize("method", METHODS)
def test_quarter_wave_layer_removes_the_standing_wave(method):
    """An index-matched resist over n = sqrt(n0 n_s), d = lambda / (4 n), on a lossless substrate: no reflection at normal
    incidence, |E_s(z)| constant; without the layer it is not."""
    n0, ns = FO.WATER, 2.6
    n1 = np.sqrt(n0 * ns)
    depths = np.linspace(0.0, 150.0, 31)
    Es, _, _ = FO.film_fields(n0, [(n0, 0.0, 150.0), (n1, 0.0, WL / (4.0 * n1))], (ns, 0.0), 0, np.zeros(1), WL, depths, method)
    mod = np.abs(Es[:, 0])
    _close(f"{method} |E_s(z)| with the quarter-wave layer", mod, np.full_like(mod, 1.0))
    bare, _, _ = FO.film_fields(n0, [(n0, 0.0, 150.0)], (ns, 0.0), 0, np.zeros(1), WL, depths, method)
    swing = np.abs(bare[:, 0]).max() / np.abs(bare[:, 0]).min()
    print(f"{method}: without the layer |E_s| swings by a factor {swing:.3f}")
    assert swing > 1.5


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pol", ["s", "p"])
def test_flux_is_conserved_in_a_lossless_stack(pol, method):
    """Re(u conj(v)) is the same at every depth of the sampled layer and in the substrate, and equals what the incident medium
    sends in minus what comes back, for s from normal incidence up to NA^2 -- with a frustrated layer (n < NA) on the way."""
    n0 = FO.WATER
    layers = [(1.56, 0.0, 40.0), (1.72, 0.0, 110.0), (1.30, 0.0, 25.0), (1.9, 0.0, 33.0)]
    s = np.linspace(0.0, 1.35 ** 2, 57)
    depths = np.linspace(0.0, 110.0, 12)
    u, v, us, vs = FO.SOLVERS[method](pol, n0, layers, (2.4, 0.0), 1, s, WL, depths)
    flux = (u * v.conj()).real
    sub = (us * vs.conj()).real
    _close(f"{method} {pol}: flux at 12 depths against the substrate's", flux, np.broadcast_to(sub, flux.shape))
    # the incident side: eta0 a0^2 (1 - |r|^2) with r from the field at the top of the stack
    ut, vt, _, _ = FO.SOLVERS[method](pol, n0, layers, (2.4, 0.0), 0, s, WL, [0.0])
    _close(f"{method} {pol}: flux at the top of the stack", (ut[0] * vt[0].conj()).real, sub)
    assert (sub > 0).all()


@pytest.mark.parametrize("method", METHODS)
def test_absorption_decays_with_depth(method):
    """An absorbing resist on a substrate of its own index at normal incidence: |E|^2 = |t|^2 exp(-4 pi k z / lambda).  A wrong
    sign of k would grow."""
    n, k = 1.7, 0.08
    depths = np.linspace(0.0, 400.0, 9)
    Es, _, _ = FO.film_fields(FO.WATER, [(n, k, 400.0)], (n, k), 0, np.zeros(1), WL, depths, method)
    t2 = abs(2.0 * FO.WATER / (FO.WATER + complex(n, -k))) ** 2
    _close(f"{method} |E_s|^2", np.abs(Es[:, 0]) ** 2, t2 * np.exp(-4.0 * np.pi * k * depths / WL))


@pytest.mark.parametrize("method", METHODS)
def test_standing_wave_period(method):
    """A lossless resist on silicon: |E_s(z)|^2 repeats after lambda / (2 Re w) and is in antiphase half a period on."""
    n0, n = FO.WATER, 1.7
    s = np.array([0.0, 0.9 ** 2, 1.3 ** 2])
    period = WL / (2.0 * np.sqrt(n * n - s))
    for i in range(3):
        z = np.array([5.0, 5.0 + period[i], 5.0 + 2 * period[i], 5.0 + 0.5 * period[i]])
        Es, _, _ = FO.film_fields(n0, [(n, 0.0, 200.0)], FO.SILICON, 0, s[i:i + 1], WL, z, method)
        I = np.abs(Es[:, 0]) ** 2
        _close(f"{method} s {s[i]:.2f}: |E_s|^2 one and two periods ({period[i]:.2f} nm) on", I[1:3], np.full(2, I[0]))
        assert abs(I[3] - I[0]) > 0.05 * I[0]


def test_frustrated_and_thick_absorbing_layers_stay_finite():
    """A layer with n < NA (evanescent in it beyond s = n^2) and 5,000 nm of k = 0.5 under the resist: cos of the complex phase
    reaches e^81, which double holds, so the matrix form is still exact to rounding and the two formulations agree; 50,000 nm
    overflow it (e^814), and the bottom-referenced form stays finite."""
    P = _random_pupil(32, 5).numpy()
    layers = [(1.30, 0.0, 30.0), (1.7, 0.02, 100.0), (1.8, 0.5, 5000.0)]
    depths = [0.0, 40.0, 100.0]
    a = FO.film_pupils(P, 1.35, FO.WATER, layers, FO.SILICON, 1, depths, WL, True, 20.0, "matrix")
    b = FO.film_pupils(P, 1.35, FO.WATER, layers, FO.SILICON, 1, depths, WL, True, 20.0, "stable")
    _close("frustrated top coat, 5,000 nm of k = 0.5: matrix against stable", a, b)
    assert np.abs(b).max() > 0.1
    layers[2] = (1.8, 0.5, 50000.0)
    c = FO.film_pupils(P, 1.35, FO.WATER, layers, FO.SILICON, 1, depths, WL, True, 20.0, "stable")
    _close("50,000 nm: stable against 5,000 nm (nothing comes back from either)", c, b)
    with np.errstate(all="ignore"):
        assert not np.isfinite(FO.film_pupils(P, 1.35, FO.WATER, layers, FO.SILICON, 1, depths, WL, True, 20.0, "matrix")).all()


def _host_planes(P, NA_, n0, rad, zs, stack, depths):
    from lithographysimulator_amd import film as F
    layers, sub, res = stack
    return F._host_film_pupils(P, NA_, n0, rad, zs, WL, F.FilmStack(layers, sub, res), np.asarray(depths, dtype=np.float64)).numpy()


@pytest.mark.parametrize("name", ["L1", "L3", "L16"])
def test_host_planes_match_the_oracle(name):
    """film._host_film_pupils (float64 torch, rounded to complex64 once) against the oracle at pn 32, the optics of
    vector_oracle.OPTICS, with and without gamma^(-1/2), three defocus values."""
    stack = FO.STACKS[name] if name in FO.STACKS else FO.stack16(8)
    layers, sub, res = stack
    depths = [0.0, 0.37 * layers[res][2], layers[res][2]]
    P = _random_pupil(32, 6)
    zs = np.array([-100.0, 0.0, 100.0])
    worst = 0.0
    for NA_, n0 in VO.OPTICS:
        for rad in (False, True):
            got = _host_planes(P[None].expand(3, 32, 32), NA_, n0, rad, zs, stack, depths).astype(np.complex128)
            for i, z in enumerate(zs):
                want = FO.film_pupils(P.numpy(), NA_, n0, layers, sub, res, depths, WL, rad, z)
                excess = np.abs(got[i] - want) - 2.0 ** -22 * np.abs(want) - 1e-12 * np.abs(want).max()
                worst = max(worst, float((np.abs(got[i] - want)[want != 0] / np.abs(want)[want != 0]).max()))
                assert (excess <= 0).all() and not got[i][want == 0].any() and (want == 0).any()
    print(f"{name}: worst relative error of the host planes {worst:.2e}")


def test_film_stack_and_film_pupils_argument_errors():
    import lithographysimulator_amd as L
    ok = [(1.7, 0.02, 100.0)]
    for layers, sub, res in (([], FO.SILICON, 0), ([(1.7, 0.02)], FO.SILICON, 0), ([(1.7, -0.1, 100.0)], FO.SILICON, 0),
                             ([(0.0, 0.0, 100.0)], FO.SILICON, 0), ([(1.7, 0.0, 0.0)], FO.SILICON, 0),
                             ([(1.7, 0.0, float("nan"))], FO.SILICON, 0), (ok, (0.88,), 0), (ok, (0.88, -1.0), 0),
                             (ok, (float("inf"), 0.0), 0), (ok, FO.SILICON, 1), (ok, FO.SILICON, -1), (ok, FO.SILICON, 0.5),
                             (ok * 17, FO.SILICON, 0), ("abc", FO.SILICON, 0)):
        with pytest.raises(ValueError):
            L.FilmStack(layers, sub, res)
    stack = L.FilmStack(FO.STACKS["L3"][0], FO.STACKS["L3"][1], FO.STACKS["L3"][2])
    assert stack.thickness == 100.0 and stack.depths(4) == [12.5, 37.5, 62.5, 87.5] and stack.depths(1) == [50.0]
    with pytest.raises(ValueError):
        stack.depths(0)
    P = _random_pupil(16, 7)
    for kw in (dict(depths=[-1.0]), dict(depths=[100.5]), dict(depths=[]), dict(depths=[float("nan")]), dict(wavelength=0.0),
               dict(wavelength=None), dict(NA=1.5), dict(depths=[[1.0]]), dict(defocus=[0.0, 1.0], pupilF=torch.stack([P, P, P]))):
        args = dict(pupilF=P, NA=1.35, stack=stack, depths=[10.0], wavelength=WL, mediumIndex=FO.WATER)
        args.update(kw)
        with pytest.raises(ValueError):
            L.filmPupils(**args)
    with pytest.raises(TypeError):
        L.filmPupils(P, 1.35, FO.STACKS["L3"], [10.0], WL, FO.WATER)                # plain data is not a FilmStack
    with pytest.raises(RuntimeError):
        L.filmPupils(P, 1.35, stack, [10.0], WL, FO.WATER)                          # the kernel runs on a GPU only
    W = torch.zeros((16, 16))
    W[8, 8] = 1.0
    ap = lambda X: X                                                                # noqa: E731 -- never reached
    for kw in (dict(depths=[10.0]), dict(depthWeights=[1.0]), dict(film=stack), dict(film=stack, depths=[10.0], wavelength=None),
               dict(film=stack, depths=[10.0, 20.0], depthWeights=[1.0]), dict(film=stack, depths=[10.0, 20.0], depthWeights=[0.0, 0.0]),
               dict(film=stack, depths=[10.0, 20.0], depthWeights=[1.0, -1.0]), dict(film=stack, depths=[10.0, 200.0])):
        args = dict(wavelength=WL, mediumIndex=FO.WATER, applier=ap)
        args.update(kw)
        with pytest.raises(ValueError):
            L.vectorSocsKernels(P, W, 1.35, **args)


def _bulk_case():
    """pn 16, three lit points with grey weights, the L3 stack at two depths, pure "x"."""
    pn = 16
    P = _random_pupil(pn, 8) * torch.from_numpy(VO.cosines(pn, 1.35, FO.WATER)[3])
    W = torch.zeros((pn, pn), dtype=torch.float64)
    W[8, 8], W[8, 10], W[6, 7] = 1.0, 0.6, 1.4
    layers, sub, res = FO.STACKS["L3"]
    depths, omega = [20.0, 75.0], [0.3, 0.7]
    Q = FO.film_pupils(P.numpy(), 1.35, FO.WATER, layers, sub, res, depths, WL, True, 15.0)
    return P, W, (layers, sub, res), depths, omega, Q


def test_bulk_factorisation_through_the_applier():
    """sum_k phi_k phi_k^H = sum_d w_d T_d at K = rank, the operator applied in float64 on the host; `trace` is the weighted sum
    of the per-depth traces; without weights every depth is a plane of its own."""
    import lithographysimulator_amd as L
    P, W, (layers, sub, res), depths, omega, Q = _bulk_case()
    maps = VO.weight_maps(W.numpy(), "x")
    rows = [VO.explicit_rows(Qd, W.numpy(), "x") for Qd in Q]
    T = sum(o * SO.tcc(A) for o, A in zip(omega, rows))
    rank = int(np.linalg.matrix_rank(np.concatenate([np.sqrt(o) * A for o, A in zip(omega, rows)])))
    assert 9 < rank <= 3 * 3 * 2                                                  # more than one depth's 3 S

    def bulk(X):
        x = X.detach().cpu().numpy()
        return torch.from_numpy(sum(o * VO.fft_apply(Qd, maps, x) for o, Qd in zip(omega, Q))).to(torch.complex64)

    stack = L.FilmStack(layers, sub, res)
    k = L.vectorSocsKernels(P, W, 1.35, polarization="x", mediumIndex=FO.WATER, radiometric=True, defocus=15.0, wavelength=WL,
                            kernels=rank, oversample=0, applier=bulk, film=stack, depths=depths, depthWeights=omega)
    assert isinstance(k, L.SOCSKernels) and not k.stacked and k.K == rank and tuple(k.kernels.shape) == (rank, 16, 16)
    phi = k.kernels.numpy().astype(np.complex128).reshape(rank, -1)
    err = float(np.abs(np.einsum("kf,kg->fg", phi, phi.conj()) - T).max() / np.abs(T).max())
    tr = sum(o * VO.trace(Qd, maps) for o, Qd in zip(omega, Q))
    print(f"bulk D 2 S 3 x: rank {rank}, sum phi phi^H against sum w_d T_d {err:.2e} (bound {TOL_IMAGE_MAX:.0e}), trace {k.trace:.8f} "
          f"(oracle {tr:.8f}), captured {k.captured:.8f}")
    assert err < TOL_IMAGE_MAX
    assert abs(k.trace - tr) <= 1e-6 * tr and abs(k.captured - 1.0) < 1e-5
    # the clamp: J = min(kernels + oversample, 3 S D)
    big = L.vectorSocsKernels(P, W, 1.35, polarization="x", mediumIndex=FO.WATER, radiometric=True, defocus=15.0, wavelength=WL,
                              kernels=64, applier=bulk, film=stack, depths=depths, depthWeights=omega)
    assert big.K == 18
    # without weights: planes f D + d, each its own operator
    per = [VO.apply_as_applier(Qd, maps) for Qd in Q]
    k2 = L.vectorSocsKernels(P, W, 1.35, polarization="x", mediumIndex=FO.WATER, radiometric=True, defocus=15.0, wavelength=WL,
                             kernels=9, oversample=0, applier=per, film=stack, depths=depths)
    assert k2.stacked and k2.planes == 2 and tuple(k2.kernels.shape) == (2, 9, 16, 16)
    for d in range(2):
        phi = k2.kernels[d].numpy().astype(np.complex128).reshape(9, -1)
        Td = SO.tcc(rows[d])
        e = float(np.abs(np.einsum("kf,kg->fg", phi, phi.conj()) - Td).max() / np.abs(Td).max())
        print(f"  depth {d}: sum phi phi^H against T_d {e:.2e}, trace {float(k2.trace[d]):.8f}")
        assert e < TOL_IMAGE_MAX and abs(float(k2.trace[d]) - VO.trace(Q[d], maps)) <= 1e-6 * float(k2.trace[d])
    assert abs(k.trace - sum(o * float(t) for o, t in zip(omega, k2.trace))) <= 1e-12 * k.trace
