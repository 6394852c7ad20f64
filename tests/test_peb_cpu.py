"""The post-exposure bake without a GPU: tests/peb_oracle.py (the float64 restatement that tests/test_gpu_peb.py measures the
kernels against) pinned to closed forms, the host side of the library (litho_peb_min_steps, the workspace size, the argument
errors, which come back as codes before any GPU call) and ChemicallyAmplifiedResist's argument checks."""
import ctypes
import math

import numpy as np
import pytest

import peb_oracle as PO

EPS = 2.0 ** -52
LDS_BUDGET = 0                          # the library's PEB_LDS_BUDGET: measured, the direct kernel wins at every D (LABNOTES)
NO_REACTION = dict(beta=0.0, fl=1.0, half_dt=0.5)


# ---- diffusion -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,axis,k", [((3, 4, 12), -1, 1), ((3, 4, 12), -1, 5), ((3, 12, 4), -2, 3), ((7, 3, 3), -3, 2), ((2, 5, 5), -3, 1),
                                          ((1, 1, 9), -1, 8)])
def test_an_eigenmode_of_the_mirrored_grid_decays_by_its_eigenvalue(shape, axis, k):
    """cos(pi k (i + 1/2) / n) along one axis is an eigenvector of the no-flux second difference with eigenvalue
    -4 sin^2(pi k / 2n): a step multiplies it by exactly 1 - 4 lambda sin^2(pi k / 2n), lambda that axis's."""
    n = shape[axis]
    mode = np.cos(math.pi * k * (np.arange(n) + 0.5) / n)
    idx = [None, None, None]
    idx[axis] = slice(None)
    h0 = np.broadcast_to(mode[tuple(idx)], shape).copy()
    lxy, lz, S = 0.21, 0.07, 9
    lam = lz if axis == -3 else lxy
    factor = 1.0 - 4.0 * lam * math.sin(math.pi * k / (2 * n)) ** 2
    h, q, a = PO.bake(h0, 0.0, S, (lxy, lz), None, **NO_REACTION)
    err = float(np.abs(h - h0 * factor ** S).max())
    print(f"mode k {k} along axis {axis} of {shape}: factor {factor:.6f}, error after {S} steps {err:.1e}")
    assert err <= 16 * S * EPS
    assert np.array_equal(q, np.zeros(shape))                                  # sigma = 0: untouched
    # the quencher takes the same step with its own lambdas
    h2, q2, _ = PO.bake_step(np.zeros(shape), h0, np.zeros(shape), None, (lxy, lz), **NO_REACTION)
    assert np.abs(q2 - h0 * factor).max() <= 16 * EPS and np.array_equal(h2, np.zeros(shape))


def test_mass_is_conserved():
    """No flux through any face: sum h is conserved without reaction, sum (h - q) with neutralisation (R leaves both)."""
    rng = np.random.default_rng(3)
    for shape in ((5, 9, 9), (1, 7, 7), (2, 1, 6), (3, 1, 1)):
        h0 = rng.uniform(0.0, 1.0, shape)
        h, q, _ = PO.bake(h0, 0.0, 12, (0.2, 0.1), (0.05, 0.3), **NO_REACTION)
        drift = abs(h.sum() - h0.sum()) / h0.sum()
        assert drift <= 64 * EPS, (shape, drift)
        for beta in (0.8, 40.0, math.inf):
            h, q, _ = PO.bake(h0, 0.4, 12, (0.2, 0.1), (0.05, 0.3), beta=beta, fl=1.0, half_dt=0.5)
            want = h0.sum() - 0.4 * h0.size
            drift = abs((h - q).sum() - want) / h0.sum()
            print(f"{shape} beta {beta}: sum (h - q) drifts by {drift:.1e} of sum h0")
            assert drift <= 64 * EPS, (shape, beta, drift)


def test_maximum_principle_at_the_minimum_number_of_steps():
    """S = min_steps: every diffusion update is a convex combination, so a non-negative field stays within [0, max]; with
    instantaneous neutralisation on top nothing goes negative."""
    rng = np.random.default_rng(4)
    thickness, D, pixel, sigma_h, sigma_q, vs = 90.0, 6, 10.0, 23.0, 9.0, 0.7
    S = PO.min_steps(sigma_h, sigma_q, vs, thickness, D, pixel)
    lam_h, lam_q = PO.lambdas(sigma_h, vs, pixel, thickness / D, S), PO.lambdas(sigma_q, vs, pixel, thickness / D, S)
    assert 0.9 < 4 * lam_h[0] + 2 * lam_h[1] < 0.999                            # convex with room for the rounding
    h0 = rng.uniform(0.0, 1.0, (D, 11, 11)) * (rng.uniform(size=(D, 11, 11)) < 0.3)      # most cells empty
    top = h0.max()
    h, _, a = PO.bake(h0, 0.0, S, lam_h, lam_q, **NO_REACTION)
    assert h.min() >= 0.0 and h.max() <= top and a.min() >= 0.0
    h, q, a = PO.bake(h0, 0.25, S, lam_h, lam_q, beta=math.inf, fl=0.97, half_dt=0.5)
    print(f"S = {S}: after the bake h in [{h.min():.3g}, {h.max():.3g}], q in [{q.min():.3g}, {q.max():.3g}]")
    assert h.min() >= 0.0 and q.min() >= 0.0 and h.max() <= top and q.max() <= 0.25 and a.min() >= 0.0


# ---- uniform fields, no diffusion ----------------------------------------------------------------------------------------------
def test_instantaneous_neutralisation_takes_the_smaller_species():
    for h0, q0 in ((0.7, 0.3), (0.2, 0.5), (0.4, 0.4), (0.0, 0.3), (0.6, 0.0)):
        h, q, a = PO.bake(np.full((2, 3, 3), h0), q0, 1, None, None, beta=math.inf, fl=1.0, half_dt=0.5)
        assert np.all(h == max(h0 - q0, 0.0)) and np.all(q == max(q0 - h0, 0.0))
        assert np.all(a == 0.5 * (h0 + max(h0 - q0, 0.0)))


def test_acid_loss_alone_is_an_exponential_and_the_trapezoid_bounds_a():
    """h_S = h0 e^(-k t) up to rounding.  a is the composite trapezoid of h(t) = h0 e^(-k t) on S intervals of dt: its error
    is at most t dt^2 / 12 max |h''| = t dt^2 k^2 h0 / 12, and the trapezoid of a convex function overestimates."""
    h0, k, t = 0.8, 0.35, 6.0
    exact = h0 * (1.0 - math.exp(-k * t)) / k
    for S in (4, 8, 16, 64):
        dt = t / S
        h, _, a = PO.bake(np.full((1, 2, 2), h0), 0.0, S, None, None, beta=0.0, fl=math.exp(-k * dt), half_dt=0.5 * dt)
        assert np.abs(h - h0 * math.exp(-k * t)).max() <= 4 * S * EPS
        err = float(a.flat[0] - exact)
        bound = t * dt * dt * k * k * h0 / 12.0
        print(f"S {S}: a - exact = {err:.3e}, bound {bound:.3e}")
        assert 0.0 < err <= bound


def test_finite_neutralisation_converges_to_the_exact_solution_at_first_order():
    """h' = q' = -k h q with u = h0 - q0 conserved: h(t) = u h0 / (h0 - q0 e^(-k u t)).  The step R = beta h q / (1 + beta (h + q))
    is first order in dt: doubling S halves the error, and the ratio of successive errors tends to 1/2 (a second-order scheme
    would give 1/4, an inconsistent one 1).  The oracle, run before the factor was fixed: ratios 0.490 ... 0.499 from S = 32 to
    1024 for both parameter sets (one acid-rich, one quencher-rich); asserted: every ratio within 0.45 ... 0.55."""
    for h0, q0, k, t in ((0.7, 0.3, 2.0, 3.0), (0.25, 0.6, 5.0, 1.5)):
        u = h0 - q0
        exact = u * h0 / (h0 - q0 * math.exp(-k * u * t))
        errs = []
        for S in (32, 64, 128, 256, 512, 1024):
            dt = t / S
            h, q, _ = PO.bake(np.full((1, 1, 1), h0), q0, S, None, None, beta=k * dt, fl=1.0, half_dt=0.5 * dt)
            assert abs((h - q).flat[0] - u) <= 4 * S * EPS
            errs.append(abs(float(h.flat[0]) - exact))
        ratios = [b / a for a, b in zip(errs, errs[1:])]
        print(f"h0 {h0} q0 {q0}: exact {exact:.6f}, errors {['%.2e' % e for e in errs]}, ratios {['%.3f' % r for r in ratios]}")
        assert all(0.45 <= r <= 0.55 for r in ratios)


def test_exposure_and_rate_landmarks():
    h = PO.expose(np.array([[[[0.0, 1.0], [-1.0, np.nan]]]]), [1.0, 2.0], 0.5)
    assert h.shape == (2, 1, 2, 2) and h[0, 0, 0, 0] == 0.0 and h[1, 0, 0, 1] == 1.0 - math.exp(-1.0)
    assert np.isnan(h[:, 0, 1, :]).all()
    m, s = PO.rate(np.array([[[0.0, 2.0, -1.0, np.nan]]]), 1.5, 100.0, 0.1, 5.0, 0.5, 80.0)
    assert m[0, 0, 0] == 1.0 and s[0, 0, 0] == 1.0 / 0.1 and m[0, 0, 1] == math.exp(-3.0)
    assert np.isnan(s[0, 0, 2:]).all() and np.isfinite(s[0, 0, :2]).all()


# ---- the host side of the library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    return _native


def test_new_symbols_are_bound(nat):
    names = nat.exported_symbols()
    for must in ("litho_peb_expose", "litho_peb_min_steps", "litho_peb_work_bytes", "litho_peb_steps_per_launch", "litho_peb_bake",
                 "litho_peb_rate"):
        assert must in names and hasattr(nat.lib(), must)
    import lithographysimulator_amd as L
    for name in ("ChemicallyAmplifiedResist", "BakeResult", "postExposureBake"):
        assert name in L.__all__ and hasattr(L, name)


def test_min_steps_is_the_smallest_stable_number(nat):
    f = nat.lib().litho_peb_min_steps
    cases = [(0.0, 0.0, 1.0, 100.0, 8, 25.0), (10.0, 0.0, 1.0, 100.0, 8, 25.0), (30.0, 5.0, 1.0, 120.0, 8, 25.0), (5.0, 30.0, 1.0, 120.0, 8, 25.0),
             (20.0, 2.0, 1.0, 100.0, 32, 25.0),                                   # hz = 3.125 << pixel: the vertical term decides
             (20.0, 2.0, 0.0, 100.0, 32, 25.0), (20.0, 2.0, 0.3, 100.0, 1, 4.0), (60.0, 10.0, 1.5, 50.0, 17, 2.0), (12.5, 0.0, 0.0, 10.0, 1, 25.0),
             (25.0, 0.0, 0.0, 10.0, 1, 25.0 * math.sqrt(2.0))]
    for sh, sq, vs, thick, D, pixel in cases:
        S = f(sh, sq, vs, thick, D, pixel)
        want = PO.min_steps(sh, sq, vs, thick, D, pixel)
        hz = thick / D
        total = lambda S: max(4 * lxy + 2 * lz for lxy, lz in (PO.lambdas(s, vs, pixel, hz, S) for s in (sh, sq)))   # noqa: E731
        print(f"sigma {sh}/{sq} x{vs}, hz {hz:g}, pixel {pixel:g}: S = {S}, 4 lxy + 2 lz = {total(S):.4f}")
        assert S == want and total(S) <= 1.0 and (S == 1 or total(S - 1) > 1.0)
    assert f(20.0, 2.0, 1.0, 100.0, 32, 25.0) == math.ceil(400.0 * (2 / 625.0 + 1 / 3.125 ** 2))
    assert f(12.5, 0.0, 0.0, 10.0, 1, 25.0) == 1                               # 4 lxy = 0.5
    nan, inf = float("nan"), float("inf")
    for bad in ((-1.0, 0.0, 1.0, 100.0, 8, 25.0), (nan, 0.0, 1.0, 100.0, 8, 25.0), (1.0, inf, 1.0, 100.0, 8, 25.0), (1.0, 1.0, -1.0, 100.0, 8, 25.0),
                (1.0, 1.0, nan, 100.0, 8, 25.0), (1.0, 1.0, 1.0, 0.0, 8, 25.0), (1.0, 1.0, 1.0, inf, 8, 25.0), (1.0, 1.0, 1.0, 100.0, 0, 25.0),
                (1.0, 1.0, 1.0, 100.0, 33, 25.0), (1.0, 1.0, 1.0, 100.0, 8, 0.0), (1.0, 1.0, 1.0, 100.0, 8, nan),
                (1000.0, 0.0, 1.0, 100.0, 8, 1.0)):                              # 2e6 steps: beyond the cap
        assert f(*bad) == 0, bad


def test_work_bytes_and_the_automatic_steps_per_launch(nat):
    f = nat.lib().litho_peb_work_bytes
    assert f(3, 5, 17) == 2 * 4 * 3 * 5 * 17 * 17 and f(1, 1, 1) == 8 and f(1, 32, 16384) == 2 * 4 * 32 * 16384 * 16384
    for bad in ((0, 5, 17), (1, 0, 17), (1, 33, 17), (1, 5, 0), (1, 5, 16385), (2048, 32, 17)):
        assert f(*bad) == 0, bad
    g = nat.lib().litho_peb_steps_per_launch
    assert g(0) == 0 and g(33) == 0
    for D in range(1, 33):                                                     # LDS of the fused kernel: D (4 (16 + 2 s)^2 + 256) floats
        fits = [s for s in (2, 3, 4) if D * (4 * (16 + 2 * s) ** 2 + 256) * 4 <= LDS_BUDGET]
        assert g(D) == (max(fits) if fits else 1), D
    assert g(32) == 1


def test_argument_errors_come_back_before_any_gpu_call(nat):
    """Every refused call returns its code on a machine without a GPU: the checks run before the first HIP call.  The pointers
    are never dereferenced on the host."""
    lib = nat.lib()
    V = 4 * 4 * 64                                                             # bytes of a [1, 4, 8, 8] volume
    p = [ctypes.c_void_p(65536 + 4096 * i) for i in range(6)]
    nan, inf = float("nan"), float("inf")
    E = nat.E_ARG
    g = (ctypes.c_float * 64)(*([1.0] * 64))
    gnan = (ctypes.c_float * 2)(1.0, nan)
    near = lambda base, off: ctypes.c_void_p(base.value + off)                   # noqa: E731
    # litho_peb_expose(image, volumes, D, n, gains, n_gains, C, acid, stream)
    ok = dict(image=p[0], volumes=1, D=4, n=8, gains=g, n_gains=2, C=0.05, acid=p[1])
    for kw in (dict(image=None), dict(acid=None), dict(gains=None), dict(n_gains=0), dict(n_gains=65), dict(gains=gnan), dict(volumes=0), dict(D=0),
               dict(D=33), dict(n=0), dict(n=16385), dict(volumes=16384), dict(volumes=8192, n_gains=2), dict(C=0.0), dict(C=-1.0), dict(C=nan),
               dict(C=inf), dict(acid=near(p[0], V - 4)), dict(acid=near(p[0], -2 * V + 4))):
        assert lib.litho_peb_expose(*{**ok, **kw}.values(), None) == E, kw
    # litho_peb_bake(acid_in, B, D, n, thickness, pixel, q0, k_quench, k_loss, sigma_h, sigma_q, vscale, bake_time, steps, steps_per_launch,
    #                acid, quencher, acid_dose, work, work_bytes, stream)
    ok = dict(acid_in=p[0], B=1, D=4, n=8, thickness=100.0, pixel=25.0, q0=0.1, kq=5.0, kl=0.01, sh=20.0, sq=5.0, vs=1.0, t=60.0, steps=8, spl=0,
              acid=p[1], quencher=p[2], dose=p[3], work=p[4], wb=2 * V)
    least = lib.litho_peb_min_steps(20.0, 5.0, 1.0, 100.0, 4, 25.0)
    assert 1 < least <= 8
    bad = [dict(acid_in=None), dict(acid=None), dict(quencher=None), dict(dose=None), dict(work=None), dict(B=0), dict(D=0), dict(D=33), dict(n=0),
           dict(n=16385), dict(B=16384), dict(thickness=0.0), dict(thickness=nan), dict(thickness=inf), dict(pixel=0.0), dict(pixel=-25.0),
           dict(pixel=nan), dict(q0=-0.1), dict(q0=nan), dict(q0=inf), dict(kq=-1.0), dict(kq=nan), dict(kl=-0.5), dict(kl=nan), dict(kl=inf),
           dict(sh=-1.0), dict(sh=nan), dict(sh=inf), dict(sq=-1.0), dict(sq=nan), dict(vs=-1.0), dict(vs=inf), dict(t=0.0), dict(t=-1.0),
           dict(t=nan), dict(t=inf), dict(steps=least - 1), dict(steps=0), dict(steps=65537), dict(spl=-1), dict(spl=5),
           dict(D=32, spl=2), dict(D=32, spl=4), dict(D=17, spl=4),               # the fused kernel's LDS beyond a workgroup's 160 KiB
           dict(work=near(p[4], 4)),                                            # not 16-byte aligned
           # overlapping buffers: each pair
           dict(acid=p[0]), dict(quencher=p[0]), dict(dose=p[0]), dict(work=p[0]), dict(quencher=p[1]), dict(dose=p[1]), dict(work=p[1]),
           dict(dose=p[2]), dict(work=p[2]), dict(work=p[3]), dict(acid=near(p[0], V - 4)), dict(work=near(p[3], -2 * V + 16)),
           dict(work=near(p[3], V - 16)), dict(dose=near(p[4], 2 * V - 4))]
    for kw in bad:
        assert lib.litho_peb_bake(*{**ok, **kw}.values(), None) == E, kw
    assert lib.litho_peb_bake(*{**ok, "wb": 2 * V - 1}.values(), None) == nat.E_WORKSPACE
    # litho_peb_rate(acid_dose, B, D, n, k_amp, rmax, rmin, q, mth, r0, delta, thickness, slowness, inhibitor, stream)
    ok = dict(a=p[0], B=1, D=4, n=8, kamp=1.0, rmax=100.0, rmin=0.1, q=5.0, mth=0.5, r0=1.0, delta=10.0, thickness=100.0, s=p[1], m=p[2])
    bad = [dict(a=None), dict(s=None), dict(B=0), dict(D=0), dict(D=33), dict(n=0), dict(n=16385), dict(B=16384), dict(kamp=0.0), dict(kamp=-1.0),
           dict(kamp=nan), dict(kamp=inf), dict(rmax=0.0), dict(rmax=nan), dict(rmin=0.0), dict(rmin=inf), dict(q=1.0), dict(q=nan), dict(q=inf),
           dict(mth=-0.01), dict(mth=1.0), dict(mth=nan), dict(r0=0.0), dict(r0=1.01), dict(r0=nan), dict(delta=0.0), dict(delta=nan),
           dict(delta=inf), dict(thickness=0.0), dict(thickness=nan), dict(thickness=inf), dict(s=p[0]), dict(m=p[0]), dict(m=p[1]),
           dict(s=near(p[0], V - 4)), dict(m=near(p[1], 4 - V))]
    for kw in bad:
        assert lib.litho_peb_rate(*{**ok, **kw}.values(), None) == E, kw


# ---- the value class -------------------------------------------------------------------------------------------------------------
def test_the_value_class_refuses_what_the_library_refuses():
    from lithographysimulator_amd import ChemicallyAmplifiedResist, MackResist
    mack = MackResist(C=1.0, rMax=100.0, rMin=0.1, q=5.0, mTh=0.5)
    good = dict(C=0.05, quencher=0.1, kAmp=1.0, kQuench=5.0, kLoss=0.01, acidDiffusionLength=20.0, quencherDiffusionLength=5.0, bakeTime=60.0,
                mack=mack)
    r = ChemicallyAmplifiedResist(**good)
    assert r.verticalScale == 1.0 and r.minSteps(100.0, 4, 25.0) > 1
    ChemicallyAmplifiedResist(**{**good, "kQuench": float("inf"), "quencher": 0.0, "kLoss": 0.0, "acidDiffusionLength": 0.0, "verticalScale": 0.0})
    nan, inf = float("nan"), float("inf")
    for bad in (dict(C=0.0), dict(C=nan), dict(C=inf), dict(quencher=-0.1), dict(quencher=nan), dict(quencher=inf), dict(kAmp=0.0), dict(kAmp=nan),
                dict(kQuench=-1.0), dict(kQuench=nan), dict(kLoss=-1.0), dict(kLoss=inf), dict(acidDiffusionLength=-1.0),
                dict(acidDiffusionLength=inf), dict(quencherDiffusionLength=nan), dict(verticalScale=-0.5), dict(verticalScale=inf),
                dict(bakeTime=0.0), dict(bakeTime=inf), dict(bakeTime=nan),
                dict(mack=MackResist(C=1.0, rMax=100.0, rMin=0.1, q=5.0, mTh=0.5, diffusionLength=5.0)),
                dict(mack=MackResist(C=1.0, rMax=100.0, rMin=0.1, q=5.0, mTh=0.5, verticalDiffusionLength=5.0))):
        with pytest.raises(ValueError):
            ChemicallyAmplifiedResist(**{**good, **bad})
    with pytest.raises(TypeError):
        ChemicallyAmplifiedResist(**{**good, "mack": None})
    with pytest.raises(ValueError):
        ChemicallyAmplifiedResist(**{**good, "acidDiffusionLength": 1000.0}).minSteps(100.0, 8, 1.0)     # beyond the step cap
