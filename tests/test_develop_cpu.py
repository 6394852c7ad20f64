"""Resist development without a GPU: tests/develop_oracle.py (the float64 restatement that tests/test_gpu_develop.py measures the
kernels against) pinned to closed forms, MackResist's argument checks, and the C entry points' argument errors, which come back
as codes before any GPU call."""
import ctypes
import math

import numpy as np
import pytest

import develop_oracle as DO

H, THICK = 25.0, 100.0


# ---- the solver's restatement against closed forms -----------------------------------------------------------------------------
def test_uniform_rate_is_depth_over_rate():
    """s constant: the front is a plane, T_d = z_d / r exactly (one-axis updates only)."""
    for D, n, r in ((1, 1, 3.0), (5, 7, 0.5), (17, 4, 40.0)):
        T, it = DO.arrival_time(np.full((D, n, n), 1.0 / r), THICK, H)
        want = DO.depths(THICK, D)[:, None, None] / r * np.ones((D, n, n))
        err = float(np.abs(T - want).max() / want.max())
        print(f"uniform D {D} n {n}: {it} iterations, relative error {err:.1e}")
        assert err <= 4 * 2.0 ** -52 * D


def test_rate_depending_on_depth_only_accumulates_plane_by_plane():
    """T_0 = hz / (2 r_0), T_d = T_{d-1} + hz / r_d in every column."""
    r = np.array([1.0, 3.0, 0.5, 2.0, 7.0])
    D, n = len(r), 9
    hz = THICK / D
    T, it = DO.arrival_time(np.broadcast_to((1.0 / r)[:, None, None], (D, n, n)).copy(), THICK, H)
    want = np.cumsum(np.concatenate([[0.5 * hz / r[0]], hz / r[1:]]))
    err = float(np.abs(T - want[:, None, None]).max() / want.max())
    print(f"z-only rate: {it} iterations, relative error {err:.1e}")
    assert err <= 4 * 2.0 ** -52 * D
    # a slow plane above a fast one is not overtaken from the side: the columns are identical
    assert float(np.ptp(T, axis=(1, 2)).max()) == 0.0


def slot_volume(n, col, r_fast, r_slow):
    """Two planes: a wall top plane opened over column `col` (a slot along y), below it the slot in slow surroundings."""
    s = np.full((2, n, n), np.nan)
    s[0, :, col] = 1.0 / r_fast
    s[1] = 1.0 / r_slow
    s[1, :, col] = 1.0 / r_fast
    return s


def test_slot_feeds_its_surroundings_along_the_grid_axis():
    """Under the wall plane the only way into plane 1 is the slot: T = T_slot + distance / r_slow along x, T_slot = 1.5 hz / r_fast."""
    n, col, r_fast, r_slow = 12, 3, 50.0, 0.25
    T, it = DO.arrival_time(slot_volume(n, col, r_fast, r_slow), THICK, H)
    hz = THICK / 2
    t_slot = 1.5 * hz / r_fast
    want = t_slot + np.abs(np.arange(n) - col) * H / r_slow
    err = float(np.abs(T[1] - want[None, :]).max() / want.max())
    print(f"slot: {it} iterations, relative error {err:.1e}")
    assert err <= 1e-13
    assert np.isinf(T[0][:, np.arange(n) != col]).all() and np.allclose(T[0][:, col], 0.5 * hz / r_fast, rtol=1e-15)


def test_walls_keep_infinity_and_shadow_what_they_enclose():
    D, n = 3, 9
    s = np.full((D, n, n), 0.1)
    s[:, 2, 2:7] = s[:, 6, 2:7] = s[:, 2:7, 2] = s[:, 2:7, 6] = np.nan          # the side walls of a box through the depth
    s[0, 2:7, 2:7] = np.nan                                                    # and its lid; the bottom is the layer's
    T, _ = DO.arrival_time(s, THICK, H)
    assert np.isinf(T[:, 2:7, 2:7]).all()                                      # walls and the enclosed cells alike
    outside = np.ones((n, n), dtype=bool)
    outside[2:7, 2:7] = False
    assert np.isfinite(T[:, outside]).all()
    assert np.allclose(T[:, 0, 0], DO.depths(THICK, D) * 0.1)


def test_fixed_point_and_serpentine_iteration_count():
    rng = np.random.default_rng(1)
    s = 10.0 ** rng.uniform(-3, 0, (5, 17, 17))
    T, it = DO.arrival_time(s, THICK, H)
    res = float(np.abs(DO.godunov(T, s, H, THICK / 5) - T).max() / T.max())
    print(f"random 17^2 x 5: {it} iterations, |G(T) - T| / max T = {res:.1e}")
    assert res <= 1e-15
    n = 16
    sp = np.full((2, n, n), np.nan)
    sp[0, 0, 0] = 0.01
    sp[1] = DO.serpentine(n, 0.01, 2.0)
    T, it = DO.arrival_time(sp, 50.0, H)
    print(f"serpentine {n}^2: {it} iterations")
    assert it > n * n // 2 - n                                                 # the front walks the channel cell by cell
    assert np.isfinite(T[1]).all() and int(np.isfinite(T[0]).sum()) == 1
    # along the channel's first row the front is one-dimensional
    assert np.allclose(T[1, 0, :], 1.5 * 25.0 * 0.01 + np.arange(n) * H * 0.01, rtol=1e-12)


# ---- the rate --------------------------------------------------------------------------------------------------------------------
def test_mack_rate_at_its_three_landmarks():
    """m = 1 (unexposed): r_min; m = 0: r_max + r_min; m = m_th: r_max (a + 1)(q - 1) / (2 q) + r_min, the inflection."""
    from lithographysimulator_amd import MackResist
    for r_max, r_min, q, m_th in ((100.0, 0.1, 5.0, 0.5), (30.0, 0.01, 2.5, 0.1), (250.0, 1.0, 12.0, 0.9), (80.0, 0.5, 1.5, 0.0)):
        a = DO.mack_a(q, m_th)
        assert a == (q + 1.0) / (q - 1.0) * (1.0 - m_th) ** q
        assert DO.rate_of_m(1.0, r_max, r_min, q, m_th) == r_min
        assert abs(DO.rate_of_m(0.0, r_max, r_min, q, m_th) - (r_max + r_min)) <= 1e-14 * r_max
        want = r_max * (a + 1.0) * (q - 1.0) / (2.0 * q) + r_min
        assert abs(DO.rate_of_m(m_th, r_max, r_min, q, m_th) - want) <= 1e-14 * r_max
        model = MackResist(0.05, r_max, r_min, q, m_th)
        m = np.linspace(0.0, 1.0, 11)
        assert np.array_equal(model.rate(m), DO.rate_of_m(m, r_max, r_min, q, m_th))
        assert (np.diff(model.rate(m)) < 0).all()                             # more inhibitor, slower
    # the slowness volume: gain-major, exposure through exp(-C g I), the surface factor by plane
    I = np.array([[[0.0, 0.5], [1.0, 2.0]]] * 2)
    s = DO.slowness(I, [1.0, 2.0], 0.05, 100.0, 0.1, 5.0, 0.5, THICK, r0=0.2, delta=30.0)
    assert s.shape == (2, 2, 2, 2)
    f = 1.0 - 0.8 * np.exp(-np.array([25.0, 75.0]) / 30.0)
    assert np.allclose(s[0, :, 0, 0], 1.0 / (0.1 * f), rtol=1e-15)
    assert np.allclose(s[1, 0, 1, 0], 1.0 / (DO.rate_of_m(math.exp(-0.1), 100.0, 0.1, 5.0, 0.5) * f[0]), rtol=1e-15)


def test_mack_resist_refuses_what_the_library_refuses():
    from lithographysimulator_amd import MackResist
    good = dict(C=0.05, rMax=100.0, rMin=0.1, q=5.0, mTh=0.5)
    MackResist(**good)
    MackResist(**good, surfaceRate=0.3, surfaceDepth=20.0, diffusionLength=10.0, verticalDiffusionLength=5.0)
    nan = float("nan")
    for bad in (dict(C=0.0), dict(C=nan), dict(rMax=-1.0), dict(rMin=0.0), dict(q=1.0), dict(q=nan), dict(mTh=1.0), dict(mTh=-0.1),
                dict(surfaceRate=0.0), dict(surfaceRate=1.1), dict(surfaceRate=0.5), dict(surfaceDepth=0.0), dict(surfaceDepth=nan),
                dict(diffusionLength=-1.0), dict(verticalDiffusionLength=float("inf"))):
        with pytest.raises(ValueError):
            MackResist(**{**good, **bad})


# ---- the diffusion ---------------------------------------------------------------------------------------------------------------
def test_mirror_index_and_conserved_column_sum():
    assert [DO.mirror_index(i, 3) for i in range(-7, 10)] == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2]
    assert [DO.mirror_index(i, 1) for i in (-3, -1, 0, 1, 4)] == [0] * 5
    rng = np.random.default_rng(2)
    for D, sigma in ((1, 2.0), (2, 3.0), (5, 0.7), (5, 8.0), (17, 1.3)):       # R up to 32 > D: the mirror folds more than once
        V = rng.uniform(0.0, 2.0, (D, 6, 6))
        out = DO.diffuse(V, 0.0, sigma)
        drift = float(np.abs(out.sum(axis=0) - V.sum(axis=0)).max() / V.sum(axis=0).max())
        print(f"z mirror D {D} sigma {sigma} cells: column sums drift by {drift:.1e}")
        assert drift <= (2 * math.ceil(4 * sigma) + 2) * 2.0 ** -24                # the fp32 rounding of the normalised taps
        if D == 1:
            assert np.allclose(out, V, rtol=1e-6)
    assert np.array_equal(DO.diffuse(V, 0.0, 0.0), V)
    # laterally the volume is open: diffusion loses what leaves the grid, plane by plane as the 2-D model does
    import resist_oracle as RO
    assert np.array_equal(DO.diffuse(V, 1.5, 0.0), RO.diffuse(V, 1.5))


# ---- the developed depth ---------------------------------------------------------------------------------------------------------
def test_developed_depth_cases():
    D = 4
    hz = THICK / D
    T = np.zeros((D, 1, 5))
    T[:, 0, 0] = [1.0, 2.0, 3.0, 4.0]            # cleared at t = 5
    T[:, 0, 1] = [10.0, 20.0, 30.0, 40.0]        # not even the first plane
    T[:, 0, 2] = [1.0, 2.0, 8.0, 9.0]            # between planes 1 and 2
    T[:, 0, 3] = [1.0, 7.0, 3.0, 4.0]            # an undercut: the FIRST crossing counts
    T[:, 0, 4] = [1.0, 2.0, np.inf, np.inf]      # stops at a wall
    z = DO.developed_depth(T, THICK, 5.0)[0]
    want = [THICK, 0.5 * hz * 5.0 / 10.0, 1.5 * hz + hz * (5.0 - 2.0) / (8.0 - 2.0), 0.5 * hz + hz * (5.0 - 1.0) / (7.0 - 1.0), 1.5 * hz]
    assert np.allclose(z, want, rtol=1e-15), (z, want)


# ---- the C boundary --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    return _native


def test_new_symbols_are_bound_and_the_error_code_raises(nat):
    names = nat.exported_symbols()
    for must in ("litho_latent_diffuse", "litho_develop_rate", "litho_develop_time", "litho_develop_work_bytes", "litho_developed_depth"):
        assert must in names and hasattr(nat.lib(), must)
    assert nat.E_NOCONV == -6
    with pytest.raises(RuntimeError, match="fixed point"):
        nat.check(nat.E_NOCONV, "litho_develop_time")
    import lithographysimulator_amd as L
    for name in ("MackResist", "developmentRate", "developmentTime", "developedDepth", "resistProfile", "latentDiffusion"):
        assert name in L.__all__ and hasattr(L, name)


def test_work_bytes(nat):
    f = nat.lib().litho_develop_work_bytes
    assert f(3, 5, 17, 1024) == 4096 + 4 * 3 * 5 * 17 * 17
    assert f(1, 1, 1, 1) == 256 + 4
    assert f(1, 32, 16384, 65536) == 4 * 65536 + 4 * 32 * 16384 * 16384
    for bad in ((0, 5, 17, 10), (1, 0, 17, 10), (1, 33, 17, 10), (1, 5, 0, 10), (1, 5, 16385, 10), (1, 5, 17, 0), (1, 5, 17, 65537),
                (2048, 32, 17, 10)):
        assert f(*bad) == 0, bad


def test_argument_errors_come_back_before_any_gpu_call(nat):
    """Every refused call returns LITHO_E_ARG on a machine without a GPU: the checks run before the first HIP call.  The
    pointers are never dereferenced on the host."""
    lib = nat.lib()
    p, q, w = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(16384)
    nan, inf = float("nan"), float("inf")
    E = nat.E_ARG
    # litho_latent_diffuse(image, B, D, n, sigma_xy, sigma_z, out, work, work_bytes, stream)
    diffuse = lib.litho_latent_diffuse
    for args in ((None, 1, 4, 8, 1.0, 1.0, q, w, 1 << 20), (p, 1, 4, 8, 1.0, 1.0, None, w, 1 << 20), (p, 1, 4, 8, 1.0, 1.0, p, w, 1 << 20),
                 (p, 0, 4, 8, 1.0, 1.0, q, w, 1 << 20), (p, 1, 0, 8, 1.0, 1.0, q, w, 1 << 20), (p, 1, 33, 8, 1.0, 1.0, q, w, 1 << 20),
                 (p, 1, 4, 0, 1.0, 1.0, q, w, 1 << 20), (p, 1, 4, 16385, 1.0, 1.0, q, w, 1 << 20), (p, 16384, 4, 8, 1.0, 1.0, q, w, 1 << 20),
                 (p, 1, 4, 8, -1.0, 1.0, q, w, 1 << 20), (p, 1, 4, 8, 8.01, 1.0, q, w, 1 << 20), (p, 1, 4, 8, nan, 1.0, q, w, 1 << 20),
                 (p, 1, 4, 8, 1.0, -0.5, q, w, 1 << 20), (p, 1, 4, 8, 1.0, 8.01, q, w, 1 << 20), (p, 1, 4, 8, 1.0, inf, q, w, 1 << 20),
                 (p, 1, 4, 8, 1.0, 1.0, q, None, 0), (p, 1, 4, 8, 1.0, 0.0, q, None, 0)):
        assert diffuse(*args, None) == E, args
    assert diffuse(p, 1, 4, 8, 1.0, 1.0, q, w, 4 * 4 * 64 - 1, None) == nat.E_WORKSPACE
    # buffers that overlap (a volume here is 1024 bytes): a pass would read what it writes
    near = lambda base, off: ctypes.c_void_p(base.value + off)                   # noqa: E731
    for args in ((p, 1, 4, 8, 1.0, 1.0, near(p, 1020), w, 1 << 20), (p, 1, 4, 8, 1.0, 1.0, near(p, -512), w, 1 << 20),
                 (p, 1, 4, 8, 1.0, 1.0, q, p, 1 << 20), (p, 1, 4, 8, 1.0, 1.0, q, q, 1 << 20), (p, 1, 4, 8, 1.0, 1.0, q, near(q, 512), 1 << 20),
                 (p, 1, 4, 8, 1.0, 0.0, q, near(p, -1020), 1 << 20), (p, 1, 4, 8, 0.0, 1.0, near(p, 4), None, 0)):
        assert diffuse(*args, None) == E, args
    # litho_develop_rate(image, volumes, D, n, gains, n_gains, C, rmax, rmin, q, mth, r0, delta, thickness, out, stream)
    rate = lib.litho_develop_rate
    g = (ctypes.c_float * 64)(*([1.0] * 64))
    gnan = (ctypes.c_float * 2)(1.0, nan)
    ok = dict(image=p, volumes=1, D=4, n=8, gains=g, n_gains=2, C=0.05, rmax=100.0, rmin=0.1, q=5.0, mth=0.5, r0=1.0, delta=10.0,
              thickness=100.0, out=q)
    bad = [dict(image=None), dict(out=None), dict(gains=None), dict(n_gains=0), dict(n_gains=65), dict(gains=gnan), dict(volumes=0),
           dict(D=0), dict(D=33), dict(n=0), dict(n=16385), dict(volumes=16384), dict(volumes=8192, n_gains=2),
           dict(C=0.0), dict(C=-1.0), dict(C=nan), dict(C=inf), dict(rmax=0.0), dict(rmax=nan), dict(rmin=0.0), dict(rmin=-0.1), dict(rmin=inf),
           dict(q=1.0), dict(q=0.5), dict(q=nan), dict(q=inf), dict(mth=-0.01), dict(mth=1.0), dict(mth=nan),
           dict(r0=0.0), dict(r0=1.01), dict(r0=nan), dict(delta=0.0), dict(delta=-3.0), dict(delta=nan), dict(delta=inf),
           dict(thickness=0.0), dict(thickness=nan), dict(thickness=inf)]
    for kw in bad:
        a = {**ok, **kw}
        assert rate(*a.values(), None) == E, kw
    # litho_develop_time(slowness, B, D, n, thickness, pixel, max_iterations, T, work, work_bytes, launches_host, stream)
    time = lib.litho_develop_time
    launches = ctypes.c_int(-7)
    ok = dict(s=p, B=1, D=4, n=8, thickness=100.0, pixel=25.0, it=16, T=q, work=w, wb=1 << 20)
    bad = [dict(s=None), dict(T=None), dict(work=None), dict(T=p), dict(B=0), dict(D=0), dict(D=33), dict(n=0), dict(n=16385),
           dict(B=16384), dict(thickness=0.0), dict(thickness=nan), dict(thickness=inf), dict(pixel=0.0), dict(pixel=-25.0),
           dict(pixel=nan), dict(it=0), dict(it=65537), dict(work=ctypes.c_void_p(16388)), dict(thickness=1e-30), dict(pixel=1e30)]
    for kw in bad:
        a = {**ok, **kw}
        assert time(*a.values(), ctypes.byref(launches), None) == E, kw
        assert launches.value == 0
    assert time(*ok.values(), None, None) == E
    # the workspace holds the flag words and the second T buffer (256 + 1024 bytes here): it may overlap neither T nor the slowness
    for kw in (dict(work=q), dict(work=p), dict(work=ctypes.c_void_p(q.value - 1264)), dict(work=ctypes.c_void_p(p.value + 1008)),
               dict(T=ctypes.c_void_p(p.value + 1020)), dict(T=ctypes.c_void_p(w.value + 1276))):
        a = {**ok, **kw}
        assert time(*a.values(), ctypes.byref(launches), None) == E, kw
    assert time(*{**ok, "wb": 256 + 4 * 4 * 64 - 1}.values(), ctypes.byref(launches), None) == nat.E_WORKSPACE
    # litho_developed_depth(T, B, D, n, thickness, t, depth, stream)
    depth = lib.litho_developed_depth
    for args in ((None, 1, 4, 8, 100.0, 5.0, q), (p, 1, 4, 8, 100.0, 5.0, None), (p, 0, 4, 8, 100.0, 5.0, q), (p, 1, 0, 8, 100.0, 5.0, q),
                 (p, 1, 33, 8, 100.0, 5.0, q), (p, 1, 4, 0, 100.0, 5.0, q), (p, 1, 4, 16385, 100.0, 5.0, q), (p, 16384, 4, 8, 100.0, 5.0, q),
                 (p, 1, 4, 8, 0.0, 5.0, q), (p, 1, 4, 8, nan, 5.0, q), (p, 1, 4, 8, inf, 5.0, q), (p, 1, 4, 8, 100.0, -1.0, q),
                 (p, 1, 4, 8, 100.0, nan, q), (p, 1, 4, 8, 100.0, inf, q)):
        assert depth(*args, None) == E, args
