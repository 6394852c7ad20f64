"""Resist development on the GPU (csrc/develop.hip): litho_latent_diffuse, litho_develop_rate, litho_develop_time and
litho_developed_depth through lithographysimulator_amd/develop.py, against the float64 restatement tests/develop_oracle.py (pinned
to closed forms in test_develop_cpu.py).

Bounds.
  rate       |got - want| <= 2^-22 |want|: one fp32 rounding of a double result, one more for a last-place difference of the
             device's exp / pow (the film test's bound).
  diffusion  the resist diffusion test's: every pass is a (2R+1)-term fp32 sum of non-negative products, 2R+2 roundings, plus 2
             for the fp32 taps and margin, each at most 2^-24 of the largest value: sum over the passes that run of
             (2R + 4) 2^-24 max D  (two lateral passes: (2 (2R+2) + 4), that test's bound).
  solver     max |T - T_f64| <= C_SOLVER (D + 2n) 2^-24 max T: a handful of roundings per update along the longest possible
             chain of cells.  Measured on an MI355X over the 25 random (n, D) cases: 0.016 ... 0.070 of (D + 2n) 2^-24 (the
             worst at n 15, D 5; serpentine 0.011, closed box 0.035, depth-only closed form 0.030); C_SOLVER = 0.3, about four
             times the worst.
  residual   the device's T through the oracle's G in float64: |G(T) - T| <= C_RESIDUAL 2^-24 T per cell: the update is about a
             dozen fp32 operations on quantities no larger than T.  Measured: 2.5 ... 3.7; C_RESIDUAL = 16, about four times the
             worst.  (With the discriminant in its literal form Bq^2 - A Cq the residual was 33 at D = 32, where hz = h / 8; the
             kernel evaluates the non-cancelling form, include/litho_abbe.h.)
  depth      |z - z_f64| <= 2^-22 (thickness + hz (|t| + |T_a| + |T_b|) / |T_b - T_a|): one fp32 interpolation, the division's
             condition as in the CD test; on the random, the constructed and the slot volumes (whole columns of +inf in plane 0).
  CD         end to end: the CD test's tolerance (tests/test_gpu_resist.py) plus 2 dT_bound / (ils t), with dT_bound the bound
             asserted on max |T - T_f64| in the same test -- that tolerance alone compares ONE image through two implementations.
Shapes: n = 15, 16, 17 (tile edge -1, 0, +1), 24 (partial tiles), 48 (three tiles), 1; D = 1, 2 (the top half-step and the
missing lower neighbour in one cell), 5, 17, 32 (more than 64 KiB of LDS).  Every test prints what it observed (-s)."""
import numpy as np
import pytest
import torch

import develop_oracle as DO
import resist_oracle as RO

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_SOLVER, C_RESIDUAL = 0.3, 16.0
H, THICK = 25.0, 100.0
SIZES = [(n, D) for n in (15, 16, 17, 24, 48) for D in (1, 2, 5, 17, 32)]


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


def same_bits(a, b):
    """Equal as bit patterns (int32 views): a NaN-bearing result compares like any other, and -0 is not +0."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def solver_bound(n, D, t_max):
    return C_SOLVER * (D + 2 * n) * U * t_max


_random = {}


def random_case(L, dev, n, D):
    """B = 3 different volumes of rates log-uniform over three decades: (slowness fp32 on the host, device T, launches, oracle T)."""
    if (n, D) not in _random:
        rng = np.random.default_rng(1000 * n + D)
        s = (10.0 ** rng.uniform(-3.0, 0.0, (3, D, n, n))).astype(np.float32)
        T, launches = L.developmentTime(torch.from_numpy(s).to(dev), THICK, H, returnLaunches=True)
        want, its = DO.arrival_time(s.astype(np.float64), THICK, H)
        _random[(n, D)] = (s, T, launches, want, its)
    return _random[(n, D)]


# ---- rate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(1, 1), (15, 2), (16, 5), (17, 17), (24, 32), (48, 5)])
def test_rate_against_the_oracle(L, dev, n, D):
    rng = np.random.default_rng(n + D)
    I = rng.uniform(0.0, 3.0, (2, D, n, n)).astype(np.float32)
    I.flat[0] = 0.0                                                            # unexposed: exactly r_min
    doses = (0.6, 1.0, 1.7)
    gains = [float(np.float32(d)) for d in doses]
    for r0, delta in ((1.0, None), (0.25, 30.0)):
        resist = L.MackResist(C=0.9, rMax=120.0, rMin=0.05, q=5.0, mTh=0.4, surfaceRate=r0, surfaceDepth=delta)
        got = L.developmentRate(torch.from_numpy(I).to(dev), resist, THICK, H, doses)
        assert got.dtype == torch.float32 and tuple(got.shape) == (6, D, n, n)
        want = DO.slowness(I, gains, 0.9, 120.0, 0.05, 5.0, 0.4, THICK, r0, delta if delta else 1.0)
        g = got.cpu().numpy().astype(np.float64)
        rel = float((np.abs(g - want) / want).max())
        print(f"rate n {n} D {D} surface {r0}: worst relative error {rel:.2e} (bound {2.0 ** -22:.2e}); s in [{want.min():.3g}, {want.max():.3g}]")
        assert rel <= 2.0 ** -22
        if r0 == 1.0:
            assert g.flat[0] == float(np.float32(1.0 / 0.05))
            one = L.developmentRate(torch.from_numpy(I[1]).to(dev), resist, THICK, H, doses[2:])     # [D,n,n] in, one dose
            assert torch.equal(one[0], got[5])


@pytest.mark.parametrize("q", [4.0, 5.0, 4.5])
def test_negative_or_nan_exposure_is_a_wall(L, dev, q):
    """(1 - m)^q is finite under a negative exposure for an integer q (even: like an exposed cell; odd: below r_min or negative):
    the kernel writes NaN itself, on the 16-byte path (n = 16) and the scalar one (n = 15), and the solver leaves +inf there."""
    for n in (15, 16):
        I = np.full((2, n, n), 0.7, dtype=np.float32)
        I[0, 1, 2], I[1, 3, 3], I[1, n - 1, n - 1], I[0, 0, 0] = -0.5, np.nan, -1e-30, 0.0
        resist = L.MackResist(C=0.9, rMax=120.0, rMin=0.05, q=q, mTh=0.4)
        s = L.developmentRate(torch.from_numpy(I).to(dev), resist, THICK, H, (1.0, -2.0))
        g = s.cpu().numpy()
        assert np.isnan(g[0, 0, 1, 2]) and np.isnan(g[0, 1, 3, 3])
        assert g[0, 1, n - 1, n - 1] == g[0, 0, 0, 0] == np.float32(1.0 / 0.05)  # exp(+0.9e-30) = 1 exactly: unexposed, not negative
        assert int(np.isnan(g[0]).sum()) == 2
        assert np.isnan(g[1]).sum() == g[1].size - 3                              # a negative dose: NaN wherever I > 0; I = -0.5 develops
        want = DO.slowness(I[None], [1.0, -2.0], 0.9, 120.0, 0.05, q, 0.4, THICK)
        assert np.array_equal(np.isnan(g), np.isnan(want))
        T = L.developmentTime(s[0], THICK, H).cpu().numpy()
        assert np.isinf(T[0, 1, 2]) and np.isinf(T[1, 3, 3]) and int(np.isinf(T).sum()) == 2


# ---- diffusion -------------------------------------------------------------------------------------------------------------------
def diffusion_bound(Rxy, Rz):
    return ((2 * (2 * Rxy + 4) if Rxy else 0) + ((2 * Rz + 4) if Rz else 0)) * U


@pytest.mark.parametrize("n,D", [(1, 1), (17, 2), (24, 5), (48, 17), (15, 32)])
def test_diffusion_against_the_oracle(L, dev, n, D):
    """Lateral R = 0, 2, 5, 12, 32 (the regimes of the 2-D diffusion test) against vertical R = 0, 2, 12, 32: with D <= 5 the
    mirror folds more than once."""
    rng = np.random.default_rng(7 * n + D)
    V = rng.uniform(0.0, 4.0, (2, D, n, n)).astype(np.float32)
    Vd = torch.from_numpy(V).to(dev)
    hz = THICK / D
    worst = 0.0
    for sxy_nm in (0.0, 0.45 * H, 1.2 * H, 2.9 * H, 7.9 * H):
        for sz_nm in (0.0, 0.45 * hz, 2.9 * hz, 7.9 * hz):
            sxy, sz = sxy_nm / H, sz_nm / hz                                   # in cells, as the library forms them
            Rxy, Rz = RO.radius(sxy), RO.radius(sz)
            assert Rxy in (0, 2, 5, 12, 32) and Rz in (0, 2, 12, 32)
            got = L.latentDiffusion(Vd, THICK, H, sxy_nm, sz_nm)
            if Rxy == 0 and Rz == 0:
                assert torch.equal(got, Vd)
                continue
            want = DO.diffuse(V.astype(np.float64), sxy, sz)
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
            bound = diffusion_bound(Rxy, Rz) * float(want.max())
            worst = max(worst, err / bound)
            assert err <= bound, (n, D, Rxy, Rz, err, err / bound)
            if Rxy == 0:                                                       # the mirror keeps what is in the layer
                drift = float((got.double().sum(dim=1) - Vd.double().sum(dim=1)).abs().max() / Vd.double().sum(dim=1).max())
                assert drift <= (2 * Rz + 2) * U * 2
    print(f"diffusion n {n} D {D}: worst error {worst:.3f} of its bound over 19 (R_xy, R_z) pairs")
    one = L.latentDiffusion(Vd[1], THICK, H, 30.0, 0.5 * hz)                       # a [D,n,n] volume equals its slice of the batch
    assert torch.equal(one, L.latentDiffusion(Vd, THICK, H, 30.0, 0.5 * hz)[1])


# ---- the solver: closed forms ----------------------------------------------------------------------------------------------------
def test_uniform_and_depth_only_rates(L, dev):
    n, D = 17, 5
    hz = THICK / D
    r = 0.8
    T, launches = L.developmentTime(torch.full((D, n, n), 1.0 / r, dtype=torch.float32, device=dev), THICK, H, returnLaunches=True)
    want = DO.depths(THICK, D)[:, None, None] / r * np.ones((D, n, n))
    err = float(np.abs(T.cpu().numpy() - want).max())
    print(f"uniform rate: {launches} launches, max error {err:.2e} = {err / solver_bound(n, D, want.max()):.3f} of the bound")
    assert err <= solver_bound(n, D, want.max())
    rates = np.array([1.0, 3.0, 0.5, 2.0, 7.0])
    s = torch.from_numpy(np.broadcast_to((1.0 / rates)[:, None, None], (D, n, n)).astype(np.float32).copy()).to(dev)
    T, launches = L.developmentTime(s, THICK, H, returnLaunches=True)
    s64 = s[:, 0, 0].cpu().numpy().astype(np.float64)
    want = np.cumsum(np.concatenate([[0.5 * hz * s64[0]], hz * s64[1:]]))
    err = float(np.abs(T.cpu().numpy() - want[:, None, None]).max())
    print(f"depth-only rate: {launches} launches, max error {err:.2e} = {err / solver_bound(n, D, want.max()):.3f} of the bound")
    assert err <= solver_bound(n, D, want.max())
    assert float((T.amax(dim=(1, 2)) - T.amin(dim=(1, 2))).max()) == 0.0          # every column the same bits


# ---- the solver: random rates, residual, determinism -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", SIZES)
def test_random_rates_against_the_oracle(L, dev, n, D):
    s, T, launches, want, its = random_case(L, dev, n, D)
    got = T.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = float(np.abs(got - want).max() / want.max())
    unit = (D + 2 * n) * U
    print(f"random n {n} D {D}: {launches} launches (oracle {its} Jacobi sweeps), max |dT| / max T = {err:.2e} = {err / unit:.3f} (D + 2n) 2^-24")
    assert err <= C_SOLVER * unit
    # a fixed point of the float64 update, to a few fp32 units in the last place of T
    G = DO.godunov(got, s.astype(np.float64), H, THICK / D)
    res = float((np.abs(G - got) / got).max() / U)
    print(f"   residual max |G(T) - T| / T = {res:.2f} x 2^-24")
    assert res <= C_RESIDUAL


@pytest.mark.parametrize("n,D", [(17, 5), (48, 2), (24, 32)])
def test_second_call_and_batch_are_bit_identical(L, dev, n, D):
    s, T, launches, _, _ = random_case(L, dev, n, D)
    sd = torch.from_numpy(s).to(dev)
    again, l2 = L.developmentTime(sd, THICK, H, returnLaunches=True)
    assert same_bits(again, T) and l2 == launches
    singles = [L.developmentTime(sd[b], THICK, H, returnLaunches=True) for b in range(3)]
    assert all(same_bits(t, T[b]) for b, (t, _) in enumerate(singles))
    assert max(l for _, l in singles) == launches                               # the batch runs until its slowest volume is done
    print(f"n {n} D {D}: second call and 3 single calls equal the batch bit for bit; launches {launches} vs {[l for _, l in singles]}")


# ---- slot, serpentine, walls -----------------------------------------------------------------------------------------------------
SLOT = dict(n=48, col=3, r_fast=50.0, r_slow=0.25)


def _slot_volume():
    """A wall top plane opened over column 3 (a slot along y); below it the slot in slow surroundings."""
    n, col = SLOT["n"], SLOT["col"]
    s = np.full((2, n, n), np.nan, dtype=np.float32)
    s[0, :, col] = 1.0 / SLOT["r_fast"]
    s[1] = 1.0 / SLOT["r_slow"]
    s[1, :, col] = 1.0 / SLOT["r_fast"]
    return s


def test_slot_front_crosses_three_tiles(L, dev):
    """Under the wall plane the only way into plane 1 is the slot: T = T_slot + |col - 3| h / r_slow."""
    n, col = SLOT["n"], SLOT["col"]
    s = _slot_volume()
    T, launches = L.developmentTime(torch.from_numpy(s).to(dev), THICK, H, returnLaunches=True)
    got = T.cpu().numpy().astype(np.float64)
    s64 = s.astype(np.float64)
    closed = 1.5 * (THICK / 2) * s64[0, 0, col] + np.abs(np.arange(n) - col) * H * s64[1, 0, 0]
    want, _ = DO.arrival_time(s64, THICK, H)
    e1, e2 = float(np.abs(got[1] - closed[None]).max()), float(np.abs(got[1] - want[1]).max())
    b = solver_bound(n, 2, closed.max())
    print(f"slot: {launches} launches; max error {e1:.2e} from the closed form, {e2:.2e} from the oracle; bound {b:.2e}")
    assert e1 <= b and e2 <= b and launches > 3
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.isinf(got[0][:, np.arange(n) != col]).all()


def _serpentine(n):
    s = np.full((2, n, n), np.nan, dtype=np.float32)
    s[0, 0, 0] = 0.01
    s[1] = DO.serpentine(n, 0.01, 2.0).astype(np.float32)
    return s


def test_serpentine_converges_late_and_the_launch_cap_raises(L, dev):
    n = 48
    s = _serpentine(n)
    sd = torch.from_numpy(s).to(dev)
    T, launches = L.developmentTime(sd, 50.0, H, returnLaunches=True)
    want, its = DO.arrival_time(s.astype(np.float64), 50.0, H)
    got = T.cpu().numpy().astype(np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and int(fin[0].sum()) == 1 and fin[1].all()
    err = float(np.abs(got[fin] - want[fin]).max() / want[fin].max())
    unit = (2 + 2 * n) * U
    print(f"serpentine: {launches} launches (oracle {its} sweeps), max |dT| / max T = {err:.2e} = {err / unit:.3f} (D + 2n) 2^-24")
    assert launches > 3                                                        # more launches than tiles across
    assert err <= C_SOLVER * unit
    with pytest.raises(RuntimeError, match="fixed point"):
        L.developmentTime(sd, 50.0, H, maxIterations=2)
    torch.cuda.synchronize()
    T2, l2 = L.developmentTime(sd, 50.0, H, maxIterations=launches, returnLaunches=True)    # exactly enough, and nothing is left behind
    assert torch.equal(T2, T) and l2 == launches
    if launches > 1:
        with pytest.raises(RuntimeError, match="fixed point"):
            L.developmentTime(sd, 50.0, H, maxIterations=launches - 1)


def test_closed_box_of_walls(L, dev):
    n, D = 24, 5
    rng = np.random.default_rng(5)
    s = (10.0 ** rng.uniform(-2.0, 0.0, (D, n, n))).astype(np.float32)
    lo, hi = 6, 19                                                             # the box straddles the tile seam at 16
    s[:, lo, lo:hi + 1] = s[:, hi, lo:hi + 1] = s[:, lo:hi + 1, lo] = s[:, lo:hi + 1, hi] = np.nan
    s[0, lo:hi + 1, lo:hi + 1] = np.nan
    s[2, 0, 0], s[3, 1, 1], s[1, 2, 2] = 0.0, -1.0, np.inf                     # not finite and positive: walls as well
    T, launches = L.developmentTime(torch.from_numpy(s).to(dev), THICK, H, returnLaunches=True)
    got = T.cpu().numpy().astype(np.float64)
    want, _ = DO.arrival_time(s.astype(np.float64), THICK, H)
    assert np.isinf(got[:, lo:hi + 1, lo:hi + 1]).all() and np.array_equal(np.isinf(got), np.isinf(want))
    assert not np.isnan(got).any() and np.isinf(got[2, 0, 0]) and np.isinf(got[3, 1, 1]) and np.isinf(got[1, 2, 2])
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max() / want[fin].max())
    print(f"closed box: {launches} launches, {int((~fin).sum())} cells at +inf, max |dT| / max T outside = {err:.2e}")
    assert err <= C_SOLVER * (D + 2 * n) * U


# ---- developed depth -------------------------------------------------------------------------------------------------------------
def _depth_check(tag, L, T, thickness, t):
    t = float(np.float32(t))
    got = L.developedDepth(T, thickness, t).cpu().numpy().astype(np.float64)
    T64 = T.cpu().numpy().astype(np.float64)
    want = DO.developed_depth(T64, thickness, t)
    D = T64.shape[-3]
    hz = thickness / D
    # the condition of the crossing's division: d = the first plane that is not developed
    und = ~(T64 <= t)
    first = np.where(und.any(axis=-3), und.argmax(axis=-3), D)
    idx = np.clip(first, 1, D - 1)
    Tb = np.take_along_axis(T64, np.expand_dims(idx, -3), axis=-3).squeeze(-3)
    Ta = np.take_along_axis(T64, np.expand_dims(idx - 1, -3), axis=-3).squeeze(-3) if D > 1 else Tb
    with np.errstate(invalid="ignore", divide="ignore"):
        cond = np.where((first >= 1) & (first < D) & np.isfinite(Tb), (abs(t) + np.abs(Ta) + np.abs(Tb)) / np.abs(Tb - Ta), 0.0)
    tol = 2.0 ** -22 * (thickness + hz * cond)
    worst = float((np.abs(got - want) / tol).max())
    kinds = (int((first == D).sum()), int((first == 0).sum()), int(((first > 0) & (first < D)).sum()))
    print(f"depth {tag}: cleared / above plane 0 / between planes = {kinds}; worst error {worst:.3f} of its bound")
    assert worst <= 1.0
    assert (got[first == D] == float(np.float32(thickness))).all()
    return kinds


def test_developed_depth(L, dev):
    seen = np.zeros(3, dtype=np.int64)
    for n, D in ((17, 5), (48, 2), (24, 32), (16, 1)):
        _, T, _, want, _ = random_case(L, dev, n, D)
        for frac in (0.05, 0.4, 1.1):
            seen += _depth_check(f"random n {n} D {D} t {frac} max T", L, T, THICK, frac * float(want.max()))
    assert (seen > 10).all()                                                   # every branch was exercised
    # constructed columns: cleared, not even plane 0, between planes, an undercut (the FIRST crossing), a wall below
    D, n = 4, 5
    T = np.zeros((D, n, n), dtype=np.float32)
    T[:, :, 0] = np.array([1.0, 2.0, 3.0, 4.0])[:, None]
    T[:, :, 1] = np.array([10.0, 20.0, 30.0, 40.0])[:, None]
    T[:, :, 2] = np.array([1.0, 2.0, 8.0, 9.0])[:, None]
    T[:, :, 3] = np.array([1.0, 7.0, 3.0, 4.0])[:, None]
    T[:, :, 4] = np.array([1.0, 2.0, np.inf, np.inf])[:, None]
    hz = THICK / D
    z = L.developedDepth(torch.from_numpy(T).to(dev), THICK, 5.0).cpu().numpy()
    want = np.array([THICK, 0.5 * hz * 5.0 / 10.0, 1.5 * hz + hz * 3.0 / 6.0, 0.5 * hz + hz * 4.0 / 6.0, 1.5 * hz])
    print("constructed columns:", z[0].tolist(), "want", want.tolist())
    assert np.allclose(z, want[None, :], rtol=2.0 ** -22, atol=0.0)
    _depth_check("constructed", L, torch.from_numpy(T).to(dev), THICK, 5.0)
    # the slot volume: plane 0 is +inf in whole columns (0.5 hz (t / inf) = 0 there, whatever lies below), the slot has
    # T_0 = 0.5 s and T_1 = 1.5 s: a crossing between the planes at t = 1 s, cleared at t = 2 s and later
    n, col = SLOT["n"], SLOT["col"]
    Ts = L.developmentTime(torch.from_numpy(_slot_volume()).to(dev), THICK, H)
    under = np.arange(n) != col
    for t_dev, in_slot in ((1.0, 0.5 * THICK), (2.0, THICK), (150.0, THICK)):
        kinds = _depth_check(f"slot t {t_dev} s", L, Ts, THICK, t_dev)
        z = L.developedDepth(Ts, THICK, t_dev).cpu().numpy()
        assert (z[:, under] == 0.0).all()                                      # nothing is developed under the wall plane
        assert np.allclose(z[:, col], in_slot, rtol=2.0 ** -20, atol=0.0) and kinds[1] == n * (n - 1)
        print(f"   slot t {t_dev} s: z* = {float(z[0, col])} nm in the slot, 0 under the wall plane ({kinds[1]} columns)")


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_resist_profile_end_to_end(L, dev):
    """pn 64, the film test's three-layer stack at four depths, a small kernel set: resistProfile equals the chain of the single
    calls bit for bit, and its CDs are those of the oracle's T within the CD test's tolerance plus what the asserted bound on
    max |dT| moves an edge (the existing tolerance alone compares one image through two implementations; here the images differ)."""
    import film_oracle as FO
    import socs_oracle as SO
    from helpers import DEMO_AB, NA, PS, f16
    from lithographysimulator_amd.synthetic import lines_mask
    from oracle import abbe_oracle as O
    pn, Dp, WL = 64, 4, FO.WL
    W = SO.strided_points(O.source_annular(0.3, 0.9, pn), 5).to(torch.float32)
    layers, sub, res = FO.STACKS["L3"]
    stack = L.FilmStack(layers, sub, res)
    P = O.pupil_function(f16(DEMO_AB), pn, NA, WL).to(torch.complex64).to(dev)
    M = O.mask_spectrum(lines_mask(pn), PS, WL).to(torch.complex64).to(dev)
    N = O.calculate_epsilon_n(4 / pn, PS, WL)[1]
    k = L.vectorSocsKernels(P, W.to(dev), 1.35, polarization="x", mediumIndex=FO.WATER, radiometric=True, wavelength=WL, kernels=8,
                            oversample=0, film=stack, depths=stack.depths(Dp))
    image = L.hopkinsIntensity(M, k, N)
    assert tuple(image.shape) == (Dp, pn, pn)
    image = (image / image.max()).contiguous()
    resist = L.MackResist(C=2.0, rMax=100.0, rMin=0.05, q=4.0, mTh=0.5, surfaceRate=0.5, surfaceDepth=20.0, diffusionLength=15.0,
                          verticalDiffusionLength=12.0)
    doses, t_dev = (0.8, 1.2), 20.0
    prof = L.resistProfile(image, resist, stack, PS, t_dev, doses=doses)
    assert tuple(prof.T.shape) == (2, 1, Dp, pn, pn) and tuple(prof.depth.shape) == (2, 1, pn, pn) and prof.launches >= 2
    s = L.developmentRate(image, resist, stack.thickness, PS, doses)
    T = L.developmentTime(s, stack.thickness, PS)
    assert torch.equal(prof.T.reshape(2, Dp, pn, pn), T)
    assert torch.equal(prof.depth.reshape(2, pn, pn), L.developedDepth(T, stack.thickness, t_dev))
    # the float64 chain from the device's image
    hz = stack.thickness / Dp
    lat = DO.diffuse(image.cpu().numpy().astype(np.float64)[None], 15.0 / PS, 12.0 / hz)
    s64 = DO.slowness(lat, [float(np.float32(d)) for d in doses], 2.0, 100.0, 0.05, 4.0, 0.5, stack.thickness, 0.5, 20.0)
    T64, its = DO.arrival_time(s64, stack.thickness, PS)
    got = prof.T.reshape(2, Dp, pn, pn).cpu().numpy().astype(np.float64)
    dT = float(np.abs(got - T64).max())
    print(f"end to end: {prof.launches} launches (oracle {its} sweeps), T in [{T64.min():.3g}, {T64.max():.3g}] s, max |dT| = {dT:.2e}")
    row = pn // 2
    line = got[0, 0, row]
    cols = [int(c) for c in np.nonzero(line < t_dev)[0]]
    assert cols and len(cols) < pn, "the development time must cut the profile"
    c = cols[len(cols) // 2]
    gauges = [(row, c, 0), (row + 3, c, 0), (row, c, 1), (row, int(np.argmax(line)), 0)]
    cd = prof.cd(gauges)
    assert tuple(cd.shape) == (2, Dp, len(gauges), 5)
    ref_T = np.where(np.isinf(T64), 2.0 * t_dev + 1.0, T64).astype(np.float32)
    ref = L.measureCD(torch.from_numpy(ref_T).reshape(2 * Dp, pn, pn).to(dev), t_dev, gauges, PS,
                      exposed=False).reshape(2, Dp, len(gauges), 5).cpu().numpy().astype(np.float64)
    g = cd.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(ref)) and np.array_equal(g[..., 0] == 0.0, ref[..., 0] == 0.0)
    # max |dT| is within the solver bound plus what its input carries: the rate's 2^-22 and the diffused image's bound times
    # |d ln s / d ln I| <= q (d ln r / d ln x <= 1, d ln x / d ln (1 - m) = q, d ln (1 - m) / d ln I = E / (e^E - 1) <= 1)
    feed = 2.0 ** -22 + resist.q * diffusion_bound(RO.radius(15.0 / PS), RO.radius(12.0 / hz))
    dT_bound = (C_SOLVER * (Dp + 2 * pn) * U + feed) * float(T64.max())
    print(f"   max |dT| / max T = {dT / T64.max():.2e}; bound {dT_bound / T64.max():.2e}")
    assert dT <= dT_bound
    # CDs: the CD test's tolerance (tests/test_gpu_resist.py: fp32 positions with the crossing's division condition, the fp32
    # difference and product) holds for ONE image through two implementations.  Here the two images themselves differ, by at most
    # dT_bound, and an edge moves by dT / |dT/dx| = dT / (ils t) nm, two edges per CD: that term is added, with the ASSERTED bound.
    _, _, conds = RO.measure_cd(ref_T.reshape(2 * Dp, pn, pn), gauges, [1.0], t_dev, False, PS)
    pos_tol = 2.0 ** -22 * (pn + conds.reshape(2, Dp, len(gauges), 2))
    ils = np.fmin(ref[..., 3], ref[..., 4])
    fin = np.isfinite(ils) & (ref[..., 0] > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        tol = (pos_tol.sum(-1) + 2.0 ** -22 * pn) * PS + 2.0 * dT_bound / (ils * t_dev)
    worst = float((np.abs(g[..., 0] - ref[..., 0])[fin] / tol[fin]).max())
    print(f"   CDs at {int(fin.sum())} (dose, depth, gauge) entries: worst |dCD| = {float(np.abs(g[..., 0] - ref[..., 0])[fin].max()):.2e} nm "
          f"= {worst:.3f} of its tolerance (largest {float(tol[fin].max()):.2e} nm); CD per depth at dose {doses[0]}: {g[0, :, 0, 0].tolist()}")
    assert int(fin.sum()) >= Dp and worst <= 1.0
    angle = prof.sidewallAngle(gauges[0])
    assert angle.shape == (2, 1, 2) and np.isfinite(angle).any()
    polys = prof.contours(0)
    assert len(polys) == 2 and len(polys[0]) == 1 and len(polys[0][0].polygons) >= 1
    print(f"   side-wall angles {angle[:, 0].tolist()} deg; {len(polys[0][0].polygons)} contour(s) at the top plane")
