"""The float64 restatement of the forward mode of the resist chain (tests/resist_tangent_oracle.py) pinned without a GPU:
  1. to central differences of the forward oracles (peb_oracle.bake / expose, develop_oracle.slowness / arrival_time);
  2. to the adjoint oracles by <g, J v> = <J^T g, v>, 1e-12 relative to the sum of the absolute terms;
  3. the library's two host chains (litho_peb_param_tangent, litho_develop_rate_param_tangent) against their transposes and the
     oracle, and every argument error of every new entry point, returned before any launch.
Every test prints what it observed (-s)."""
import ctypes
import math

import numpy as np
import pytest

import develop_grad_oracle as DGO
import develop_oracle as DO
import peb_grad_oracle as GO
import peb_oracle as PO
import resist_param_oracle as RP
import resist_tangent_oracle as TO
from test_resist_param_cpu import BAKE, H, RESISTS, SHAPES, STEP_SETS, THICK, clear_seed, perturbed, volumes

FD_BOUND = 1e-6            # central differences with e = 1e-6: truncation e^2 and cancellation 2^-53 / e leave ~1e-9
DUAL_BOUND = 1e-12
MACK = dict(r_max=120.0, r_min=0.05, q=5.0, m_th=0.4)


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    return _native


def directions(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, shape), float(rng.uniform(-1.0, 1.0)), rng.uniform(-1.0, 1.0, 6) * np.array([0.01, 0.01, 0.01, 0.01, 1.0, 0.05])


# ---- 1. central differences --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", SHAPES)
def test_the_bake_tangent_against_central_differences(n, D):
    """Each kind of direction alone -- dh0, dq0 and the six step slots -- against (bake(+e) - bake(-e)) / 2e, per output."""
    S, q0, worst = 5, 0.3, 0.0
    for si, base in enumerate(STEP_SETS):
        P = dict(base, half_dt=0.5 * BAKE / S)
        instant = math.isinf(P["beta"])
        e = 1e-8 if instant else 1e-6
        h0 = volumes(n, D, clear_seed(n, D, S, P, q0) if instant else 0)[0]
        dh0, dq0, dstep = directions(h0.shape, 7 * n + D + si)
        cases = [("dh0", dict(dh0=dh0), lambda s: (h0 + s * dh0, q0, P)), ("dq0", dict(dq0=dq0), lambda s: (h0, q0 + s * dq0, P))]
        for slot in range(6):
            absent = (slot < 2 and P["lam_h"] is None) or (2 <= slot < 4 and P["lam_q"] is None) or (slot == 4 and instant)
            one = np.zeros(6)
            one[slot] = 1.0
            if absent:
                _, tan = TO.bake_jvp(h0, q0, S, **P, dstep=one)
                assert all(np.array_equal(t, np.zeros(h0.shape)) for t in tan), (si, slot)     # a slot the step does not use
                continue
            cases.append((RP.SLOTS[slot], dict(dstep=one), lambda s, slot=slot: (h0, q0, perturbed(P, slot, s))))
        for name, kw, at in cases:
            prim, tan = TO.bake_jvp(h0, q0, S, **P, **kw)
            assert all(np.array_equal(a, b) for a, b in zip(prim, PO.bake(h0, q0, S, **P)))      # the primal is the forward oracle's
            (hp, qp, Pp), (hm, qm, Pm) = at(e), at(-e)
            up, dn = PO.bake(hp, qp, S, **Pp), PO.bake(hm, qm, S, **Pm)
            for out, t, u, d in zip("hqa", tan, up, dn):
                fd = (u - d) / (2 * e)
                scale = max(float(np.abs(t).max()), float(np.abs(fd).max()))
                rel = float(np.abs(t - fd).max()) / scale if scale > 0 else 0.0
                assert rel <= (1e-5 if instant else FD_BOUND), (si, name, out, rel)
                worst = max(worst, rel)
    print(f"bake tangent n {n} D {D}: worst |tangent - central difference| / max = {worst:.1e}")


@pytest.mark.parametrize("n,D", SHAPES)
def test_the_exposure_and_rate_tangents_against_central_differences(n, D):
    rng = np.random.default_rng(50 * n + D)
    gains, C, e = (0.8, 1.0, 1.3), 0.05, 1e-6
    I = rng.uniform(0.0, 40.0, (2, D, n, n))
    I[0, 0, 0, 0] = -1.0                                                        # a NaN acid: exactly 0 whatever the direction
    dI, dC = rng.uniform(-1.0, 1.0, I.shape), 0.7
    t = TO.expose_jvp(I, gains, C, dC, dI)
    with np.errstate(invalid="ignore"):
        fd = (PO.expose(I + e * dI, gains, C + e * dC) - PO.expose(I - e * dI, gains, C - e * dC)) / (2 * e)
    dead = np.isnan(fd)
    assert dead.sum() == 3 and np.array_equal(t[dead], np.zeros(3))
    rel = float(np.abs(t - fd)[~dead].max() / np.abs(t).max())
    print(f"exposure tangent n {n} D {D}: {rel:.1e}")
    assert rel <= FD_BOUND
    # the rate law: x, and each physical parameter through rate_param_tangent
    for r0, delta in ((1.0, 1.0), (0.4, 35.0)):
        x = rng.uniform(0.0, 60.0, (2, D, n, n))
        x[1, D - 1, n - 1, 0] = -2.0                                            # a wall
        kappa = 0.04
        par = [kappa, MACK["r_max"], MACK["r_min"], MACK["q"], MACK["m_th"], r0, delta]
        slow = lambda xx, p: DO.slowness(xx, gains, p[0], p[1], p[2], p[3], p[4], THICK, p[5], p[6])     # noqa: E731
        dx = rng.uniform(-1.0, 1.0, x.shape)
        cases = [("x", dx, np.zeros(7))]
        for k in range(7):
            if r0 == 1.0 and k == 5:
                continue                                                        # r0 + e would leave the domain
            one = np.zeros(7)
            one[k] = 1.0
            cases.append((RP.RATE_PARAMETERS[k], None, one))
        for name, ddx, dp in cases:
            dphi = TO.rate_param_tangent(*par[1:5], THICK, r0, delta, D, dp)
            t = TO.rate_jvp(x, gains, *par[:5], THICK, r0, delta, dx=ddx, dphi=dphi)
            step = e * max(1.0, float(np.abs(par) @ np.abs(dp)))
            pp, pm = list(np.array(par) + step * dp), list(np.array(par) - step * dp)
            with np.errstate(invalid="ignore"):
                fd = (slow(x + (step * ddx if ddx is not None else 0.0), pp) - slow(x - (step * ddx if ddx is not None else 0.0), pm)) / (2 * step)
            dead = np.isnan(fd)
            assert dead.sum() == 3 and np.array_equal(t[dead], np.zeros(3)), name
            if r0 == 1.0 and name == "surfaceDepth":
                assert not t.any() and not fd[~dead].any()                     # f = 1 whatever the depth
                continue
            rel = float(np.abs(t - fd)[~dead].max() / np.abs(t).max())
            print(f"rate tangent n {n} D {D} r0 {r0} {name}: {rel:.1e}")
            assert rel <= FD_BOUND, name


@pytest.mark.parametrize("n,D,walls", [(12, 4, False), (17, 3, True), (9, 6, False)])
def test_the_front_tangent_against_central_differences(n, D, walls):
    """dT against (T(s + e ds) - T(s - e ds)) / 2e per cell, the cases of test_develop_grad_cpu.  T is piecewise smooth in s: a
    cell whose branch flips inside the bracket is off by O(e) of its own value, so the bound is 1e-5 of max |dT|."""
    rng = np.random.default_rng(100 * n + D)
    s = np.exp(rng.standard_normal((D, n, n))) * 0.05
    if walls:
        s[1, 3, 4:9] = np.nan
        s[0, 10, 10], s[2, 5, 5], s[1, 0, 0] = np.inf, np.nan, -1.0
        s[:, 12:15, 12] = np.nan
    T, _ = DO.arrival_time(s, THICK, H)
    reached = np.isfinite(T)
    ds = np.where(reached, s * rng.uniform(-1.0, 1.0, s.shape), np.nan)         # ignored where the cell has no gradient
    dT = TO.time_jvp(T, s, ds, THICK, H)
    assert np.isfinite(dT).all() and (dT[~reached] == 0.0).all()
    e = 1e-6
    Tp, _ = DO.arrival_time(np.where(reached, s + e * ds, s), THICK, H)
    Tm, _ = DO.arrival_time(np.where(reached, s - e * ds, s), THICK, H)
    fd = (Tp[reached] - Tm[reached]) / (2 * e)
    rel = float(np.abs(dT[reached] - fd).max() / np.abs(dT).max())
    print(f"front tangent n {n} D {D}: max |dT - central difference| / max |dT| = {rel:.1e}")
    assert rel <= 1e-5


# ---- 2. duality with the adjoint oracles --------------------------------------------------------------------------------------------
def dual(lhs_terms, rhs_terms):
    lhs, rhs = sum(float(t.sum()) for t in lhs_terms), sum(float(t.sum()) for t in rhs_terms)
    mass = sum(float(np.abs(t).sum()) for t in lhs_terms) + sum(float(np.abs(t).sum()) for t in rhs_terms)
    return abs(lhs - rhs) / mass if mass > 0 else abs(lhs - rhs), lhs, rhs


@pytest.mark.parametrize("n,D", SHAPES)
def test_the_bake_tangent_is_the_transpose_of_the_adjoint_oracle(n, D):
    S, q0 = 5, 0.3
    for si, base in enumerate(STEP_SETS):
        P = dict(base, half_dt=0.5 * BAKE / S)
        h0, gh, gq, ga = volumes(n, D, clear_seed(n, D, S, P, q0) if math.isinf(P["beta"]) else 0)
        dh0, dq0, dstep = directions(h0.shape, 11 * n + D + si)
        _, (dh, dq, da) = TO.bake_jvp(h0, q0, S, **P, dh0=dh0, dq0=dq0, dstep=dstep)
        grad, _, hb, qb = RP.bake_param_vjp(h0, q0, S, gh, gq, ga, **P)
        rel, lhs, rhs = dual([gh * dh, gq * dq, ga * da], [hb * dh0, qb * dq0, grad * dstep[None]])
        print(f"bake duality n {n} D {D} set {si}: <g, Jv> {lhs:+.12e} <J^T g, v> {rhs:+.12e} rel {rel:.1e}")
        assert rel <= DUAL_BOUND, si


@pytest.mark.parametrize("n,D", SHAPES)
def test_the_pointwise_and_front_tangents_are_the_transposes_of_the_adjoint_oracles(n, D):
    rng = np.random.default_rng(77 * n + D)
    gains, C = (0.8, 1.0, 1.3), 0.05
    I = rng.uniform(0.0, 40.0, (2, D, n, n))
    I[1, 0, 0, 0] = -1.0
    dI, dC = rng.uniform(-1.0, 1.0, I.shape), -0.4
    g = rng.uniform(-1.0, 1.0, (6, D, n, n))
    sums, _ = RP.expose_param_sums(I, gains, C, g)
    with np.errstate(invalid="ignore"):
        ok = np.tile(1.0 - np.exp(-C * I) >= 0.0, (3, 1, 1, 1))
    gI = GO.expose_vjp(np.where(I < 0, 0.0, I), gains, C, np.where(ok, g, 0.0))          # the adjoint oracle has no wall rule of its own
    rel, lhs, rhs = dual([g * TO.expose_jvp(I, gains, C, dC, dI)], [gI * np.where(I < 0, 0.0, dI), sums * dC])
    print(f"exposure duality n {n} D {D}: {lhs:+.12e} {rhs:+.12e} rel {rel:.1e}")
    assert rel <= DUAL_BOUND
    # the rate law with the surface factor: x and the six slots; then its chain to the seven physical parameters
    r0, delta, kappa = 0.4, 35.0, 0.04
    par = (kappa, MACK["r_max"], MACK["r_min"], MACK["q"], MACK["m_th"], THICK, r0, delta)
    x = rng.uniform(0.0, 60.0, (2, D, n, n))
    x[0, 0, 0, 0] = -2.0
    dx, dphi, dp = rng.uniform(-1.0, 1.0, x.shape), rng.uniform(-1.0, 1.0, (D, 6)), rng.uniform(-1.0, 1.0, 7)
    gx = DGO.rate_vjp(x, gains, *par, g)
    psums, _ = RP.rate_param_sums(x, gains, *par, g)
    rel, lhs, rhs = dual([g * TO.rate_jvp(x, gains, *par, dx=dx, dphi=dphi)], [gx * dx, psums * dphi[None]])
    print(f"rate duality n {n} D {D}: {lhs:+.12e} {rhs:+.12e} rel {rel:.1e}")
    assert rel <= DUAL_BOUND
    chain = RP.rate_param_chain(psums, *par[1:5], THICK, r0, delta)
    rel, lhs, rhs = dual([psums * TO.rate_param_tangent(*par[1:5], THICK, r0, delta, D, dp)[None]], [chain * dp[None]])
    assert rel <= DUAL_BOUND
    # the front
    s = np.exp(rng.standard_normal((D, n, n))) * 0.05
    if n >= 5:
        s[0, 2, 1:4] = np.nan
    T, _ = DO.arrival_time(s, THICK, H)
    gT, ds = rng.standard_normal(T.shape), s * rng.uniform(-1.0, 1.0, s.shape)
    rel, lhs, rhs = dual([np.where(np.isfinite(T), gT, 0.0) * TO.time_jvp(T, s, ds, THICK, H)],
                         [DGO.time_vjp(T, s, gT, THICK, H) * np.where(np.isfinite(s), ds, 0.0)])
    print(f"front duality n {n} D {D}: {lhs:+.12e} {rhs:+.12e} rel {rel:.1e}")
    assert rel <= DUAL_BOUND


def test_the_fp32_gather_agrees_with_the_ordered_tangent():
    """The device's iteration restated in fp32 against the ordered float64 solve on the same fp32 links: 1e-5 of max |dT|."""
    rng = np.random.default_rng(16)
    s = (np.exp(rng.standard_normal((4, 16, 16))) * 0.05).astype(np.float32).astype(np.float64)
    T = DO.arrival_time(s, THICK, H)[0].astype(np.float32).astype(np.float64)
    L, sigma = DGO.links(T, s, H, THICK / 4)
    ds = rng.standard_normal(s.shape).astype(np.float32)
    got, sweeps = TO.gather_fp32_tangent(L, sigma, ds)
    want = TO.ordered_tangent(T, L.astype(np.float32).astype(np.float64), sigma.astype(np.float32).astype(np.float64), ds)
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"fp32 gather: {sweeps} sweeps, {rel:.1e} of max |dT| from the ordered solve")
    assert got.dtype == np.float32 and rel <= 1e-5


# ---- 3. the library's host chains and the argument checks ---------------------------------------------------------------------------
NEW = ("litho_peb_expose_jvp", "litho_peb_jvp_work_bytes", "litho_peb_bake_jvp", "litho_peb_param_tangent", "litho_develop_rate_jvp",
       "litho_develop_rate_param_tangent", "litho_develop_jvp_work_bytes", "litho_develop_time_jvp")


def test_new_symbols_are_bound(nat):
    import lithographysimulator_amd as L
    names = nat.exported_symbols()
    for must in NEW:
        assert must in names and hasattr(nat.lib(), must)
    for name in ("exposeAcidTangent", "bakeTangent", "bakeParameterTangent", "developmentRateTangent", "amplifiedRateTangent",
                 "rateParameterTangent", "developmentTimeTangent", "resistProfileTangent", "calibrationJacobian"):
        assert name in L.__all__ and hasattr(L, name)
    from lithographysimulator_amd import tangent
    assert tangent.MAX_DIRECTIONS == 16


def test_the_library_bake_chain_is_the_transpose_of_param_chain(nat):
    rng = np.random.default_rng(41)
    D, S, lib = 3, 9, nat.lib()
    for ri, r in enumerate(RESISTS):
        args = (THICK, H, r["kq"], r["kl"], r["sh"], r["sq"], r["vs"], BAKE, D, S)
        g, dp = rng.uniform(-1.0, 1.0, 6), rng.uniform(-1.0, 1.0, 5)
        gs, gp = (ctypes.c_double * 6)(*g), (ctypes.c_double * 5)()
        ds, dpc = (ctypes.c_double * 6)(), (ctypes.c_double * 5)(*dp)
        assert lib.litho_peb_param_chain(*args, gs, gp) == 0 and lib.litho_peb_param_tangent(*args, dpc, ds) == 0
        dstep, gparam = np.array(list(ds)), np.array(list(gp))
        lhs, rhs = float(g @ dstep), float(gparam @ dp)
        mass = float(np.abs(g) @ np.abs(dstep) + np.abs(gparam) @ np.abs(dp))
        assert abs(lhs - rhs) <= 8 * 2.0 ** -52 * mass, (ri, lhs, rhs)
        want = TO.param_tangent(*args, dp)
        assert (np.abs(dstep - want) <= 8 * 2.0 ** -52 * np.abs(want)).all(), (ri, dstep, want)
        if math.isinf(r["kq"]):
            assert dstep[4] == 0.0
        if r["sh"] == 0.0:
            assert dstep[0] == 0.0 and dstep[1] == 0.0
        if r["vs"] == 0.0:
            assert dstep[1] == 0.0 and dstep[3] == 0.0
    src, dst = (ctypes.c_double * 5)(), (ctypes.c_double * 6)()
    ok = (THICK, H, 2.0, 0.01, 25.0, 15.0, 1.0, BAKE, D, S)
    for i, bad in ((2, -1.0), (2, float("nan")), (3, -0.1), (3, float("inf")), (7, 0.0), (1, 0.0), (8, 0), (8, 33), (9, 0), (9, 65537), (4, -1.0)):
        a = list(ok)
        a[i] = bad
        assert lib.litho_peb_param_tangent(*a, src, dst) == nat.E_ARG, (i, bad)
    assert lib.litho_peb_param_tangent(*ok, None, dst) == nat.E_ARG and lib.litho_peb_param_tangent(*ok, src, None) == nat.E_ARG


def test_the_library_rate_chain_is_the_transpose_of_rate_param_chain(nat):
    rng = np.random.default_rng(42)
    lib = nat.lib()
    for D, r0, delta in ((1, 1.0, 1.0), (3, 0.25, 30.0), (5, 0.6, 55.0)):
        t, dp = rng.uniform(-1.0, 1.0, (1, D, 6)), rng.uniform(-1.0, 1.0, 7)
        args = (120.0, 0.05, 5.0, 0.4, r0, delta, THICK, D)
        ts, gp = (ctypes.c_double * (D * 6))(*t.reshape(-1)), (ctypes.c_double * 7)()
        dpc, phi = (ctypes.c_double * 7)(*dp), (ctypes.c_double * (D * 6))()
        assert lib.litho_develop_rate_param_chain(*args, 1, ts, gp) == 0 and lib.litho_develop_rate_param_tangent(*args, dpc, phi) == 0
        dphi, gparam = np.array(list(phi)).reshape(D, 6), np.array(list(gp))
        lhs, rhs = float((t[0] * dphi).sum()), float(gparam @ dp)
        mass = float((np.abs(t[0]) * np.abs(dphi)).sum() + np.abs(gparam) @ np.abs(dp))
        assert abs(lhs - rhs) <= 16 * D * 2.0 ** -52 * mass, (D, lhs, rhs)
        want = TO.rate_param_tangent(120.0, 0.05, 5.0, 0.4, THICK, r0, delta, D, dp)
        assert (np.abs(dphi - want) <= 16 * 2.0 ** -52 * (np.abs(want) + np.abs(dp).max())).all(), D
    src, dst = (ctypes.c_double * 7)(), (ctypes.c_double * 6)()
    ok = (120.0, 0.05, 5.0, 0.4, 1.0, 1.0, THICK, 1)
    for i, bad in ((0, 0.0), (1, -1.0), (2, 1.0), (3, 1.0), (3, -0.1), (4, 0.0), (4, 1.5), (5, 0.0), (6, 0.0), (7, 0), (7, 33)):
        a = list(ok)
        a[i] = bad
        assert lib.litho_develop_rate_param_tangent(*a, src, dst) == nat.E_ARG, (i, bad)
    assert lib.litho_develop_rate_param_tangent(*ok, None, dst) == nat.E_ARG and lib.litho_develop_rate_param_tangent(*ok, src, None) == nat.E_ARG


def test_work_bytes_are_the_header_formulas(nat):
    lib = nat.lib()
    for B, D, n, P, it in ((3, 5, 17, 1, 64), (3, 5, 17, 16, 1024), (1, 1, 1, 3, 1), (2, 32, 48, 8, 65536), (1, 16, 2048, 8, 1024)):
        cells = B * D * n * n
        assert lib.litho_peb_jvp_work_bytes(B, D, n, P) == (5 + 2 * P) * 4 * cells
        assert lib.litho_develop_jvp_work_bytes(B, D, n, P, it) == -(-4 * it // 256) * 256 + (4 + P) * 4 * cells
    for bad in ((0, 5, 17, 1), (1, 0, 17, 1), (1, 33, 17, 1), (1, 5, 0, 1), (1, 5, 16385, 1), (1, 5, 17, 0), (1, 5, 17, 17), (1024, 8, 17, 8)):
        assert lib.litho_peb_jvp_work_bytes(*bad) == 0, bad
        assert lib.litho_develop_jvp_work_bytes(*bad, 64) == 0, bad
    assert lib.litho_develop_jvp_work_bytes(1, 5, 17, 1, 0) == 0 and lib.litho_develop_jvp_work_bytes(1, 5, 17, 1, 65537) == 0


def tangent_argument_errors(nat):
    """Every refused call of the four new GPU entry points returns its code before the first HIP call; the pointers are never
    dereferenced.  Shared with the GPU suite.  Returns the number of refused calls."""
    lib = nat.lib()
    V = 4 * 4 * 64                                                             # bytes of a [1, 4, 8, 8] volume
    P, S = 2, 8
    p = [ctypes.c_void_p(1 << 20 + i) for i in range(11)]                        # far apart: 1 MiB, 2 MiB, 4 MiB, ...
    nan, inf, E = float("nan"), float("inf"), nat.E_ARG
    near = lambda base, off: ctypes.c_void_p(base.value + off)                   # noqa: E731
    g = (ctypes.c_float * 64)(*([1.0] * 64))
    gnan = (ctypes.c_float * 2)(1.0, nan)
    two = (ctypes.c_double * 2)(0.5, -0.5)
    twonan = (ctypes.c_double * 2)(0.5, nan)
    count = 0
    # litho_peb_expose_jvp(image, volumes, D, n, gains, n_gains, C, P, dC, dimage, dacid, stream)
    ok = dict(image=p[0], volumes=1, D=4, n=8, gains=g, n_gains=2, C=0.05, P=P, dC=two, dI=p[1], out=p[2])
    bad = [dict(image=None), dict(out=None), dict(dC=None), dict(dC=twonan), dict(gains=None), dict(n_gains=0), dict(n_gains=65), dict(gains=gnan),
           dict(volumes=0), dict(D=0), dict(D=33), dict(n=0), dict(n=16385), dict(volumes=8192), dict(C=0.0), dict(C=nan), dict(C=inf), dict(P=0),
           dict(P=17), dict(volumes=4096, P=4), dict(out=p[0]), dict(out=near(p[0], V - 16)), dict(out=p[1]), dict(out=near(p[1], 2 * V - 16)),
           dict(out=near(p[1], -4 * V + 16))]
    for kw in bad:
        assert lib.litho_peb_expose_jvp(*{**ok, **kw}.values(), None) == E, kw
    count += len(bad)
    # litho_peb_bake_jvp(acid_in, B, D, n, thickness, pixel, q0, kq, kl, sh, sq, vs, t, steps, P, dacid_in, dq0, dstep, acid, quencher,
    #                    acid_dose, dacid, dquencher, dacid_dose, work, wb, stream)
    W = lib.litho_peb_jvp_work_bytes(1, 4, 8, P)
    assert W == (5 + 2 * P) * V
    dstep = (ctypes.c_double * 12)(*([0.01] * 12))
    dstepnan = (ctypes.c_double * 12)(*([0.01] * 11 + [nan]))
    ok = dict(acid_in=p[0], B=1, D=4, n=8, thickness=100.0, pixel=25.0, q0=0.1, kq=5.0, kl=0.01, sh=20.0, sq=5.0, vs=1.0, t=60.0, steps=S, P=P,
              dh=p[1], dq0=two, dstep=dstep, h=p[2], q=p[3], a=p[4], oh=p[5], oq=p[6], oa=p[7], work=p[8], wb=W)
    least = lib.litho_peb_min_steps(20.0, 5.0, 1.0, 100.0, 4, 25.0)
    bad = [dict(steps=least - 1), dict(steps=0), dict(steps=65537), dict(B=0), dict(D=0), dict(D=33), dict(n=0), dict(n=16385), dict(B=16384),
           dict(P=0), dict(P=17), dict(B=4096, P=8), dict(acid_in=None), dict(dq0=None), dict(dstep=None), dict(dq0=twonan), dict(dstep=dstepnan),
           dict(oh=None), dict(oq=None), dict(oa=None), dict(work=None), dict(work=near(p[8], 4)),
           dict(thickness=0.0), dict(pixel=nan), dict(q0=-0.1), dict(kq=-1.0), dict(kq=nan), dict(kl=inf), dict(sh=-1.0), dict(vs=-1.0), dict(t=0.0),
           # an output over an input, another output or the workspace
           dict(oh=p[0]), dict(oh=p[1]), dict(oh=near(p[1], 2 * V - 16)), dict(oq=p[5]), dict(oq=near(p[5], 2 * V - 16)), dict(oa=p[6]),
           dict(oa=near(p[8], W - 16)), dict(oh=near(p[8], -2 * V + 16)), dict(h=p[0]), dict(h=p[3]), dict(q=p[4]), dict(a=p[5]),
           dict(a=near(p[8], W - 16)), dict(h=near(p[1], 2 * V - 16)), dict(work=near(p[0], V - 16)), dict(work=near(p[1], 2 * V - 16))]
    for kw in bad:
        assert lib.litho_peb_bake_jvp(*{**ok, **kw}.values(), None) == E, kw
    assert lib.litho_peb_bake_jvp(*{**ok, "wb": W - 1}.values(), None) == nat.E_WORKSPACE
    count += len(bad) + 1
    # litho_develop_rate_jvp(x, volumes, D, n, gains, n_gains, kappa, rmax, rmin, q, mth, r0, delta, thickness, P, dx, dphi, out, stream)
    ok = dict(x=p[0], volumes=1, D=4, n=8, gains=g, n_gains=2, kappa=0.05, rmax=120.0, rmin=0.05, q=5.0, mth=0.4, r0=1.0, delta=1.0, thick=100.0,
              P=P, dx=p[1], dphi=p[2], out=p[3])
    bad = [dict(x=None), dict(dphi=None), dict(out=None), dict(gains=None), dict(n_gains=0), dict(n_gains=65), dict(gains=gnan), dict(volumes=0),
           dict(D=0), dict(D=33), dict(n=0), dict(n=16385), dict(volumes=8192), dict(kappa=0.0), dict(kappa=nan), dict(rmax=0.0), dict(rmin=-1.0),
           dict(q=1.0), dict(mth=1.0), dict(r0=0.0), dict(delta=0.0), dict(thick=0.0), dict(P=0), dict(P=17), dict(volumes=4096, P=4),
           dict(dphi=near(p[2], 8)), dict(out=p[0]), dict(out=near(p[0], V - 16)), dict(out=p[1]), dict(out=near(p[1], 2 * V - 16)), dict(out=p[2]),
           dict(out=near(p[2], P * 4 * 48 - 16)), dict(out=near(p[2], -4 * V + 16))]
    for kw in bad:
        assert lib.litho_develop_rate_jvp(*{**ok, **kw}.values(), None) == E, kw
    count += len(bad)
    # litho_develop_time_jvp(slowness, T, dslowness, B, D, n, P, thickness, pixel, max_iterations, dT, work, wb, launches, stream)
    Wt = lib.litho_develop_jvp_work_bytes(1, 4, 8, P, 64)
    assert Wt == 256 + (4 + P) * V
    launches = ctypes.c_int(7)
    ok = dict(s=p[0], T=p[1], ds=p[2], B=1, D=4, n=8, P=P, thick=100.0, pixel=25.0, it=64, out=p[3], work=p[4], wb=Wt, launches=ctypes.byref(launches))
    bad = [dict(s=None), dict(T=None), dict(ds=None), dict(out=None), dict(work=None), dict(launches=None), dict(B=0), dict(D=0), dict(D=33), dict(n=0),
           dict(n=16385), dict(B=16384), dict(P=0), dict(P=17), dict(B=4096, P=8), dict(thick=0.0), dict(pixel=nan), dict(pixel=1e30), dict(it=0),
           dict(it=65537), dict(work=near(p[4], 8)), dict(out=p[0]), dict(out=p[1]), dict(out=p[2]), dict(out=near(p[2], 2 * V - 16)),
           dict(out=near(p[0], -2 * V + 16)), dict(work=p[0]), dict(work=near(p[1], V - 16)), dict(work=near(p[2], 2 * V - 16)),
           dict(work=near(p[3], 2 * V - 16)), dict(out=near(p[4], Wt - 16))]
    for kw in bad:
        launches.value = 7
        assert lib.litho_develop_time_jvp(*{**ok, **kw}.values(), None) == E, kw
        assert kw.get("launches", 1) is None or launches.value == 0
    assert lib.litho_develop_time_jvp(*{**ok, "wb": Wt - 1}.values(), None) == nat.E_WORKSPACE
    return count + len(bad) + 1


def test_argument_errors_come_back_before_any_gpu_call(nat):
    assert tangent_argument_errors(nat) > 120
