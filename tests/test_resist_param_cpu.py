"""Gradients with respect to the resist's parameters without a GPU: tests/resist_param_oracle.py (the float64 restatement that
tests/test_gpu_resist_param.py measures the kernels against) pinned to central differences of the forward oracles and to closed
forms, the two host chains of the library against it, and the argument errors of the new entry points, which come back as codes
before any GPU call.

The finite-difference bound.  A derivative g of l(theta) is compared with the central difference fd = (l(theta + e) - l(theta -
e)) / (2 e) as |fd - g| / M, M the sum of the absolute per-cell (per-step) terms that make up g, so a cancellation cannot flatter
it.  The truncation is e^2 l''' / 6 and the rounding 2^-52 |l| / e.  Step parameters (all of order 0.01 ... 1, l''' of order
beta^2 |l|): e = 1e-6 gives ~1e-10 and ~2e-10 |l| / M.  Physical parameters are perturbed RELATIVELY, e = 1e-6 theta, and compared
relatively to sum_slot |chain coefficient| M_slot.  Instantaneous neutralisation: the bake is piecewise smooth in the parameters
(the branch hd < qd can flip), e = 1e-8 and the trajectory must stay clear of a tie (asserted: min |hd - qd| >= 1e-5), rounding
~2e-8.  Bound: 1e-6 for all, as tests/test_peb_grad_cpu.py; a missing term or a wrong sign is wrong at 1e-1.  Observed: 1e-8 ...
1e-12."""
import ctypes
import math

import numpy as np
import pytest

import develop_oracle as DO
import peb_grad_oracle as GO
import peb_oracle as PO
import resist_param_oracle as RP

FD_BOUND = 1e-6
BAKE, THICK, H = 60.0, 100.0, 25.0
SHAPES = [(1, 1), (2, 3), (5, 3), (5, 1), (2, 1)]


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    return _native


def volumes(n, D, seed):
    rng = np.random.default_rng(1000 * n + 10 * D + seed)
    shape = (2, D, n, n)
    h0 = rng.uniform(0.0, 1.0, shape)
    gh, gq, ga = (rng.uniform(-1.0, 1.0, shape) for _ in range(3))
    return h0, gh, gq, ga / BAKE


STEP_SETS = [dict(lam_h=(0.11, 0.07), lam_q=(0.05, 0.02), beta=2.0, fl=0.97), dict(lam_h=(0.11, 0.07), lam_q=None, beta=0.6, fl=1.0),
             dict(lam_h=None, lam_q=(0.05, 0.02), beta=2.0, fl=0.9), dict(lam_h=None, lam_q=None, beta=5.0, fl=0.97),
             dict(lam_h=(0.11, 0.07), lam_q=(0.05, 0.02), beta=math.inf, fl=0.97), dict(lam_h=(0.2, 0.0), lam_q=None, beta=math.inf, fl=1.0)]


def perturbed(P, slot, e):
    Q = dict(P)
    if slot < 4:
        key = "lam_h" if slot < 2 else "lam_q"
        lam = list(Q[key])
        lam[slot & 1] += e
        Q[key] = tuple(lam)
    else:
        Q["beta" if slot == 4 else "fl"] += e
    return Q


def clear_seed(n, D, S, P, q0):
    for seed in range(32):
        if GO.branch_margin(GO.tape(volumes(n, D, seed)[0], q0, S, **P)[0]) >= 1e-5:
            return seed
    raise AssertionError("no seed keeps the instantaneous branch clear")


@pytest.mark.parametrize("n,D", SHAPES)
def test_the_six_rows_against_central_differences_of_the_bake(n, D):
    S, q0, worst = 5, 0.3, 0.0
    for si, base in enumerate(STEP_SETS):
        P = dict(base, half_dt=0.5 * BAKE / S)
        instant = math.isinf(P["beta"])
        e = 1e-8 if instant else 1e-6
        h0, gh, gq, ga = volumes(n, D, clear_seed(n, D, S, P, q0) if instant else 0)
        grad, mass, hb, qb = RP.bake_param_vjp(h0, q0, S, gh, gq, ga, **P)
        want_h, want_q = GO.bake_vjp(h0, q0, S, gh, gq, ga, **P)
        assert np.array_equal(hb, want_h) and np.array_equal(qb, want_q)       # the same backward sweep as the gradient oracle's
        loss = lambda Q: sum(float((g * o).sum()) for g, o in zip((gh, gq, ga), PO.bake(h0, q0, S, **Q)))   # noqa: E731
        for slot in range(6):
            absent = (slot < 2 and P["lam_h"] is None) or (2 <= slot < 4 and P["lam_q"] is None) or (slot == 4 and instant)
            if absent:
                assert np.array_equal(grad[:, slot], np.zeros(2)) and np.array_equal(mass[:, slot], np.zeros(2)), (si, slot)
                continue
            fd = (loss(perturbed(P, slot, e)) - loss(perturbed(P, slot, -e))) / (2 * e)
            M = float(mass[:, slot].sum())
            if n == 1 and slot in (0, 2):
                assert np.array_equal(grad[:, slot], np.zeros(2)) and M == 0.0   # one cell per plane: no lateral neighbour
            rel = abs(fd - float(grad[:, slot].sum())) / M if M > 0 else abs(fd)
            print(f"n {n} D {D} set {si} slot {RP.SLOTS[slot]}: fd {fd:+.9e} oracle {grad[:, slot].sum():+.9e} rel {rel:.1e}")
            assert rel <= FD_BOUND, (si, slot)
            worst = max(worst, rel)
    print(f"n {n} D {D}: worst relative difference {worst:.1e} (bound {FD_BOUND:.0e})")


RESISTS = [dict(kq=0.8, kl=0.0, sh=30.0, sq=0.0, vs=1.0), dict(kq=math.inf, kl=0.02, sh=30.0, sq=12.0, vs=0.5),
           dict(kq=3.0, kl=0.01, sh=25.0, sq=15.0, vs=1.0), dict(kq=math.inf, kl=0.0, sh=30.0, sq=0.0, vs=0.0),
           dict(kq=2.0, kl=0.03, sh=0.0, sq=20.0, vs=1.2), dict(kq=2.0, kl=0.03, sh=0.0, sq=0.0, vs=1.0)]
NAMES = ("kq", "kl", "sh", "sq", "vs")


def unrounded(r, D, S):
    """The step parameters of a resist in double (no fp32 rounding: the chain is the analytic derivative)."""
    hz = THICK / D
    lam = lambda s: PO.lambdas(s, r["vs"], H, hz, S) if s > 0.0 else None      # noqa: E731
    dt = BAKE / S
    return dict(lam_h=lam(r["sh"]), lam_q=lam(r["sq"]), beta=r["kq"] * dt, fl=math.exp(-r["kl"] * dt), half_dt=0.5 * dt)


@pytest.mark.parametrize("n,D", [(2, 3), (5, 3), (1, 1), (5, 1)])
def test_the_physical_parameters_against_central_differences_of_the_bake(n, D):
    S, q0 = 9, 0.3
    for ri, r in enumerate(RESISTS):
        assert PO.min_steps(r["sh"], r["sq"], r["vs"], THICK, D, H) <= S
        P = unrounded(r, D, S)
        instant = math.isinf(r["kq"])
        h0, gh, gq, ga = volumes(n, D, clear_seed(n, D, S, P, q0) if instant else 0)
        grad, mass, _, _ = RP.bake_param_vjp(h0, q0, S, gh, gq, ga, **P)
        args = lambda rr: (THICK, H, rr["kq"], rr["kl"], rr["sh"], rr["sq"], rr["vs"], BAKE, D, S)   # noqa: E731
        got = RP.param_chain(*args(r), grad).sum(axis=0)
        loss = lambda rr: sum(float((g * o).sum()) for g, o in zip((gh, gq, ga), PO.bake(h0, q0, S, **unrounded(rr, D, S))))   # noqa: E731
        for pi, name in enumerate(NAMES):
            unit = np.zeros(6)
            if r[name] == 0.0 or math.isinf(r[name]):
                if name != "kl":                                               # kLoss = 0 still has a derivative
                    assert got[pi] == 0.0 or name == "vs", (ri, name)         # an absent species, an instantaneous kQuench
                    if name != "vs":
                        continue
            e = (1e-8 if instant else 1e-6) * (r[name] if r[name] > 0.0 else 1.0)
            up, dn = dict(r), dict(r)
            up[name], dn[name] = r[name] + e, max(r[name] - e, 0.0)
            fd = (loss(up) - loss(dn)) / (up[name] - dn[name])
            # the scale: each slot's absolute mass through the magnitude of its chain coefficient
            M = 0.0
            for slot in range(6):
                unit[:] = 0.0
                unit[slot] = 1.0
                M += abs(RP.param_chain(*args(r), unit)[pi]) * float(mass[:, slot].sum())
            one_sided = dn[name] == 0.0 and r[name] == 0.0
            rel = abs(fd - got[pi]) / M if M > 0 else abs(fd - got[pi])
            print(f"n {n} D {D} resist {ri} {name}: fd {fd:+.9e} chain {got[pi]:+.9e} rel {rel:.1e}{' (one-sided)' if one_sided else ''}")
            assert rel <= (1e-4 if one_sided else FD_BOUND), (ri, name)


def test_closed_forms():
    rng = np.random.default_rng(21)
    S, half_dt = 7, 0.5 * BAKE / 7
    shape = (2, 3, 5, 5)
    gh, gq, ga = (rng.uniform(-1.0, 1.0, shape) for _ in range(3))
    # a uniform h0 with a uniform q0 stays uniform: every Laplacian is exactly 0
    uniform = np.full(shape, 0.625)
    grad, mass, _, _ = RP.bake_param_vjp(uniform, 0.25, S, gh, gq, ga, (0.125, 0.0625), (0.0625, 0.03125), 2.0, 0.96875, half_dt)
    assert np.array_equal(grad[:, :4], np.zeros((2, 4))) and np.array_equal(mass[:, :4], np.zeros((2, 4)))
    # no quencher, no diffusion, gh only: h_S = h0 fl^S, so slot 5 is S fl^(S-1) sum gh h0 and slot 4 is 0 (qd = 0)
    h0, fl = rng.uniform(0.0, 1.0, shape), 0.97
    grad, _, _, _ = RP.bake_param_vjp(h0, 0.0, S, gh, None, None, None, None, 2.0, fl, half_dt)
    want = S * fl ** (S - 1) * (gh * h0).sum(axis=(1, 2, 3))
    err = float(np.abs(grad[:, 5] - want).max() / np.abs(gh * h0).sum())
    print(f"slot fl = S fl^(S-1) sum gh h0: relative error {err:.1e}")
    assert err <= 8 * S * 2.0 ** -52 and np.array_equal(grad[:, :5], np.zeros((2, 5)))
    # one cell per plane: no lateral neighbour, the lateral slots are exactly 0 while the vertical ones are not
    col = rng.uniform(0.0, 1.0, (2, 3, 1, 1))
    g1 = rng.uniform(-1.0, 1.0, col.shape)
    grad, mass, _, _ = RP.bake_param_vjp(col, 0.3, S, g1, g1, None, (0.1, 0.2), (0.05, 0.1), 2.0, 0.97, half_dt)
    assert np.array_equal(mass[:, [0, 2]], np.zeros((2, 2))) and (mass[:, [1, 3]] > 0).all()


# ---- the rate law and the exposure -------------------------------------------------------------------------------------------------
MACK = dict(r_max=120.0, r_min=0.05, q=5.0, m_th=0.4)


@pytest.mark.parametrize("n,D", [(1, 1), (2, 3), (5, 3)])
@pytest.mark.parametrize("r0,delta", [(1.0, 1.0), (0.25, 30.0)])
def test_the_rate_sums_and_their_chain_against_central_differences(n, D, r0, delta):
    """Both uses of the rate law: kappa = C with three gains on an intensity, kappa = kAmp with one gain of 1 on an acid dose."""
    rng = np.random.default_rng(n + 10 * D)
    for kappa, gains, top in ((0.9, (0.6, 1.0, 1.7), 3.0), (0.05, (1.0,), 80.0)):
        x = rng.uniform(0.0, top, (2, D, n, n))
        x.flat[0] = 0.0                                                        # unexposed: b = 0, the q slot's explicit 0
        gs = rng.uniform(-1.0, 1.0, (2 * len(gains), D, n, n))
        sums, mass = RP.rate_param_sums(x, gains, kappa, MACK["r_max"], MACK["r_min"], MACK["q"], MACK["m_th"], THICK, r0, delta, gs)
        assert sums.shape == (2 * len(gains), D, 6)
        got = RP.rate_param_chain(sums, MACK["r_max"], MACK["r_min"], MACK["q"], MACK["m_th"], THICK, r0, delta).sum(axis=0)
        base = dict(kappa=kappa, rMax=MACK["r_max"], rMin=MACK["r_min"], q=MACK["q"], mTh=MACK["m_th"], surfaceRate=r0, surfaceDepth=delta)

        def loss(p):
            return float((gs * DO.slowness(x, gains, p["kappa"], p["rMax"], p["rMin"], p["q"], p["mTh"], THICK, p["surfaceRate"], p["surfaceDepth"])).sum())
        scale = float(np.abs(gs * DO.slowness(x, gains, kappa, MACK["r_max"], MACK["r_min"], MACK["q"], MACK["m_th"], THICK, r0, delta)).sum())
        for pi, name in enumerate(RP.RATE_PARAMETERS):
            if name in ("surfaceRate", "surfaceDepth") and r0 == 1.0:
                if name == "surfaceDepth":
                    assert got[pi] == 0.0                                      # the factor is 1 whatever delta
                    continue
                up, dn = dict(base, surfaceRate=1.0), dict(base, surfaceRate=1.0 - 2e-6)   # one-sided: r0 <= 1
            else:
                e = 1e-6 * base[name]
                up, dn = dict(base, **{name: base[name] + e}), dict(base, **{name: base[name] - e})
            fd = (loss(up) - loss(dn)) / (up[name] - dn[name])
            # relative to the size of the derivative's own terms: |theta dl/dtheta| is at most a few times sum |gs s| here
            rel = abs(fd - got[pi]) * base[name] / scale
            print(f"n {n} D {D} kappa {kappa} r0 {r0} {name}: fd {fd:+.9e} chain {got[pi]:+.9e} rel {rel:.1e}")
            assert rel <= (1e-5 if up[name] == 1.0 and name == "surfaceRate" else FD_BOUND), name
    # a wall contributes 0 whatever its cotangent holds
    x = rng.uniform(0.5, 2.0, (1, D, n, n))
    gs = rng.uniform(-1.0, 1.0, (1, D, n, n))
    ref, _ = RP.rate_param_sums(x, (1.0,), 0.9, **MACK, thickness=THICK, r0=r0, delta=delta, grad_s=gs)
    x2, gs2 = x.copy(), gs.copy()
    x2.flat[-1], gs2.flat[-1] = -1.0, np.nan
    gs_ref = gs.copy()
    gs_ref.flat[-1] = 0.0
    ref, _ = RP.rate_param_sums(x, (1.0,), 0.9, **MACK, thickness=THICK, r0=r0, delta=delta, grad_s=gs_ref)
    got, _ = RP.rate_param_sums(x2, (1.0,), 0.9, **MACK, thickness=THICK, r0=r0, delta=delta, grad_s=gs2)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("n,D", [(1, 1), (2, 3), (5, 3)])
def test_the_exposure_sum_against_central_differences(n, D):
    rng = np.random.default_rng(n + D)
    I = rng.uniform(0.0, 3.0, (2, D, n, n))
    doses, C, e = (0.6, 1.0, 1.7), 0.9, 1e-6
    g = rng.uniform(-1.0, 1.0, (6, D, n, n))
    sums, mass = RP.expose_param_sums(I, doses, C, g)
    fd = float((g * (PO.expose(I, doses, C + e) - PO.expose(I, doses, C - e))).sum()) / (2 * e)
    rel = abs(fd - float(sums.sum())) / float(mass.sum())
    print(f"exposure dl/dC n {n} D {D}: fd {fd:+.9e} oracle {sums.sum():+.9e} rel {rel:.1e}")
    assert sums.shape == (6,) and rel <= FD_BOUND
    I2, g2 = I.copy(), g.copy()
    g0 = g.copy()
    I2.flat[0] = -0.5                                                          # a NaN acid at every dose: 0 whatever the cotangent holds
    for i in range(len(doses)):
        g2[2 * i].flat[0], g0[2 * i].flat[0] = np.nan, 0.0
    assert np.array_equal(RP.expose_param_sums(I2, doses, C, g2)[0], RP.expose_param_sums(I, doses, C, g0)[0])


# ---- the host side of the library ------------------------------------------------------------------------------------------------
NEW = ("litho_peb_vjp_params_work_bytes", "litho_peb_bake_vjp_params", "litho_peb_param_chain", "litho_peb_expose_params_work_bytes",
       "litho_peb_expose_vjp_params", "litho_develop_rate_params_work_bytes", "litho_develop_rate_vjp_params",
       "litho_develop_rate_param_chain")


def test_new_symbols_are_bound(nat):
    import lithographysimulator_amd as L
    names = nat.exported_symbols()
    for must in NEW:
        assert must in names and hasattr(nat.lib(), must)
    for name in ("bakeStepGradient", "bakeParameterGradient", "rateParameterGradient", "exposureParameterGradient", "resistParameterGradient",
                 "calibrateResist"):
        assert name in L.__all__ and hasattr(L, name)


def lib_chain(nat, r, D, S, g):
    src, dst = (ctypes.c_double * 6)(*g), (ctypes.c_double * 5)()
    rc = nat.lib().litho_peb_param_chain(THICK, H, r["kq"], r["kl"], r["sh"], r["sq"], r["vs"], BAKE, D, S, src, dst)
    assert rc == 0, rc
    return np.array(list(dst))


def test_the_library_bake_chain_against_the_oracle_and_the_step_formulas(nat):
    rng = np.random.default_rng(31)
    D, S = 3, 9
    for ri, r in enumerate(RESISTS):
        g = rng.uniform(-1.0, 1.0, 6)
        got = lib_chain(nat, r, D, S, g)
        want = RP.param_chain(THICK, H, r["kq"], r["kl"], r["sh"], r["sq"], r["vs"], BAKE, D, S, g)
        scale = np.abs(RP.param_chain(THICK, H, r["kq"], r["kl"], r["sh"], r["sq"], r["vs"], BAKE, D, S, np.abs(g))) + 1e-300
        assert (np.abs(got - want) <= 8 * 2.0 ** -52 * np.maximum(scale, np.abs(want))).all(), (ri, got, want)
        # the Jacobian, column by column, against central differences of the step parameters' own formulas
        for pi, name in enumerate(NAMES):
            if math.isinf(r[name]) or (name in ("sh", "sq") and r[name] == 0.0):
                assert got[pi] == 0.0                                          # instantaneous; lambda = sigma^2 ... has slope 0 at 0
                continue
            if name == "vs" and r[name] == 0.0:
                assert got[pi] == 0.0
                continue
            e = 1e-6 * (r[name] if r[name] > 0 else 1.0)
            up, dn = dict(r), dict(r)
            up[name], dn[name] = r[name] + e, max(r[name] - e, 0.0)
            vec = lambda rr: RP.step_vector(min(rr["kq"], 1e300), rr["kl"], rr["sh"], rr["sq"], rr["vs"], BAKE, THICK, D, H, S)   # noqa: E731
            col = (vec(up) - vec(dn)) / (up[name] - dn[name])
            if math.isinf(r["kq"]):
                col[4] = 0.0
            fd = float(col @ g)
            tol = (1e-4 if dn[name] == 0.0 and r[name] == 0.0 else 1e-8) * float(np.abs(col) @ np.abs(g)) + 1e-300
            assert abs(fd - got[pi]) <= tol, (ri, name, fd, got[pi])
    # PO.step_parameters is the fp32 rounding of the same formulas
    r = RESISTS[2]
    P = PO.step_parameters(r["kq"], r["kl"], r["sh"], r["sq"], r["vs"], BAKE, THICK, D, H, S)
    v = RP.step_vector(r["kq"], r["kl"], r["sh"], r["sq"], r["vs"], BAKE, THICK, D, H, S)
    assert np.allclose([*P["lam_h"], *P["lam_q"], P["beta"], P["fl"]], v, rtol=2.0 ** -23, atol=0)
    src, dst = (ctypes.c_double * 6)(), (ctypes.c_double * 5)()
    ok = (THICK, H, 2.0, 0.01, 25.0, 15.0, 1.0, BAKE, D, S)
    for i, bad in ((2, -1.0), (2, float("nan")), (3, -0.1), (3, float("inf")), (7, 0.0), (1, 0.0), (8, 0), (8, 33), (9, 0), (9, 65537), (4, -1.0)):
        a = list(ok)
        a[i] = bad
        assert nat.lib().litho_peb_param_chain(*a, src, dst) == nat.E_ARG, (i, bad)
    assert nat.lib().litho_peb_param_chain(*ok, None, dst) == nat.E_ARG and nat.lib().litho_peb_param_chain(*ok, src, None) == nat.E_ARG
    least = nat.lib().litho_peb_min_steps(25.0, 15.0, 1.0, THICK, D, H)
    assert nat.lib().litho_peb_param_chain(*ok[:9], least - 1, src, dst) == nat.E_ARG
    assert nat.lib().litho_peb_param_chain(*ok[:9], least, src, dst) == 0


def test_the_library_rate_chain_against_the_oracle(nat):
    rng = np.random.default_rng(32)
    for D, G, r0, delta in ((1, 1, 1.0, 1.0), (3, 4, 0.25, 30.0), (5, 2, 0.6, 55.0)):
        t = rng.uniform(-1.0, 1.0, (G, D, 6))
        src, dst = (ctypes.c_double * t.size)(*t.reshape(-1)), (ctypes.c_double * (G * 7))()
        assert nat.lib().litho_develop_rate_param_chain(120.0, 0.05, 5.0, 0.4, r0, delta, THICK, D, G, src, dst) == 0
        got = np.array(list(dst)).reshape(G, 7)
        want = RP.rate_param_chain(t, 120.0, 0.05, 5.0, 0.4, THICK, r0, delta)
        scale = RP.rate_param_chain(np.abs(t), 120.0, 0.05, 5.0, 0.4, THICK, r0, delta)
        a = DO.mack_a(5.0, 0.4)
        scale[:, 3] = np.abs(t[:, :, 3]).sum(axis=1) + np.abs(t[:, :, 4]).sum(axis=1) * abs(a * (1 / 6 - 1 / 4 + math.log(0.6)))
        assert (np.abs(got - want) <= 16 * D * 2.0 ** -52 * np.abs(scale) + 1e-300).all(), (D, G)
    src, dst = (ctypes.c_double * 6)(), (ctypes.c_double * 7)()
    ok = (120.0, 0.05, 5.0, 0.4, 1.0, 1.0, THICK, 1, 1)
    for i, bad in ((0, 0.0), (1, -1.0), (2, 1.0), (3, 1.0), (3, -0.1), (4, 0.0), (4, 1.5), (5, 0.0), (6, 0.0), (7, 0), (7, 33), (8, 0)):
        a = list(ok)
        a[i] = bad
        assert nat.lib().litho_develop_rate_param_chain(*a, src, dst) == nat.E_ARG, (i, bad)
    assert nat.lib().litho_develop_rate_param_chain(*ok, None, dst) == nat.E_ARG
    assert nat.lib().litho_develop_rate_param_chain(*ok, src, None) == nat.E_ARG


def test_work_bytes_are_the_header_formulas(nat):
    lib = nat.lib()
    for B, D, n, S, c in ((3, 5, 17, 7, 1), (3, 5, 17, 7, 3), (3, 5, 17, 7, 7), (1, 1, 1, 1, 1), (2, 32, 48, 33, 6), (1, 16, 2048, 32, 6)):
        cells, blocks = B * D * n * n, -(-n * n // 256)
        volumes_ = 2 * (math.ceil(S / c) - 1) + 4 * c + 8
        tape = -(-volumes_ * 4 * cells // 16) * 16
        assert lib.litho_peb_vjp_params_work_bytes(B, D, n, S, c) == tape + B * D * blocks * 48, (B, D, n, S, c)
        assert lib.litho_develop_rate_params_work_bytes(B, D, n, 3) == 3 * B * D * blocks * 48
        assert lib.litho_peb_expose_params_work_bytes(B, D, n, 3) == 3 * B * D * blocks * 8
    for bad in ((0, 5, 17, 7, 3), (1, 0, 17, 7, 3), (1, 33, 17, 7, 3), (1, 5, 0, 7, 3), (1, 5, 16385, 7, 3), (2048, 32, 17, 7, 3), (1, 5, 17, 0, 1),
                (1, 5, 17, 65537, 1), (1, 5, 17, 7, 0), (1, 5, 17, 7, 8)):
        assert lib.litho_peb_vjp_params_work_bytes(*bad) == 0, bad
    for f in (lib.litho_develop_rate_params_work_bytes, lib.litho_peb_expose_params_work_bytes):
        for bad in ((0, 5, 17, 1), (1, 0, 17, 1), (1, 33, 17, 1), (1, 5, 0, 1), (1, 5, 17, 0), (1, 5, 17, 65), (8192, 4, 17, 2)):
            assert f(*bad) == 0, bad


def param_argument_errors(nat):
    """Every refused call of the three new GPU entry points returns its code before the first HIP call; the pointers are never
    dereferenced.  Shared with the GPU suite.  Returns the number of refused calls."""
    lib = nat.lib()
    V = 4 * 4 * 64                                                             # bytes of a [1, 4, 8, 8] volume
    S, c = 8, 3
    W = lib.litho_peb_vjp_params_work_bytes(1, 4, 8, S, c)
    assert W == (2 * (math.ceil(S / c) - 1) + 4 * c + 8) * V + 4 * 48
    p = [ctypes.c_void_p(1 << 20 + i) for i in range(8)]                         # far apart: 1 MiB, 2 MiB, 4 MiB, ...
    nan, inf, E = float("nan"), float("inf"), nat.E_ARG
    near = lambda base, off: ctypes.c_void_p(base.value + off)                   # noqa: E731
    ok = dict(acid_in=p[0], B=1, D=4, n=8, thickness=100.0, pixel=25.0, q0=0.1, kq=5.0, kl=0.01, sh=20.0, sq=5.0, vs=1.0, t=60.0, steps=S, c=c,
              gh=p[1], gq=p[2], ga=p[3], out_h=p[4], out_q=p[5], out_s=p[7], work=p[6], wb=W)
    least = lib.litho_peb_min_steps(20.0, 5.0, 1.0, 100.0, 4, 25.0)
    bad = [dict(gh=None, gq=None, ga=None), dict(steps=least - 1, c=1), dict(steps=0, c=1), dict(steps=65537), dict(c=0), dict(c=S + 1),
           dict(B=0), dict(D=0), dict(D=33), dict(n=0), dict(n=16385), dict(B=16384),
           dict(acid_in=None), dict(out_h=None), dict(work=None), dict(work=near(p[6], 4)), dict(out_s=None),
           dict(out_s=near(p[7], 8)), dict(out_s=near(p[7], 4)),              # grad_step must be 16-byte aligned
           dict(thickness=0.0), dict(pixel=nan), dict(q0=-0.1), dict(kq=-1.0), dict(kq=nan), dict(kl=inf), dict(sh=-1.0), dict(vs=-1.0), dict(t=0.0),
           dict(out_h=p[0]), dict(out_h=p[1]), dict(out_q=p[3]), dict(out_q=p[4]), dict(out_h=near(p[6], W - 16)), dict(work=near(p[3], V - 16)),
           # grad_step over an input, a cotangent, an output, the workspace's volumes and its slots
           dict(out_s=p[0]), dict(out_s=near(p[0], V - 16)), dict(out_s=p[1]), dict(out_s=p[2]), dict(out_s=p[3]), dict(out_s=p[4]),
           dict(out_s=near(p[4], -32)), dict(out_s=p[5]), dict(out_s=p[6]), dict(out_s=near(p[6], W - 16)), dict(out_s=near(p[6], -32))]
    for kw in bad:
        assert lib.litho_peb_bake_vjp_params(*{**ok, **kw}.values(), None) == E, kw
    assert lib.litho_peb_bake_vjp_params(*{**ok, "wb": W - 1}.values(), None) == nat.E_WORKSPACE
    count = len(bad) + 1
    # litho_develop_rate_vjp_params(x, volumes, D, n, gains, n_gains, kappa, rmax, rmin, q, mth, r0, delta, thickness, grad_s, sums, work, wb, stream)
    g = (ctypes.c_float * 64)(*([1.0] * 64))
    gnan = (ctypes.c_float * 2)(1.0, nan)
    Wr = lib.litho_develop_rate_params_work_bytes(1, 4, 8, 2)
    assert Wr == 2 * 4 * 48
    ok = dict(x=p[0], volumes=1, D=4, n=8, gains=g, n_gains=2, kappa=0.05, rmax=120.0, rmin=0.05, q=5.0, mth=0.4, r0=1.0, delta=1.0, thick=100.0,
              gs=p[1], sums=p[2], work=p[3], wb=Wr)
    bad = [dict(x=None), dict(gs=None), dict(sums=None), dict(work=None), dict(gains=None), dict(n_gains=0), dict(n_gains=65), dict(gains=gnan),
           dict(volumes=0), dict(D=0), dict(D=33), dict(n=0), dict(n=16385), dict(volumes=8192), dict(kappa=0.0), dict(kappa=nan), dict(rmax=0.0),
           dict(rmin=-1.0), dict(q=1.0), dict(mth=1.0), dict(r0=0.0), dict(delta=0.0), dict(thick=0.0), dict(sums=near(p[2], 8)), dict(work=near(p[3], 8)),
           dict(sums=p[0]), dict(sums=near(p[0], V - 16)), dict(sums=p[1]), dict(sums=near(p[1], 2 * V - 16)), dict(sums=p[3]),
           dict(sums=near(p[3], Wr - 16)), dict(work=p[0]), dict(work=near(p[1], 2 * V - 16)), dict(work=near(p[2], -16))]
    for kw in bad:
        assert lib.litho_develop_rate_vjp_params(*{**ok, **kw}.values(), None) == E, kw
    assert lib.litho_develop_rate_vjp_params(*{**ok, "wb": Wr - 1}.values(), None) == nat.E_WORKSPACE
    count += len(bad) + 1
    # litho_peb_expose_vjp_params(image, volumes, D, n, gains, n_gains, C, grad_acid, grad_C, work, wb, stream)
    We = lib.litho_peb_expose_params_work_bytes(1, 4, 8, 2)
    assert We == 2 * 4 * 8
    ok = dict(image=p[0], volumes=1, D=4, n=8, gains=g, n_gains=2, C=0.05, ga=p[1], out=p[2], work=p[3], wb=We)
    bad = [dict(image=None), dict(ga=None), dict(out=None), dict(work=None), dict(gains=None), dict(n_gains=0), dict(n_gains=65), dict(gains=gnan),
           dict(volumes=0), dict(D=0), dict(D=33), dict(n=0), dict(n=16385), dict(volumes=8192), dict(C=0.0), dict(C=nan), dict(C=inf),
           dict(out=near(p[2], 8)), dict(work=near(p[3], 8)), dict(out=p[0]), dict(out=near(p[0], V - 16)), dict(out=p[1]),
           dict(out=near(p[1], 2 * V - 16)), dict(out=p[3]), dict(out=near(p[3], We - 16)), dict(work=p[0]), dict(work=near(p[1], 2 * V - 16)),
           dict(work=near(p[2], -16))]
    for kw in bad:
        assert lib.litho_peb_expose_vjp_params(*{**ok, **kw}.values(), None) == E, kw
    assert lib.litho_peb_expose_vjp_params(*{**ok, "wb": We - 1}.values(), None) == nat.E_WORKSPACE
    return count + len(bad) + 1


def test_argument_errors_come_back_before_any_gpu_call(nat):
    assert param_argument_errors(nat) > 100
