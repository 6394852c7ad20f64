"""Gradients with respect to the resist's parameters on the GPU (csrc/peb.hip: litho_peb_bake_vjp_params, litho_peb_expose_vjp_params;
csrc/develop_grad.hip: litho_develop_rate_vjp_params) through lithographysimulator_amd/calibrate.py, against the float64
restatement tests/resist_param_oracle.py (pinned to central differences in test_resist_param_cpu.py).

Bounds.
  grad_step     per volume and slot, |got - f64| <= C_PAR S 2^-24 M, M the oracle's sum of the absolute per-cell, per-step terms of
                that slot; a slot with M = 0 must be exactly 0.  Each term is a product of an adjoint quantity and a forward one,
                both carrying the fp32 sweeps' errors of order S 2^-24 of their scale (test_gpu_peb's and test_gpu_peb_grad's
                bounds); how much of that survives the sum over cells cannot be derived here, so C_PAR is MEASURED on an MI355X
                against the float64 oracle, fed the fp32 step parameters the library uses, and set to about four times the worst
                ratio, per class of resist (the worst over the slots, volumes, cotangent sets and S = 5, 7, 33 of every shape):
                    finite kQuench   measured 0.046 ... 3.98 of S 2^-24 M, C_PAR 16
                    instantaneous    measured 0.028 ... 0.76 of S 2^-24 M, C_PAR 3
                (per shape; the worst at n 1, D 1 and n 2, D 5, where a volume has 1 and 20 cells and nothing averages out -- the
                beta slot's factor fl hp + qb cancels while its error does not; from n 15 on both stay below 1, at n 48, D 17
                0.046 and 0.028.)
                Condition (not a measurement): C_PAR max(S) 2^-24 < 1e-3 -- a missing term or a wrong sign is wrong at 1e-1 M.
                The runs, the cotangents and the seed rule that keeps the fp32 and the float64 run of a mixed-branch
                instantaneous case on the same branch are test_gpu_peb_grad's (runs_of), imported.
  rate, exposure  per sum, |got - f64| <= (cells + C_FN) 2^-52 M: a double sum of `cells` terms in any order is within cells 2^-53 M
                of the exact one, twice for the two sides; C_FN covers the last-place differences of the device's exp, pow and
                log against numpy's, amplified by the exponents (q, kappa g x <= ~10) and by the cancellation in 1 - m.  Measured on an
                MI355X: 14.8 of 2^-52 M for the rate law's sums at n 1, D 1 (one cell per plane); at every larger shape, and for the
                exposure's sum at every shape, the error stays inside the summation's share.  C_FN = 64, about four times.
  chain         see test_the_parameter_gradient_equals_the_composition_of_the_oracles.
Shapes: test_gpu_peb's (n = 1, 2, 15, 16, 17, 24, 48; D = 1, 2, 5, 17, 32), B = 3 volumes, S = 5, 7, 33.  Every test prints what it
observed (-s)."""
import math

import numpy as np
import pytest
import torch

import develop_grad_oracle as DG
import peb_grad_oracle as GO
import peb_oracle as PO
import resist_param_oracle as RP
import test_gpu_develop_grad as TDG
import test_gpu_peb as TG
import test_gpu_peb_grad as PG
from test_resist_param_cpu import param_argument_errors

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 2.0 ** -52
C_PAR = {"finite": 16.0, "instant": 3.0}
C_FN = 64.0
H, THICK, BAKE, SHAPES, STEPS = TG.H, TG.THICK, TG.BAKE, TG.SHAPES, PG.STEPS
to_dev = PG.to_dev


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


def same64(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def test_the_bound_stays_below_the_cap():
    for kind, c in C_PAR.items():
        assert c * max(STEPS) * U < 1e-3, kind


# ---- 1. grad_step against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", SHAPES)
def test_step_gradient_against_the_oracle(L, dev, n, D):
    """All three cotangents together, and the acid dose's alone (what the chain from the arrival times hands over)."""
    worst = {"finite": 0.0, "instant": 0.0}
    failures = []
    for label, kind, r, S, h0, cots, floor in PG.runs_of(L, n, D):
        P, q0 = PG.parameters(r, D, S), float(np.float32(r.quencher))
        if floor is not None:
            margin = GO.branch_margin(GO.tape(h0, q0, S, **P)[0])
            assert margin >= floor, (label, S, margin, floor)
        (h0d,) = to_dev(dev, h0)
        for pick in ((0, 1, 2), (2,)):
            given = [c if i in pick else None for i, c in enumerate(cots)]
            want, mass, _, _ = RP.bake_param_vjp(h0.astype(np.float64), q0, S, *given, **P)
            gh0, gq0, got = L.bakeStepGradient(h0d, r, THICK, H, *to_dev(dev, *given), steps=S)
            assert got.dtype == torch.float64 and tuple(got.shape) == (3, 6)
            g = got.cpu().numpy()
            dead = mass == 0.0
            if not np.array_equal(g[dead], np.zeros(int(dead.sum()))):
                failures.append((label, S, pick, "a slot without terms is not exactly 0"))
            ratio = float((np.abs(g - want)[~dead] / (S * U * mass[~dead])).max(initial=0.0))
            worst[kind] = max(worst[kind], ratio)
            if not ratio <= C_PAR[kind]:
                failures.append((label, S, pick, ratio))
    print(f"step gradient n {n} D {D}: worst error / (S 2^-24 M) = {worst['finite']:.3f} (finite kQuench; C_PAR {C_PAR['finite']}) "
          f"{worst['instant']:.3f} (instantaneous; C_PAR {C_PAR['instant']})")
    assert not failures, failures


# ---- 2. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(2, 5), (17, 5), (48, 2)])
def test_the_bits_do_not_depend_on_the_checkpoints_the_batch_or_the_call(L, dev, n, D):
    """gradAcid0 and gradQuencher0 equal bakeGradient's; grad_step at checkpointEvery 1, 3, the default and S, for volume b alone
    and inside the batch, and in two calls: the same bit patterns."""
    from lithographysimulator_amd import peb
    h0, cots = PG.volumes(n, D, 3)
    h0d, gh, gq, ga = to_dev(dev, h0, *cots)
    for r in TG.resist_variants(L, D)[1:3]:                                     # both species diffuse; kQuench inf and finite
        base = {}
        for S in (7, 33):
            plain = peb.bakeGradient(h0d, r, THICK, H, gh, gq, ga, steps=S)
            base[S] = L.bakeStepGradient(h0d, r, THICK, H, gh, gq, ga, steps=S, checkpointEvery=1)
            assert TG.same_bits(base[S][:2], plain), f"S {S}: gradAcid0 / gradQuencher0 differ from bakeGradient's"
            for c in (3, None, S):
                again = L.bakeStepGradient(h0d, r, THICK, H, gh, gq, ga, steps=S, checkpointEvery=c)
                assert TG.same_bits(again[:2], plain) and same64(again[2], base[S][2]), f"S {S} c {c}"
            assert same64(L.bakeStepGradient(h0d, r, THICK, H, gh, gq, ga, steps=S)[2], base[S][2])
        for b in range(3):
            alone = L.bakeStepGradient(h0d[b:b + 1], r, THICK, H, gh[b:b + 1], gq[b:b + 1], ga[b:b + 1], steps=7)
            assert same64(alone[2], base[7][2][b:b + 1]), f"volume {b} alone"
            one = L.bakeStepGradient(h0d[b], r, THICK, H, gh[b], gq[b], ga[b], steps=7)
            assert tuple(one[2].shape) == (6,) and same64(one[2], alone[2][0]) and TG.same_bits(one[:2], [t[0] for t in alone[:2]])
    print(f"bit identity n {n} D {D}: bakeGradient's outputs; checkpointEvery 1, 3, default, S; batch and single volumes; two calls agree")


def test_exact_zero_slots(L, dev):
    """A species that does not diffuse, an instantaneous beta, and n = 1 laterally: exactly 0, as bit patterns of +0."""
    for n, D in ((1, 5), (17, 5)):
        h0, cots = PG.volumes(n, D, 1)
        h0d, gh, gq, ga = to_dev(dev, h0, *cots)
        for ri, r in enumerate(TG.resist_variants(L, D)):
            g = L.bakeStepGradient(h0d, r, THICK, H, gh, gq, ga, steps=7)[2].cpu()
            zero = set()
            if r.acidDiffusionLength == 0.0:
                zero |= {0, 1}
            if r.quencherDiffusionLength == 0.0:
                zero |= {2, 3}
            if math.isinf(r.kQuench):
                zero.add(4)
            if n == 1:
                zero |= {0, 2}
            for slot in range(6):
                if slot in zero:
                    assert bool((g[:, slot].view(torch.int64) == 0).all()), (n, D, ri, slot, g[:, slot])
                else:
                    assert bool((g[:, slot] != 0).all()), (n, D, ri, slot)
    print("exact zeros: non-diffusing species, instantaneous beta, n = 1 lateral")


def test_the_bake_parameters_are_the_chain_of_the_step_gradient(L, dev):
    n, D, S = 17, 5, 7
    h0, cots = PG.volumes(n, D, 2)
    h0d, gh, gq, ga = to_dev(dev, h0, *cots)
    for r in TG.resist_variants(L, D):
        gh0, gq0, gs = L.bakeStepGradient(h0d, r, THICK, H, gh, gq, ga, steps=S)
        a, b, params = L.bakeParameterGradient(h0d, r, THICK, H, gh, gq, ga, steps=S)
        assert TG.same_bits((a, b), (gh0, gq0)) and set(params) == {"quencher", "kQuench", "kLoss", "acidDiffusionLength",
                                                                   "quencherDiffusionLength", "verticalScale"}
        want = RP.param_chain(THICK, H, r.kQuench, r.kLoss, r.acidDiffusionLength, r.quencherDiffusionLength, r.verticalScale, r.bakeTime, D, S,
                              gs.cpu().numpy())
        scale = np.abs(RP.param_chain(THICK, H, r.kQuench, r.kLoss, r.acidDiffusionLength, r.quencherDiffusionLength, r.verticalScale,
                                      r.bakeTime, D, S, np.abs(gs.cpu().numpy())))
        for i, name in enumerate(RP.PHYSICAL):
            got = params[name].numpy()
            assert got.dtype == np.float64 and got.shape == (3,) and (np.abs(got - want[:, i]) <= 8 * EPS * scale[:, i] + 1e-300).all(), name
        q = gq0.double().sum(dim=(1, 2, 3)).cpu().numpy()
        assert np.array_equal(params["quencher"].numpy(), q)


# ---- 3. the rate law's and the exposure's sums -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(1, 1), (15, 2), (16, 5), (17, 17), (24, 32), (48, 2)])
def test_rate_and_exposure_sums_against_the_oracle(L, dev, n, D):
    from lithographysimulator_amd import calibrate
    rng = np.random.default_rng(n + D)
    I = rng.uniform(0.0, 3.0, (2, D, n, n)).astype(np.float32)
    I.flat[0] = 0.0                                                            # unexposed: b = 0
    doses = (0.6, 1.0, 1.7)
    gs = rng.standard_normal((6, D, n, n)).astype(np.float32)
    if n > 1:
        I[1, 0, 1, 2], I[0, D - 1, n - 1, n - 1] = -0.5, np.nan                  # walls, the cotangent of one of them NaN
        gs[1::2, 0, 1, 2] = np.nan
    Id, gsd = to_dev(dev, I, gs)
    cells = n * n
    worst_rate = worst_exp = 0.0
    for r0, delta in ((1.0, None), (0.25, 30.0)):
        resist = L.MackResist(C=0.9, rMax=120.0, rMin=0.05, q=5.0, mTh=0.4, surfaceRate=r0, surfaceDepth=delta)
        got = calibrate._rate_sums("test", Id, doses, 0.9, resist, THICK, gsd)
        assert got.dtype == torch.float64 and tuple(got.shape) == (6, D, 6)
        want, mass = RP.rate_param_sums(I, doses, 0.9, 120.0, 0.05, 5.0, 0.4, THICK, r0, delta if delta else 1.0, gs)
        g = got.cpu().numpy()
        assert np.isfinite(g).all()                                            # the walls contributed 0
        ratio = float((np.abs(g - want) / (EPS * np.where(mass > 0, mass, 1.0))).max())
        worst_rate = max(worst_rate, ratio - cells)
        assert (np.abs(g - want) <= (cells + C_FN) * EPS * mass).all(), ratio
        again = calibrate._rate_sums("test", Id, doses, 0.9, resist, THICK, gsd)
        alone = calibrate._rate_sums("test", Id[1:], doses, 0.9, resist, THICK, gsd[1::2].contiguous())
        assert same64(again, got) and same64(alone, got[1::2].contiguous())
        table = L.rateParameterGradient(Id, resist, THICK, gsd, doses)
        chain = RP.rate_param_chain(g, 120.0, 0.05, 5.0, 0.4, THICK, r0, delta if delta else 1.0)
        assert set(table) == ({"C", "rMax", "rMin", "q", "mTh"} | ({"surfaceRate", "surfaceDepth"} if delta else set()))
        for i, name in enumerate(("C", "rMax", "rMin", "q", "mTh", "surfaceRate", "surfaceDepth")):
            if name in table:
                assert np.allclose(table[name].numpy(), chain[:, i], rtol=1e-12, atol=1e-12 * np.abs(chain[:, i]).max()), name
    # the amplified resist: kappa = kAmp, x = the acid dose, a single gain of 1
    r = TG.resist_variants(L, D)[0]
    a = (I * 20.0).astype(np.float32)
    (ad,) = to_dev(dev, a)
    m = r.mack
    got = calibrate._rate_sums("test", ad, (1.0,), r.kAmp, m, THICK, gsd[:2].contiguous()).cpu().numpy()
    want, mass = RP.rate_param_sums(a, (1.0,), r.kAmp, m.rMax, m.rMin, m.q, m.mTh, THICK, 1.0, 1.0, gs[:2])
    worst_rate = max(worst_rate, float((np.abs(got - want) / (EPS * np.where(mass > 0, mass, 1.0))).max()) - cells)
    assert (np.abs(got - want) <= (cells + C_FN) * EPS * mass).all()
    table = L.rateParameterGradient(ad, r, THICK, gsd[:2].contiguous())
    assert set(table) == {"kAmp", "rMax", "rMin", "q", "mTh"} and all(v.shape == (2,) for v in table.values())
    # the exposure
    got = L.exposureParameterGradient(Id, 0.9, doses, gsd)
    want, mass = RP.expose_param_sums(I, doses, 0.9, gs)
    assert got.dtype == torch.float64 and tuple(got.shape) == (6,) and bool(torch.isfinite(got).all())
    cells_v = cells * D
    worst_exp = float((np.abs(got.numpy() - want) / (EPS * np.where(mass > 0, mass, 1.0))).max()) - cells_v
    assert (np.abs(got.numpy() - want) <= (cells_v + C_FN) * EPS * mass).all()
    alone = L.exposureParameterGradient(Id[1], 0.9, doses, gsd[1::2].contiguous())
    assert np.array_equal(alone.numpy(), got.numpy()[1::2])
    print(f"parameter sums n {n} D {D}: error beyond the summation's share, in units of 2^-52 M: rate {max(worst_rate, 0.0):.1f}, "
          f"exposure {max(worst_exp, 0.0):.1f} (C_FN {C_FN})")


# ---- 4. the chain ----------------------------------------------------------------------------------------------------------------
def structure(h0, q0, S, lam_h, lam_q, beta, fl, half_dt):
    """Per slot, the sum over steps and cells of the absolute factor that multiplies the adjoint quantity in the slot's term:
    |Laplacians|, 2 hd qd / Dn^2 (|fl hp + qb| <= 2 G), |hd - R|.  An error of at most e on every adjoint quantity moves the
    slot by at most e times this."""
    h = np.asarray(h0, dtype=np.float64)
    q = np.full(h.shape, float(q0))
    a = np.zeros(h.shape)
    out = np.zeros(6)
    for _ in range(S):
        hd, qd = PO.diffuse_step(h, lam_h), PO.diffuse_step(q, lam_q)
        if lam_h is not None:
            out[0:2] += [np.abs(x).sum() for x in RP.laplacians(h)]
        if lam_q is not None:
            out[2:4] += [np.abs(x).sum() for x in RP.laplacians(q)]
        Dn = 1.0 + beta * (hd + qd)
        out[4] += float((2.0 * hd * qd / (Dn * Dn)).sum())
        out[5] += float(np.abs(hd - beta * hd * qd / Dn).sum())
        h, q, a = PO.bake_step(h, q, a, lam_h, lam_q, beta, fl, half_dt)
    return out


@pytest.mark.parametrize("n,D", [(17, 4), (32, 2)])
def test_the_parameter_gradient_equals_the_composition_of_the_oracles(L, dev, n, D):
    """resistParameterGradient for a chemically amplified resist, two doses, and for a MackResist with two doses and two focal
    planes, the pattern of test_the_profile_gradient_equals_the_composition_of_the_oracles: the oracles are composed from the
    device's own slowness and T.  Stage bounds, summed through the chains' coefficients:
      rate      the solver's error on gradSlowness, at most TOL_CHAIN_TIME max |gradSlowness| per cell, times the sum over the
                cells of the slot's |ds/d.| (the oracle's M for a cotangent of ones), plus the kernel's own (cells + C_FN) 2^-52 M;
      bake      abar carries e_a per cell (the solver's error through |ds/dx|, the fp32 rounding of the rate's vjp); the adjoint
                quantities then move by at most bakeTime e_a (the header's convex-combination bound), times structure(); plus
                the kernel's own C_PAR S 2^-24 M;
      quencher  every qbar_0 within C_GRAD S 2^-24 G + bakeTime e_a;
      C         hbar_0 within the same per cell, times the sum of |d h0 / dC|, plus the exposure kernel's own."""
    from lithographysimulator_amd import peb
    pixel, thick, doses, F = 10.0, 80.0, (0.8, 1.0), 2
    I = (TG.line_space(n, D, 16)[None] * np.array([1.0, 0.7], dtype=np.float32)[:, None, None, None]).astype(np.float32)
    (Id,) = to_dev(dev, I)
    rng = np.random.default_rng(n + D)
    gT = rng.standard_normal((2, F, D, n, n)).astype(np.float32)
    (gTd,) = to_dev(dev, gT)
    cells = n * n
    tol_t = TDG.TOL_CHAIN_TIME
    # -- chemically amplified resist, one focal plane
    r = PG.chain_resist(L)
    got = L.resistParameterGradient(Id[0], r, thick, pixel, gTd[:, :1].contiguous(), doses=doses)
    bake = L.postExposureBake(Id[:1], r, thick, pixel, doses)
    S = bake.steps
    T = L.developmentTime(bake.slowness, thick, pixel)
    gs = TDG.oracle_time_vjp(T.cpu().numpy(), bake.slowness.cpu().numpy(), gT[:, 0], thick, pixel)
    a = bake.acidDose.cpu().numpy()
    m = r.mack
    mp = (r.kAmp, m.rMax, m.rMin, m.q, m.mTh, thick, 1.0, 1.0)
    e_s = tol_t * float(np.abs(gs).max())
    sums, mass = RP.rate_param_sums(a, (1.0,), *mp, gs)
    _, slope = RP.rate_param_sums(a, (1.0,), *mp, np.ones_like(gs))
    want = dict(zip(("kAmp", "rMax", "rMin", "q", "mTh"), RP.rate_param_chain(sums, *mp[1:5], thick, 1.0, 1.0).sum(axis=0)))
    slot_bound = e_s * slope + (cells + C_FN) * EPS * mass
    bound = dict(zip(("kAmp", "rMax", "rMin", "q", "mTh"), np.abs(RP.rate_param_chain(slot_bound, *mp[1:5], thick, 1.0, 1.0)).sum(axis=0)))
    da_dq = DG.DO.mack_a(m.q, m.mTh) * (1 / (m.q + 1) - 1 / (m.q - 1) + math.log(1 - m.mTh))
    bound["q"] = float((slot_bound[:, :, 3] + slot_bound[:, :, 4] * abs(da_dq)).sum())
    ga = DG.rate_vjp(a, [1.0], *mp, gs)
    e_a = float((e_s * np.abs(DG.rate_vjp(a, [1.0], *mp, np.ones_like(gs))) + 2.0 ** -22 * np.abs(ga)).max())
    h0 = peb.exposeAcid(Id[:1], r.C, doses).cpu().numpy().astype(np.float64)
    P = PO.step_parameters(r.kQuench, r.kLoss, r.acidDiffusionLength, r.quencherDiffusionLength, r.verticalScale, r.bakeTime, thick, D, pixel, S)
    q0 = float(np.float32(r.quencher))
    gstep, gmass, hb, qb = RP.bake_param_vjp(h0, q0, S, None, None, ga, **P)
    phys = (thick, pixel, r.kQuench, r.kLoss, r.acidDiffusionLength, r.quencherDiffusionLength, r.verticalScale, r.bakeTime, D, S)
    want.update(zip(RP.PHYSICAL, RP.param_chain(*phys, gstep).sum(axis=0)))
    e_adj = r.bakeTime * e_a
    step_bound = C_PAR["finite"] * S * U * gmass + e_adj * np.stack([structure(h0[b:b + 1], q0, S, **P) for b in range(2)])
    bound.update(zip(RP.PHYSICAL, np.abs(RP.param_chain(*phys, step_bound)).sum(axis=0)))     # no chain coefficient mixes signs
    G = GO.bound_scale(None, None, ga, r.bakeTime)
    per_cell = PG.C_GRAD["finite"] * S * U * G + e_adj
    want["quencher"], bound["quencher"] = float(qb.sum()), per_cell * qb.size
    csum, cmass = RP.expose_param_sums(I[:1].astype(np.float64), doses, r.C, hb)
    _, cslope = RP.expose_param_sums(I[:1].astype(np.float64), doses, r.C, np.ones_like(hb))
    want["C"], bound["C"] = float(csum.sum()), float((per_cell * cslope + (cells * D + C_FN) * EPS * cmass).sum())
    assert set(got) == set(want), (sorted(got), sorted(want))
    for name in sorted(want):
        err = abs(got[name] - want[name])
        print(f"chain (amplified) n {n} D {D} S {S} {name}: got {got[name]:+.9e} oracle {want[name]:+.9e} error {err:.2e} = "
              f"{err / bound[name]:.3f} of its bound {bound[name]:.2e}")
        assert err <= bound[name], name
    # the bounds are loose (bakeTime e_a on every adjoint quantity) but still tell a result from a wrong one: a missing stage or
    # a wrong sign is wrong at 1
    assert all(bound[k] < 1e-1 * abs(want[k]) for k in ("kAmp", "rMax", "C", "acidDiffusionLength", "kLoss"))
    # -- Mack resist with diffusion and the surface factor, two focal planes
    resist = L.MackResist(C=2.0, rMax=100.0, rMin=0.05, q=4.0, mTh=0.5, surfaceRate=0.5, surfaceDepth=20.0, diffusionLength=15.0,
                          verticalDiffusionLength=12.0)
    got = L.resistParameterGradient(Id.reshape(F * D, n, n), resist, thick, pixel, gTd, doses=doses, focalPlanes=F)
    s = L.developmentRate(Id, resist, thick, pixel, doses)
    T = L.developmentTime(s, thick, pixel)
    gs = TDG.oracle_time_vjp(T.cpu().numpy(), s.cpu().numpy(), gT.reshape(2 * F, D, n, n), thick, pixel)
    lat = L.latentDiffusion(Id, thick, pixel, 15.0, 12.0).cpu().numpy()        # the rate law's own input, the device's bits
    par = (2.0, 100.0, 0.05, 4.0, 0.5, thick, 0.5, 20.0)
    sums, mass = RP.rate_param_sums(lat, doses, *par, gs)
    _, slope = RP.rate_param_sums(lat, doses, *par, np.ones_like(gs))
    names = ("C", "rMax", "rMin", "q", "mTh", "surfaceRate", "surfaceDepth")
    want = dict(zip(names, RP.rate_param_chain(sums, *par[1:5], thick, 0.5, 20.0).sum(axis=0)))
    slot_bound = tol_t * float(np.abs(gs).max()) * slope + (cells + C_FN) * EPS * mass
    bound = dict(zip(names, np.abs(RP.rate_param_chain(slot_bound, *par[1:5], thick, 0.5, 20.0)).sum(axis=0)))
    da_dq = DG.DO.mack_a(4.0, 0.5) * (1 / 5.0 - 1 / 3.0 + math.log(0.5))
    bound["q"] = float((slot_bound[:, :, 3] + slot_bound[:, :, 4] * abs(da_dq)).sum())
    assert set(got) == set(want)
    for name in names:
        err = abs(got[name] - want[name])
        print(f"chain (Mack) n {n} D {D} {name}: got {got[name]:+.9e} oracle {want[name]:+.9e} error {err:.2e} = "
              f"{err / bound[name]:.3f} of its bound {bound[name]:.2e}")
        assert err <= bound[name], name


# ---- 5. calibration --------------------------------------------------------------------------------------------------------------
def test_calibration_recovers_two_parameters(L, dev):
    """n = 32, D = 4, two doses: CDs of a known resist on a line-space pattern, the fit started with kAmp and acidDiffusionLength
    off by 20 %.  The loss of the known resist on its own CDs is 0 (to rounding).  Every accepted step lowers the loss, the
    final loss is below the initial one, and both parameters end nearer the truth than they started: from (x 1.2, x 1.2) in 20
    iterations, from (x 1.2, x 0.8) -- where the two errors nearly compensate in the CDs and the descent has to walk along the
    valley -- in 40.  From (x 0.8, x 0.8) nothing develops within 2 developTime at any measured edge: the clamped loss is 1 with
    a zero gradient, and the fit returns its starting point after one evaluation (a property of the loss, stated, not hidden)."""
    from lithographysimulator_amd import calibrate
    n, D, pixel, thick, doses, t = 32, 4, 10.0, 80.0, (0.8, 1.0), 20.0
    truth = PG.chain_resist(L)
    I = torch.from_numpy(TG.line_space(n, D, 16)).to(dev)
    S = max(8, 2 * truth.minSteps(thick, D, pixel))
    T = L.resistArrivalTimes(I, truth, thick, pixel, doses, 1, S)
    prof = L.ResistProfile(T, None, 0, thick, pixel, t, doses)
    gauge = (n // 2, n // 2, 0)                                                # the bright space in the middle, along its row
    cds = prof.cd([gauge]).cpu().numpy()[:, :, 0]                              # [doses, D, 5]
    measurements = [(di, 0, d, (n // 2, 0.5 * float(cds[di, d, 1] + cds[di, d, 2]), 0), float(cds[di, d, 0]))
                    for di in range(2) for d in range(D) if cds[di, d, 0] > 0 and 0 < cds[di, d, 1] and cds[di, d, 2] < n - 1]
    print(f"calibration: {len(measurements)} CDs of the known resist, " + " ".join(f"{m[4]:.2f}" for m in measurements) + " nm")
    assert len(measurements) >= 4
    at_truth = calibrate._edge_loss(T.reshape(2, D, n, n), t, *calibrate._edge_points("test", measurements, 2, 1, D, n, pixel, dev))[0]
    assert at_truth < 1e-8, at_truth
    for fk, fa, iterations in ((1.2, 1.2, 20), (1.2, 0.8, 40)):
        start = L.resistWith(truth, kAmp=fk * truth.kAmp, acidDiffusionLength=fa * truth.acidDiffusionLength)
        fitted, history = L.calibrateResist(I, start, thick, pixel, t, measurements, parameters=("kAmp", "acidDiffusionLength"), doses=doses,
                                            iterations=iterations, steps=S)
        best = None
        for rec in history:
            if rec["accepted"]:
                assert best is None or rec["loss"] < best
                best = rec["loss"]
        print(f"calibration from (x {fk}, x {fa}), {iterations} iterations, {sum(h['accepted'] for h in history)} accepted: loss "
              f"{history[0]['loss']:.3e} -> {best:.3e}; kAmp {start.kAmp:.5f} -> {fitted.kAmp:.5f} (truth {truth.kAmp}); "
              f"acidDiffusionLength {start.acidDiffusionLength:.3f} -> {fitted.acidDiffusionLength:.3f} (truth {truth.acidDiffusionLength})")
        assert len(history) == iterations + 1 and history[0]["accepted"] and best < history[0]["loss"]
        for name in ("kAmp", "acidDiffusionLength"):
            assert abs(getattr(fitted, name) - getattr(truth, name)) < abs(getattr(start, name) - getattr(truth, name)), name
        assert fitted.kQuench == truth.kQuench and fitted.mack.rMax == truth.mack.rMax          # what was not fitted stays
    dark = L.resistWith(truth, kAmp=0.8 * truth.kAmp, acidDiffusionLength=0.8 * truth.acidDiffusionLength)
    fitted, history = L.calibrateResist(I, dark, thick, pixel, t, measurements, parameters=("kAmp", "acidDiffusionLength"), doses=doses,
                                        iterations=5, steps=S)
    assert len(history) == 1 and history[0]["loss"] == 1.0 and fitted.kAmp == dark.kAmp


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_argument_errors(L, dev):
    from lithographysimulator_amd import _native as nat
    assert param_argument_errors(nat) > 100                                    # every code of the C ABI, before any launch
    r = PG.chain_resist(L)
    inst = PG.with_quencher(L, TG.resist_variants(L, 4)[1], 0.3)
    I = torch.rand((4, 8, 8), device=dev)
    meas = [(0, 0, 0, (4, 4, 0), 30.0)]
    for resist, names in ((r, ("bakeTime",)), (r, ("surfaceRate",)), (inst, ("kQuench",)), (TG.mack(L), ("kAmp",)), (r, ())):
        with pytest.raises(ValueError):
            L.calibrateResist(I, resist, 80.0, 10.0, 20.0, meas, parameters=names)
    with pytest.raises(ValueError):
        L.calibrateResist(I, r, 80.0, 10.0, 20.0, [(0, 0, 9, (4, 4, 0), 30.0)])
    with pytest.raises(TypeError):
        L.bakeStepGradient(torch.rand((2, 4, 8, 8), device=dev), TG.mack(L), 80.0, 10.0, gradAcid=torch.rand((2, 4, 8, 8), device=dev))
    with pytest.raises(ValueError):
        L.bakeStepGradient(torch.rand((2, 4, 8, 8), device=dev), r, 80.0, 10.0)
