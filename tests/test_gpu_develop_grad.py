"""Gradients through development on the GPU (csrc/develop_grad.hip: litho_develop_time_vjp, litho_develop_rate_vjp) through
lithographysimulator_amd/develop.py, peb.amplifiedRateGradient and ilt.developedResistModel, against the float64 restatement
tests/develop_grad_oracle.py (pinned to central differences in test_develop_grad_cpu.py).

The oracle is evaluated on the device's own fp32 T and slowness with h = fp32(pixel), hz = fp32(thickness / D), so the branch, tie
and strict-upwind decisions are the same comparisons on the same numbers.

Bounds.
  solver   max |grad - f64| <= TOL_TIME[(n, D)] max |grad| per volume.  lambda is a sum along dependency paths, each term one fp32
           product and one addition, so the error grows with the path length and cannot be derived tighter than that; it is
           MEASURED: the constant is 4 x the larger of the device's error and of the CPU fp32 emulation's error
           (develop_grad_oracle.gather_fp32) for the same volumes, the margin for the seed-to-seed scatter of such a sum.  The
           numbers are beside the constants.  An error above 2e-6 at these shapes is a finding to explain, not a tolerance to
           widen: every constant stays below that (asserted).
  uniform  closed form, see the test.
  serpentine  one dependency path through the whole channel, a running fp32 sum of positive terms: per cell of the channel at most
           three products and three additions, 6 (cells of the channel) 2^-24 of the largest value.
  rate     relative 1e-6 of the largest value: double per cell, rounded once (2^-24), a last-place difference of the device's exp and
           pow amplified by the exponents (q, kappa g x <= ~10): the argument of test_rate_against_the_oracle.
  chain    see test_the_profile_gradient_equals_the_composition_of_the_oracles.
Shapes (n, D): (1, 1) the smallest volume; (15, 2) a partial tile; (17, 5) a one-cell second tile, halo traffic both ways; (33, 3)
an interior tile with four neighbours; (48, 17) an odd D; (24, 32) the dynamic-LDS path above 64 KiB.  n % 4 != 0 takes the scalar path of the pointwise kernels, n % 4 == 0 the 16-byte one.
Every test prints what it observed (-s)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import develop_grad_oracle as GO
import develop_oracle as DO
import resist_oracle as RO
import socs_grad_oracle as SG
import test_gpu_develop as TD
import test_gpu_peb as TG
from test_develop_grad_cpu import develop_vjp_argument_errors

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
H, THICK = 25.0, 100.0
SHAPES = [(1, 1), (15, 2), (17, 5), (33, 3), (48, 17), (24, 32)]
# (n, D): 4 x max(device, emulation), both relative to max |grad| per volume, the worst of the B = 3 volumes.  Measured on an MI355X;
# the device's result equalled the emulation's bit for bit at every shape, so the two columns are one:
#   (1, 1)    4.27e-08  (the one rounding of sigma)      (33, 3)   1.86e-07
#   (15, 2)   1.16e-07                                   (48, 17)  2.72e-07
#   (17, 5)   1.56e-07                                   (24, 32)  3.04e-07
TOL_TIME = {(1, 1): 4 * 4.28e-8, (15, 2): 4 * 1.16e-7, (17, 5): 4 * 1.57e-7, (33, 3): 4 * 1.86e-7, (48, 17): 4 * 2.72e-7,
            (24, 32): 4 * 3.04e-7}


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


def f32(v):
    return float(np.float32(v))


def inputs(n, D):
    """B = 3 volumes: slowness log-uniform over three decades (the forward test's) and a standard normal cotangent, fp32."""
    rng = np.random.default_rng(7000 * n + D)
    s = (10.0 ** rng.uniform(-3.0, 0.0, (3, D, n, n))).astype(np.float32)
    return s, rng.standard_normal((3, D, n, n)).astype(np.float32)


def oracle_time_vjp(T, s, g, thickness=THICK, h=H):
    """float64 from the device's fp32 T and s, with the geometry as the library rounds it."""
    D = T.shape[-3]
    return GO.time_vjp(T.astype(np.float64), s.astype(np.float64), g.astype(np.float64), thickness, f32(h), f32(thickness / D))


_random = {}


def random_case(L, dev, n, D):
    if (n, D) not in _random:
        s, g = inputs(n, D)
        sd, gd = torch.from_numpy(s).to(dev), torch.from_numpy(g).to(dev)
        T = L.developmentTime(sd, THICK, H)
        grad, launches = L.developmentTimeGradient(sd, T, gd, THICK, H, returnLaunches=True)
        _random[(n, D)] = (s, g, sd, gd, T, grad, launches)
    return _random[(n, D)]


def per_volume_error(got, want):
    """max over the volumes of max |got - want| / max |want|."""
    B = want.shape[0]
    e = np.abs(got.astype(np.float64) - want).reshape(B, -1).max(axis=1)
    return float((e / np.abs(want).reshape(B, -1).max(axis=1)).max())


def test_the_constants_stay_below_the_finding_threshold():
    assert set(TOL_TIME) == set(SHAPES) and all(v <= 2e-6 for v in TOL_TIME.values())


# ---- 5. the solver against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", SHAPES)
def test_time_gradient_against_the_oracle(L, dev, n, D):
    s, g, _, _, T, grad, launches = random_case(L, dev, n, D)
    T_h = T.cpu().numpy()
    assert np.isfinite(T_h).all()
    want = oracle_time_vjp(T_h, s, g)
    got = grad.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == s.shape and np.isfinite(got).all()
    err = per_volume_error(got, want)
    L64, sig = GO.links(T_h.astype(np.float64), s.astype(np.float64), f32(H), f32(THICK / D))
    emu, sweeps = GO.gather_fp32(L64, sig, g)
    emu_err = per_volume_error(emu, want)
    same = bool(np.array_equal(emu.view(np.uint32), got.view(np.uint32)))
    print(f"time vjp n {n} D {D}: {launches} launches (emulation {sweeps} Jacobi sweeps); error / max |grad|: device {err:.3e}, "
          f"emulation {emu_err:.3e}, bound {TOL_TIME[(n, D)]:.2e}; device == emulation bit for bit: {same}")
    assert err <= TOL_TIME[(n, D)]


# ---- 6. bit identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(17, 5), (48, 2), (24, 32)])
def test_second_call_batch_and_batch_index_are_bit_identical(L, dev, n, D):
    _, _, sd, gd, T, grad, launches = random_case(L, dev, n, D)
    again, l2 = L.developmentTimeGradient(sd, T, gd, THICK, H, returnLaunches=True)
    assert TD.same_bits(again, grad) and l2 == launches                         # int32 views: NaN and -0 compare as bits
    singles = [L.developmentTimeGradient(sd[b], T[b], gd[b], THICK, H, returnLaunches=True) for b in range(3)]
    assert all(tuple(t.shape) == (D, n, n) and TD.same_bits(t, grad[b]) for b, (t, _) in enumerate(singles))
    assert max(l for _, l in singles) == launches
    order = [1, 2, 0]                                                           # volume 0 at batch index 2
    moved = L.developmentTimeGradient(sd[order].contiguous(), T[order].contiguous(), gd[order].contiguous(), THICK, H)
    assert TD.same_bits(moved[2], grad[0]) and TD.same_bits(moved[0], grad[1])
    print(f"n {n} D {D}: second call, 3 single calls and a permuted batch equal the batch bit for bit; launches {launches} vs "
          f"{[l for _, l in singles]}")


# ---- 7. structured cases ---------------------------------------------------------------------------------------------------------
def test_slot_gradient_runs_along_the_upwind_path(L, dev):
    """The forward tests' slot across three tiles.  A cotangent of 1 on one cell of plane 1, 37 columns from the slot: its arrival
    time is the sum of the step lengths times the slownesses along the one upwind path -- along its row to the slot, up the slot
    to the top -- so the gradient is h on the row's cells outside the slot, hz on the slot's cell in plane 1, hz / 2 on the one in
    plane 0, and exactly 0 everywhere else."""
    n, col = TD.SLOT["n"], TD.SLOT["col"]
    s = TD._slot_volume()
    sd = torch.from_numpy(s).to(dev)
    T = L.developmentTime(sd, THICK, H)
    row, at = 20, 40
    g = np.zeros_like(s)
    g[1, row, at] = 1.0
    grad, launches = L.developmentTimeGradient(sd, T, torch.from_numpy(g).to(dev), THICK, H, returnLaunches=True)
    got = grad.cpu().numpy().astype(np.float64)
    want = np.zeros(s.shape)
    want[1, row, col + 1:at + 1] = H
    want[1, row, col] = THICK / 2
    want[0, row, col] = THICK / 4
    oracle = oracle_time_vjp(T.cpu().numpy(), s, g)
    e1, e2 = float(np.abs(got - want).max()), float(np.abs(got - oracle).max())
    print(f"slot: {launches} launches; {int((got != 0).sum())} non-zero cells (path {int((want != 0).sum())}); max error {e1:.2e} from "
          f"the closed form, {e2:.2e} from the oracle")
    assert np.array_equal(got != 0, want != 0)
    # 39 links of weight 1 up to rounding; against the closed form also: where the stored T_i - T_upwind came out an ulp below
    # h s the update is the two-axis branch with a weight of up to ulp(T) / (h s) on the y axis, whose neighbours tie with the cell
    # and are dropped -- the x weight lacks it, once per cell of the path
    lost = (at - col) * (2.0 ** -23 * float(T.max()) / (H * float(s[1, 0, 0]))) * H
    assert e2 <= 64 * U * THICK and e1 <= 64 * U * THICK + lost
    assert launches >= 3                                                        # one tile per launch at the least


def test_serpentine_converges_late_and_the_launch_cap_raises(L, dev):
    n = 48
    s = TD._serpentine(n)
    sd = torch.from_numpy(s).to(dev)
    T = L.developmentTime(sd, 50.0, H)
    T_h = T.cpu().numpy()
    fin = np.isfinite(T_h)
    g = np.where(fin, 1.0, np.nan).astype(np.float32)                           # NaN where the developer never arrives: ignored
    gd = torch.from_numpy(g).to(dev)
    grad, launches = L.developmentTimeGradient(sd, T, gd, 50.0, H, returnLaunches=True)
    got = grad.cpu().numpy()
    want = oracle_time_vjp(T_h, s, np.where(fin, 1.0, 0.0), 50.0, H)
    assert np.isfinite(got).all() and (got[~fin] == 0).all()
    err = float(np.abs(got - want).max() / np.abs(want).max())
    channel = int((s[1] == np.float32(0.01)).sum())
    print(f"serpentine: {launches} launches, channel of {channel} cells, max error / max |grad| = {err:.2e} (bound {6 * channel * U:.2e})")
    assert launches > 3 and err <= 6 * channel * U
    with pytest.raises(RuntimeError, match="fixed point"):
        L.developmentTimeGradient(sd, T, gd, 50.0, H, maxIterations=2)
    torch.cuda.synchronize()
    g2, l2 = L.developmentTimeGradient(sd, T, gd, 50.0, H, maxIterations=launches, returnLaunches=True)
    assert torch.equal(g2, grad) and l2 == launches
    with pytest.raises(RuntimeError, match="fixed point"):
        L.developmentTimeGradient(sd, T, gd, 50.0, H, maxIterations=launches - 1)


def test_closed_box_of_walls(L, dev):
    n, D = 24, 5
    rng = np.random.default_rng(5)
    s = (10.0 ** rng.uniform(-2.0, 0.0, (D, n, n))).astype(np.float32)
    lo, hi = 6, 19                                                             # the box straddles the tile seam at 16
    s[:, lo, lo:hi + 1] = s[:, hi, lo:hi + 1] = s[:, lo:hi + 1, lo] = s[:, lo:hi + 1, hi] = np.nan
    s[0, lo:hi + 1, lo:hi + 1] = np.nan
    s[2, 0, 0], s[3, 1, 1], s[1, 2, 2] = 0.0, -1.0, np.inf
    sd = torch.from_numpy(s).to(dev)
    T = L.developmentTime(sd, THICK, H)
    T_h = T.cpu().numpy()
    g = rng.standard_normal(s.shape).astype(np.float32)
    g[2, 10, 10], g[3, 15, 16], g[1, lo, lo], g[2, 0, 0] = np.nan, np.inf, np.nan, -np.inf    # inside the box and on walls
    grad, launches = L.developmentTimeGradient(sd, T, torch.from_numpy(g).to(dev), THICK, H, returnLaunches=True)
    got = grad.cpu().numpy()
    unreached = ~np.isfinite(T_h)
    assert unreached[1:, lo + 1:hi, lo + 1:hi].all()
    assert np.isfinite(got).all() and (got[unreached] == 0).all()
    want = oracle_time_vjp(T_h, s, np.where(unreached, 0.0, g))
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"closed box: {launches} launches, {int(unreached.sum())} cells without a gradient, max error / max |grad| = {err:.2e}")
    assert err <= 2e-6


def test_uniform_slowness_closed_form(L, dev):
    """T = s z: every cell hangs on the cell above it with weight 1, so dl/ds of a cell is the sum of g from it to the bottom of
    its column times its step length (hz / 2 on plane 0, hz below).  Rounding: the running fp32 sum, D 2^-24; where the stored
    T_d - T_(d-1) came out an ulp below hz s the update is the two-axis branch with a lateral weight of about (hz / h)^2 (d + 1)
    2^-24 that the strict-upwind rule drops (the lateral neighbours tie), which the z weight then lacks: summed down a column at
    most (hz / h)^2 D^2 2^-24.  Bound (2 D + (hz / h)^2 D^2) 2^-24 of the largest value."""
    n, D = 17, 5
    hz = THICK / D
    s = torch.full((D, n, n), 1.0 / 0.8, dtype=torch.float32, device=dev)
    T = L.developmentTime(s, THICK, H)
    g = np.random.default_rng(1).uniform(0.5, 1.5, (D, n, n)).astype(np.float32)
    grad = L.developmentTimeGradient(s, T, torch.from_numpy(g).to(dev), THICK, H).cpu().numpy().astype(np.float64)
    below = np.cumsum(g.astype(np.float64)[::-1], axis=0)[::-1]
    want = below * np.where(np.arange(D) == 0, 0.5 * hz, hz)[:, None, None]
    err = float(np.abs(grad - want).max() / want.max())
    bound = (2 * D + (hz / H) ** 2 * D * D) * U
    print(f"uniform slowness: max error / max |grad| = {err:.2e} (bound {bound:.2e})")
    assert err <= bound


# ---- 8. the rate law backwards ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(1, 1), (15, 2), (16, 5), (24, 32)])
def test_rate_gradients_against_the_oracle(L, dev, n, D):
    from lithographysimulator_amd import peb
    rng = np.random.default_rng(n + D)
    I = rng.uniform(0.0, 3.0, (2, D, n, n)).astype(np.float32)
    I.flat[0] = 0.0                                                            # unexposed
    if n > 1:
        I[1, 0, 1, 2], I[0, D - 1, n - 1, n - 1] = -0.5, np.nan                  # walls
    doses = (0.6, 1.0, 1.7)
    gains = [f32(d) for d in doses]
    gs = rng.standard_normal((6, D, n, n)).astype(np.float32)
    if n > 1:
        gs[1::2, 0, 1, 2] = np.nan                                             # volume 1, every dose: the cotangent of a wall is ignored
    Id, gsd = torch.from_numpy(I).to(dev), torch.from_numpy(gs).to(dev)
    for r0, delta in ((1.0, None), (0.25, 30.0)):
        resist = L.MackResist(C=0.9, rMax=120.0, rMin=0.05, q=5.0, mTh=0.4, surfaceRate=r0, surfaceDepth=delta)
        got = L.developmentRateGradient(Id, resist, THICK, H, doses, gsd)
        assert got.dtype == torch.float32 and tuple(got.shape) == I.shape
        want = GO.rate_vjp(I, gains, 0.9, 120.0, 0.05, 5.0, 0.4, THICK, r0, delta if delta else 1.0, gs)
        gn = got.cpu().numpy().astype(np.float64)
        err = float(np.abs(gn - want).max() / np.abs(want).max())
        print(f"rate vjp n {n} D {D} surface {r0}: max error {err:.2e} of max |grad| {np.abs(want).max():.3e} (bound 1e-6)")
        assert err <= 1e-6 and gn.flat[0] == 0.0
        if n > 1:
            assert gn[1, 0, 1, 2] == 0.0 and gn[0, D - 1, n - 1, n - 1] == 0.0
        one = L.developmentRateGradient(Id[1], resist, THICK, H, doses, gsd[1::2].contiguous())     # [D,n,n] in
        assert tuple(one.shape) == (D, n, n) and torch.equal(one, got[1])
    # the amplified resist: kappa = kAmp, x = the acid dose, a single gain of 1
    r = TG.resist_variants(L, D)[0]
    a = (I * 20.0).astype(np.float32)                                          # kAmp a up to 3
    ga = peb.amplifiedRateGradient(torch.from_numpy(a).to(dev), r, THICK, gsd[:2].contiguous())
    m = r.mack
    want = GO.rate_vjp(a, [1.0], r.kAmp, m.rMax, m.rMin, m.q, m.mTh, THICK, 1.0, 1.0, gs[:2])
    err = float(np.abs(ga.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
    print(f"amplified rate vjp n {n} D {D}: max error {err:.2e} of max |grad|")
    assert err <= 1e-6 and tuple(ga.shape) == a.shape
    if n > 1:
        assert float(ga[1, 0, 1, 2]) == 0.0 and float(ga[0, D - 1, n - 1, n - 1]) == 0.0
    one = peb.amplifiedRateGradient(torch.from_numpy(a[0]).to(dev), r, THICK, gsd[0].contiguous())
    assert torch.equal(one, ga[0])


# ---- 9. the chain ----------------------------------------------------------------------------------------------------------------
TOL_CHAIN_TIME = 2e-6       # the solver's share: the cap that every TOL_TIME stays below


@pytest.mark.parametrize("n,D", [(17, 4), (32, 2)])
def test_the_profile_gradient_equals_the_composition_of_the_oracles(L, dev, n, D):
    """resistProfileGradient for a MackResist with diffusion, two doses and two focal planes, and for a chemically amplified one.
    The oracles are composed from the device's own slowness and T (what the call computes inside, bit for bit): time_vjp, then
    rate_vjp on the float64 diffused image, then the diffusion again (it is its own adjoint); for the amplified resist rate_vjp on
    the device's acid dose, then the bake's oracle chain of test_gpu_peb_grad.  Bound per cell: the solver's error, at most
    TOL_CHAIN_TIME max |gradSlowness|, times the cell's |ds/dx| summed over the doses, plus 2^-22 of the cell's own terms for the
    rate kernel -- pushed through the diffusion (non-negative taps: the bound of the sum is the sum of the bounds), plus the
    diffusion test's bound on the largest value.  For the bake: its adjoint maps an error e on gradAcidDose to at most
    bakeTime e on hbar_0 (the header's convex-combination argument), and the exposure multiplies by C dose; on top of
    oracle_chain's own bound."""
    import test_gpu_peb_grad as PG
    from lithographysimulator_amd import peb
    pixel, thick, doses, F = 10.0, 80.0, (0.8, 1.0), 2
    hz = thick / D
    I = (TG.line_space(n, D, 16)[None] * np.array([1.0, 0.7], dtype=np.float32)[:, None, None, None]).astype(np.float32)
    Id = torch.from_numpy(I).to(dev)
    rng = np.random.default_rng(n + D)
    gT = rng.standard_normal((2, F, D, n, n)).astype(np.float32)
    gTd = torch.from_numpy(gT).to(dev)
    gains = [f32(d) for d in doses]
    # -- Mack resist
    resist = L.MackResist(C=2.0, rMax=100.0, rMin=0.05, q=4.0, mTh=0.5, surfaceRate=0.5, surfaceDepth=20.0, diffusionLength=15.0,
                          verticalDiffusionLength=12.0)
    got = L.resistProfileGradient(Id.reshape(F * D, n, n), resist, thick, pixel, gTd, doses=doses, focalPlanes=F)
    assert got.dtype == torch.float32 and tuple(got.shape) == (F * D, n, n)
    s = L.developmentRate(Id, resist, thick, pixel, doses)
    T = L.developmentTime(s, thick, pixel)
    gs = oracle_time_vjp(T.cpu().numpy(), s.cpu().numpy(), gT.reshape(2 * F, D, n, n), thick, pixel)
    sxy, sz = 15.0 / pixel, 12.0 / hz
    lat = DO.diffuse(I.astype(np.float64), sxy, sz)
    par = (2.0, 100.0, 0.05, 4.0, 0.5, thick, 0.5, 20.0)
    pre = GO.rate_vjp(lat, gains, *par, gs)
    want = DO.diffuse(pre, sxy, sz)
    e_s = TOL_CHAIN_TIME * np.abs(gs).reshape(2 * F, -1).max(axis=1).max()
    slope = np.abs(GO.rate_vjp(lat, gains, *par, np.ones_like(gs)))            # sum over the doses of |ds/dx|: one sign
    terms = np.abs(GO.rate_vjp(lat, gains, *par, np.abs(gs)))
    bound = DO.diffuse(e_s * slope + 2.0 ** -22 * terms, sxy, sz) + TD.diffusion_bound(RO.radius(sxy), RO.radius(sz)) * np.abs(pre).max()
    err = np.abs(got.cpu().numpy().astype(np.float64).reshape(F, D, n, n) - want)
    print(f"profile gradient (Mack) n {n} D {D}: max error {err.max():.2e} = {float((err / bound).max()):.3f} of its bound; "
          f"max |gradImage| {np.abs(want).max():.3e}, largest bound {bound.max():.2e}")
    assert (err <= bound).all() and bound.max() < 1e-2 * np.abs(want).max()
    # -- chemically amplified resist, one focal plane per call as resistProfile takes it
    r = PG.chain_resist(L)
    got = L.resistProfileGradient(Id[0], r, thick, pixel, gTd[:, :1].contiguous(), doses=doses)
    bake = L.postExposureBake(Id[:1], r, thick, pixel, doses)
    T = L.developmentTime(bake.slowness, thick, pixel)
    gs = oracle_time_vjp(T.cpu().numpy(), bake.slowness.cpu().numpy(), gT[:, 0], thick, pixel)
    a = bake.acidDose.cpu().numpy()
    m = r.mack
    mp = (r.kAmp, m.rMax, m.rMin, m.q, m.mTh, thick, 1.0, 1.0)
    ga = GO.rate_vjp(a, [1.0], *mp, gs)
    h0 = peb.exposeAcid(Id[:1], r.C, doses).cpu().numpy().astype(np.float64)
    want, bound = PG.oracle_chain(I[:1].astype(np.float64), r, thick, pixel, doses, bake.steps, h0, None, ga, None, None)
    e_a = float((TOL_CHAIN_TIME * np.abs(gs).max() * np.abs(GO.rate_vjp(a, [1.0], *mp, np.ones_like(gs))) + 2.0 ** -22 * np.abs(ga)).max())
    bound = bound + sum(r.C * g for g in gains) * r.bakeTime * e_a
    err = np.abs(got.cpu().numpy().astype(np.float64)[None] - want)
    print(f"profile gradient (amplified) n {n} D {D} S {bake.steps}: max error {err.max():.2e} = {float((err / bound).max()):.3f} of its "
          f"bound; max |gradImage| {np.abs(want).max():.3e}")
    assert tuple(got.shape) == (D, n, n) and (err <= bound).all() and bound.max() < 1e-2 * np.abs(want).max()


# ---- 10. the model for optimizeMask ----------------------------------------------------------------------------------------------
def _model_resists(L):
    mack = L.MackResist(C=2.0, rMax=100.0, rMin=0.05, q=4.0, mTh=0.5, surfaceRate=0.5, surfaceDepth=20.0, diffusionLength=15.0,
                        verticalDiffusionLength=12.0)
    car = L.ChemicallyAmplifiedResist(C=2.0, quencher=0.15, kAmp=0.04, kQuench=5.0, kLoss=0.002, acidDiffusionLength=12.0,
                                      quencherDiffusionLength=4.0, verticalScale=1.0, bakeTime=TG.BAKE, mack=TG.mack(L))
    return {"mack": mack, "amplified": car}


def _arrival_times(L, dev, socs, resist, thick, pixel, deltaK, scale, t):
    """T of the transmission t through the device model and the public calls, [planes, n_out, n_out]."""
    from lithographysimulator_amd.ilt import _device_model
    image = _device_model(socs, int(socs.pn), pixel, deltaK, 193.0, True, dev)[0](t) * scale
    image = image if image.dim() == 3 else image[None]
    if isinstance(resist, L.MackResist):
        s = L.developmentRate(image, resist, thick, pixel)
    else:
        s = L.postExposureBake(image, resist, thick, pixel).slowness
    return L.developmentTime(s, thick, pixel)[0]


@pytest.mark.parametrize("kind", ["mack", "amplified"])
@pytest.mark.parametrize("planes", [1, 2])
def test_the_developed_resist_model_adjoint(L, dev, planes, kind):
    """developedResistModel at pn = 64: <adjoint(g), dt> against the central difference of <g, imager(t)> along dt, on the device,
    both resists, one plane and two.  g is positive and dt = t itself plus a tenth of noise, so that the sum is coherent.  The
    step: T is piecewise smooth in the mask -- C^1 across a branch switch, but with a kink wherever a cell changes its upwind
    neighbour or crosses the clamp -- so the quotient is off by a term linear in eps with a lumpy coefficient (one kink of a cell
    with many cells downstream is one lump), and by the fp32 rounding of the forward, which grows as 1 / eps.  Measured on an
    MI355X, stage by stage on the hardest case (amplified, two planes; the slowness moves by 10 eps): kinks 5e-4 at eps 1e-3 and
    5e-6 at 1e-4, rounding 1e-4 at 3e-5 and 2e-4 at 1e-5; hence eps = 1e-4.  At that step the four cases gave 4.7e-5, 2.0e-5 (Mack,
    one and two planes), 6.0e-5 and 9.1e-4 (amplified; a lump -- the stage-by-stage quotients of that case agree to 7e-6 and its
    solver adjoint agrees with a float64 difference quotient to 2e-8).  Tolerance 1e-3, the baked-resist model test's."""
    case = SG.device_case(64, "copy", planes, True)
    socs = SG.socs_around(case.kernels, dev, weight_sum=SG.ILT_WEIGHT_SUM)
    resist, thick = _model_resists(L)[kind], 80.0
    scale = 0.9 / float(case.image0.median())
    t = case.t0.to(torch.complex64).to(dev)
    T0 = _arrival_times(L, dev, socs, resist, thick, case.ps, 4 / 64, scale, t).flatten()
    t_dev = float(T0[torch.isfinite(T0)].median())                               # half of the cells develop
    imager, adjoint = L.developedResistModel(socs, resist, thick, case.ps, 4 / 64, 193.0, t_dev, intensityScale=scale)
    margin = imager(t)
    assert tuple(margin.shape) == (planes, case.n_out, case.n_out) and float(margin.min()) >= -1.0 and float(margin.max()) > 0.0
    rng = np.random.default_rng(planes)
    g = torch.from_numpy(rng.uniform(0.5, 1.5, (planes, case.n_out, case.n_out)).astype(np.float32)).to(dev)
    noise = torch.from_numpy((rng.standard_normal((64, 64)) + 1j * rng.standard_normal((64, 64))).astype(np.complex64)).to(dev)
    dt = t + 0.1 * noise
    grad = adjoint(g if planes > 1 else g[0])
    assert grad.dtype == torch.complex64 and tuple(grad.shape) == (64, 64)
    analytic = float((grad.to(torch.complex128).conj() * dt.to(torch.complex128)).real.sum())
    eps = 1e-4
    up = float((g.double() * imager(t + eps * dt).double()).sum())
    down = float((g.double() * imager(t - eps * dt).double()).sum())
    numeric = (up - down) / (2 * eps)
    rel = abs(analytic - numeric) / abs(numeric)
    print(f"developed model adjoint, {kind}, planes {planes}, developTime {t_dev:.3g} s: <adjoint(g), dt> = {analytic:.6e}, "
          f"difference quotient {numeric:.6e}, relative difference {rel:.2e}")
    assert rel <= 1e-3


def test_three_iterations_with_the_model_lower_the_loss(L, dev):
    """The contact target and optical setting of the baked-resist test, the loss on the developed profile, threshold 0."""
    pn, pixel, wl, na, thick = 32, 25.0, 193.0, 0.7, 80.0
    source = L.LightSource(0.4, 0.8, pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
    socs = L.socsKernels(pupil, source, kernels=8)
    open_mask = L.Mask(torch.ones((pn, pn), dtype=torch.int16), pixel, dev)
    deltaK = open_mask.deltaK
    clear = L.hopkinsImage(open_mask, open_mask.fraunhofer(wl, True), socs, pixel, deltaK, wl, normalize=True)
    n_out = clear.shape[-1]
    target = torch.zeros((n_out, n_out), dtype=torch.float32, device=dev)
    target[12:20, 12:20] = 1.0
    scale = 1.0 / float(clear[n_out // 2, n_out // 2])
    t0 = torch.zeros((pn, pn), dtype=torch.complex64, device=dev)
    t0[12:20, 12:20] = 1.0
    for kind, resist in _model_resists(L).items():
        # a development time at which the contact of the starting mask has cleared at its centre and nothing else has
        t_dev = 1.5 * float(_arrival_times(L, dev, socs, resist, thick, pixel, deltaK, scale, t0)[:, 16, 16].max())
        assert math.isfinite(t_dev)
        imager, adjoint = L.developedResistModel(socs, resist, thick, pixel, deltaK, wl, t_dev, intensityScale=scale)
        res = L.optimizeMask(target, socs, pixel, deltaK, wl, 0.0, iterations=3, step=0.1, imager=imager, adjoint=adjoint)
        print(f"developed-resist ILT ({kind}), developTime {t_dev:.3g} s, 3 iterations: losses " + " ".join(f"{v:.6f}" for v in res.losses))
        assert len(res.losses) == 4 and all(math.isfinite(v) for v in res.losses) and res.losses[3] < res.losses[0]


# ---- 11. arguments ---------------------------------------------------------------------------------------------------------------
def test_argument_errors(L, dev):
    from lithographysimulator_amd import _native as nat
    from lithographysimulator_amd import peb
    assert develop_vjp_argument_errors(nat) > 30                                # every code of the C ABI, before any launch
    s = torch.rand((2, 4, 8, 8), device=dev) + 0.1
    T = L.developmentTime(s, 80.0, 10.0)
    g = torch.rand_like(s)
    for args, kw in (((s, T[0], g), {}), ((s, T, g[:, :2]), {}), ((s, T.double(), g), {}), ((s, T, g.cpu()), {}), ((s.cpu(), T, g), {}),
                     ((s, T, g), dict(maxIterations=0)), ((s, T, g), dict(maxIterations=65537)), ((s[0, 0], T[0, 0], g[0, 0]), {})):
        with pytest.raises((ValueError, RuntimeError)):
            L.developmentTimeGradient(*args, 80.0, 10.0, **kw)
    for thick, pixel in ((0.0, 10.0), (80.0, float("nan"))):
        with pytest.raises(ValueError):
            L.developmentTimeGradient(s, T, g, thick, pixel)
    # the library refuses an output that overlaps an input and a workspace that is too small, with the codes, before any launch
    lib = nat.lib()
    launches = ctypes.c_int(0)
    need = lib.litho_develop_vjp_work_bytes(2, 4, 8, 16)
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    call = lambda out, nbytes: lib.litho_develop_time_vjp(nat.ptr(s), nat.ptr(T), nat.ptr(g), 2, 4, 8, 80.0, 10.0, 16, nat.ptr(out),    # noqa: E731
                                                          nat.ptr(work), nbytes, ctypes.byref(launches), None)
    assert call(g, need) == nat.E_ARG and call(T, need) == nat.E_ARG and call(torch.empty_like(s), need - 1) == nat.E_WORKSPACE
    mack = TG.mack(L)
    with pytest.raises(TypeError):
        L.developmentRateGradient(s, TG.resist_variants(L, 4)[0], 80.0, 10.0, (1.0,), g)
    with pytest.raises(TypeError):
        peb.amplifiedRateGradient(s, mack, 80.0, g)
    for bad in (g[:1], g.double(), g.cpu()):
        with pytest.raises(ValueError):
            L.developmentRateGradient(s, mack, 80.0, 10.0, (1.0,), bad)
    with pytest.raises(ValueError):
        L.developmentRateGradient(s, mack, 80.0, 10.0, (1.0, 2.0), g)          # gradSlowness must hold both doses
    with pytest.raises(ValueError):
        L.resistProfileGradient(s[0], mack, 80.0, 10.0, g[0])                   # gradT must be [doses, F, D, n, n]
    with pytest.raises(ValueError):
        L.resistProfileGradient(s, mack, 80.0, 10.0, g)                         # image must be [F D, n, n]
    socs = SG.socs_around(SG.device_case(32, "copy", 1, True).kernels, dev)
    with pytest.raises(TypeError):
        L.developedResistModel(socs, "resist", 80.0, 10.0, 4 / 32, 193.0, 10.0)
    for kw in (dict(developTime=0.0), dict(developTime=10.0, intensityScale=-1.0), dict(developTime=10.0, maxIterations=0)):
        with pytest.raises(ValueError):
            L.developedResistModel(socs, mack, 80.0, 10.0, 4 / 32, 193.0, **kw)
    out = L.developmentTimeGradient(s, T, g, 80.0, 10.0, maxIterations=1024)     # the plain call still runs
    assert bool(torch.isfinite(out).all())
