"""Gradients through the post-exposure bake on the GPU (csrc/peb.hip: litho_peb_bake_vjp, litho_peb_expose_vjp) through
lithographysimulator_amd/peb.py and ilt.bakedResistModel, against the float64 restatement tests/peb_grad_oracle.py (pinned to
central differences of the bake in test_peb_grad_cpu.py).

Bounds.  G = max(|gh|_inf, |gq|_inf) + bakeTime |ga|_inf bounds |hbar_0| and |qbar_0| (the header's convex-combination argument).
  bake vjp      max |hbar_0 - f64|, max |qbar_0 - f64| <= C_GRAD S 2^-24 G over every cell.  A backward step is a fixed number of
                fp32 roundings through an update that does not expand differences, so its own errors add like the forward's; on
                top the reaction's Jacobian (Lipschitz constant of order beta) acts on the forward error of the tape, of order
                S 2^-24.  That second part cannot be derived here: C_GRAD is measured on an MI355X against the float64 oracle,
                fed the fp32 step parameters the library uses, and set to about four times the worst ratio, per class of resist:
                    finite kQuench   measured 0.35 ... 0.66 of S 2^-24 G (the worst at n 48, D 17), C_GRAD 2.6
                    instantaneous    measured 0.40 ... 0.89 of S 2^-24 G (the worst at n 1, D 1),   C_GRAD 3.5
                (the worst per shape over the resists, S = 5, 7, 33 and the four sets of cotangents).
                Condition (not a measurement): C_GRAD S 2^-24 < 1e-3 for every S used -- a missing term, a wrong sign or a wrong
                face rule is wrong at 1e-1 G.
  instantaneous the fp32 and the float64 run must take the same branch at every cell and step.  Mixed-branch inputs (h0 in
                [0, 1] around q0 = 0.3 / 0.2) run at the shapes up to (24, 5) with S = 5, 7, with a seed for which the oracle's
                trajectory keeps min |hd - qd| >= 2 C_PEB S 2^-24 max(1, q0), twice the forward's proven bound (asserted).  Every
                shape and S also runs constant-branch inputs: q0 = 1.5 with h0 in [0, 1], q0 = 0.05 with h0 in [0.2, 1].
  exposure vjp  |got - f64| <= 2^-22 sum_g |term_g|: one fp32 rounding of a double sum, one more for a last-place difference of
                the device's exp.
  chain         see test_the_chain_equals_the_composition_of_the_oracles.
Shapes: test_gpu_peb's (n = 1, 2, 15, 16, 17, 24, 48; D = 1, 2, 5, 17, 32), B = 3 volumes, S = 5, 7, 33.  Every test prints what it
observed (-s)."""
import math

import numpy as np
import pytest
import torch

import peb_grad_oracle as GO
import peb_oracle as PO
import socs_grad_oracle as SG
import test_gpu_peb as TG
from test_peb_grad_cpu import bake_vjp_argument_errors

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_GRAD = {"finite": 2.6, "instant": 3.5}
C_PEB, H, THICK, BAKE, SHAPES = TG.C_PEB, TG.H, TG.THICK, TG.BAKE, TG.SHAPES
STEPS = (5, 7, 33)
SMALL = [(n, D) for n, D in SHAPES if n <= 24 and D <= 5]                   # where mixed-branch instantaneous cases run


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


@pytest.fixture(scope="module")
def peb():
    from lithographysimulator_amd import peb
    return peb


def test_the_bound_stays_below_the_cap():
    for kind, c in C_GRAD.items():
        assert c * max(STEPS) * U < 1e-3, kind


def with_quencher(L, r, q0):
    return L.ChemicallyAmplifiedResist(C=r.C, quencher=q0, kAmp=r.kAmp, kQuench=r.kQuench, kLoss=r.kLoss,
                                       acidDiffusionLength=r.acidDiffusionLength, quencherDiffusionLength=r.quencherDiffusionLength,
                                       verticalScale=r.verticalScale, bakeTime=r.bakeTime, mack=r.mack)


def parameters(r, D, S):
    return PO.step_parameters(r.kQuench, r.kLoss, r.acidDiffusionLength, r.quencherDiffusionLength, r.verticalScale, r.bakeTime, THICK, D, H, S)


def volumes(n, D, seed, low=0.0):
    """h0 ~ U(low, 1) and the three cotangents (gh, gq ~ U(-1, 1), ga ~ U(-1, 1) / bakeTime), fp32 [3, D, n, n]."""
    rng = np.random.default_rng(1000 * n + 10 * D + seed)
    shape = (3, D, n, n)
    h0 = rng.uniform(low, 1.0, shape).astype(np.float32)
    gh, gq = (rng.uniform(-1.0, 1.0, shape).astype(np.float32) for _ in range(2))
    return h0, (gh, gq, (rng.uniform(-1.0, 1.0, shape) / BAKE).astype(np.float32))


def runs_of(L, n, D):
    """(label, kind, resist, S, h0, cotangents, floor of |hd - qd| or None) for one shape: the four resists as they are (the
    instantaneous ones at the small shapes and S = 5, 7 only, with a seed that keeps the branches apart) and the instantaneous
    ones with constant-branch inputs at every S."""
    out = []
    for ri, r in enumerate(TG.resist_variants(L, D)):
        instant = math.isinf(r.kQuench)
        if not instant:
            out += [(f"resist {ri}", "finite", r, S) + volumes(n, D, 0) + (None,) for S in STEPS]
            continue
        if (n, D) in SMALL:
            for S in (5, 7):
                P, q0 = parameters(r, D, S), float(np.float32(r.quencher))
                floor = 2 * C_PEB * S * U * max(1.0, q0)
                seed = next(s for s in range(16) if GO.branch_margin(GO.tape(volumes(n, D, s)[0], q0, S, **P)[0]) >= floor)
                out.append((f"resist {ri} mixed, seed {seed}", "instant", r, S) + volumes(n, D, seed) + (floor,))
        for q0, low in ((1.5, 0.0), (0.05, 0.2)):
            rq = with_quencher(L, r, q0)
            out += [(f"resist {ri} q0 {q0}", "instant", rq, S) + volumes(n, D, 0, low) + (2 * C_PEB * S * U * max(1.0, q0),) for S in STEPS]
    return out


def to_dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(a).to(dev) for a in arrays]


# ---- parity with the float64 oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", SHAPES)
def test_bake_gradient_against_the_oracle(L, peb, dev, n, D):
    """(hbar_0, qbar_0) over every cell, for each single cotangent and all three together."""
    worst = {"finite": 0.0, "instant": 0.0}
    failures = []
    for label, kind, r, S, h0, cots, floor in runs_of(L, n, D):
        P, q0 = parameters(r, D, S), float(np.float32(r.quencher))
        taped = GO.tape(h0, q0, S, **P)[0]
        if floor is not None:
            margin = GO.branch_margin(taped)
            assert margin >= floor, (label, S, margin, floor)
        (h0d,) = to_dev(dev, h0)
        for pick in ((0,), (1,), (2,), (0, 1, 2)):
            given = [c if i in pick else None for i, c in enumerate(cots)]
            G = GO.bound_scale(*given, r.bakeTime)
            want = GO.bake_vjp(h0, q0, S, *given, **P, taped=taped)
            got = peb.bakeGradient(h0d, r, THICK, H, *to_dev(dev, *given), steps=S)
            assert all(t.dtype == torch.float32 and tuple(t.shape) == h0.shape for t in got)
            ratio = max(float(np.abs(g.cpu().numpy().astype(np.float64) - w).max()) for g, w in zip(got, want)) / (S * U * G)
            worst[kind] = max(worst[kind], ratio)
            if not ratio <= C_GRAD[kind]:
                failures.append((label, S, pick, ratio))
    print(f"bake vjp n {n} D {D}: worst error / (S 2^-24 G) = {worst['finite']:.3f} (finite kQuench; C_GRAD {C_GRAD['finite']}) "
          f"{worst['instant']:.3f} (instantaneous; C_GRAD {C_GRAD['instant']})")
    assert not failures, failures


# ---- bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(2, 5), (17, 5), (48, 2)])
def test_the_bits_do_not_depend_on_the_checkpoints_the_batch_or_the_call(L, peb, dev, n, D):
    """c = 1, 3, ceil(sqrt S) and S at S = 7 (c does not divide S) and S = 33; B = 3 volumes at once against one at a time and a
    [D,n,n] input; two identical calls; absent cotangents against explicit zeros: the same bit patterns."""
    h0, cots = volumes(n, D, 3)
    h0d, gh, gq, ga = to_dev(dev, h0, *cots)
    zero = torch.zeros_like(h0d)
    for r in TG.resist_variants(L, D)[1:3]:                                     # both species diffuse; kQuench inf and finite
        base = {}
        for S in (7, 33):
            root = math.isqrt(S - 1) + 1
            base[S] = peb.bakeGradient(h0d, r, THICK, H, gh, gq, ga, steps=S, checkpointEvery=1)
            for c in (3, root, S):
                assert TG.same_bits(peb.bakeGradient(h0d, r, THICK, H, gh, gq, ga, steps=S, checkpointEvery=c), base[S]), f"S {S} c {c}"
            auto = peb.bakeGradient(h0d, r, THICK, H, gh, gq, ga, steps=S)
            assert TG.same_bits(auto, base[S]) and TG.same_bits(peb.bakeGradient(h0d, r, THICK, H, gh, gq, ga, steps=S), auto)
        for b in range(3):
            alone = peb.bakeGradient(h0d[b:b + 1], r, THICK, H, gh[b:b + 1], gq[b:b + 1], ga[b:b + 1], steps=7)
            assert TG.same_bits(alone, [t[b:b + 1] for t in base[7]]), f"volume {b} alone"
            plain = peb.bakeGradient(h0d[b], r, THICK, H, gh[b], gq[b], ga[b], steps=7)
            assert all(tuple(t.shape) == (D, n, n) for t in plain) and TG.same_bits(plain, [t[0] for t in alone])
        for pick in ((0,), (1,), (2,), (0, 2)):
            some = [g if i in pick else None for i, g in enumerate((gh, gq, ga))]
            full = [g if i in pick else zero for i, g in enumerate((gh, gq, ga))]
            assert TG.same_bits(peb.bakeGradient(h0d, r, THICK, H, *some, steps=7), peb.bakeGradient(h0d, r, THICK, H, *full, steps=7)), pick
    print(f"bit identity n {n} D {D}: checkpointEvery 1, 3, ceil(sqrt S), S and automatic; batch and single volumes; absent and zero cotangents agree")


# ---- the exposure ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(1, 1), (15, 2), (16, 5)])
def test_exposure_gradient_against_the_oracle(L, peb, dev, n, D):
    rng = np.random.default_rng(n + D)
    I = rng.uniform(0.0, 3.0, (2, D, n, n)).astype(np.float32)
    worst = 0.0
    for doses in ((1.3,), (0.6, 1.0, 1.7)):
        g = rng.uniform(-1.0, 1.0, (2 * len(doses), D, n, n)).astype(np.float32)
        want = GO.expose_vjp(I, doses, 0.9, g)
        terms = sum(np.abs(GO.expose_vjp(I, doses[i:i + 1], 0.9, g[2 * i:2 * i + 2])) for i in range(len(doses)))
        inputs = [to_dev(dev, I, g)]
        # the same numbers one float off a 16-byte boundary: the scalar path even where n is a multiple of 4
        flat = [torch.empty(a.size + 1, dtype=torch.float32, device=dev) for a in (I, g)]
        views = [f[1:].view(a.shape) for f, a in zip(flat, (I, g))]
        for v, a in zip(views, (I, g)):
            v.copy_(torch.from_numpy(a))
        assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views)
        inputs.append(views)
        outs = []
        for Id, gd in inputs:
            got = peb.exposeAcidGradient(Id, 0.9, doses, gd)
            assert got.dtype == torch.float32 and tuple(got.shape) == I.shape
            err = np.abs(got.cpu().numpy().astype(np.float64) - want)
            worst = max(worst, float((err / terms).max()))
            assert (err <= 2.0 ** -22 * terms).all()
            outs.append(got)
        assert torch.equal(outs[0], outs[1])
        one = peb.exposeAcidGradient(inputs[0][0][1], 0.9, doses, inputs[0][1][1::2].contiguous())      # [D,n,n] in
        assert tuple(one.shape) == (D, n, n) and torch.equal(one, outs[0][1])
    print(f"exposure vjp n {n} D {D}: worst error / sum |terms| = {worst:.2e} (bound {2.0 ** -22:.2e})")


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
def chain_resist(L, q0=0.15):
    return L.ChemicallyAmplifiedResist(C=2.0, quencher=q0, kAmp=0.04, kQuench=5.0, kLoss=0.002, acidDiffusionLength=12.0,
                                       quencherDiffusionLength=4.0, verticalScale=1.0, bakeTime=BAKE, mack=TG.mack(L))


def oracle_chain(I, r, thick, pixel, doses, S, h0, gm, ga, gh, gq):
    """gradImage by the three oracles from the scaled intensity I [F,D,n,n] and the device's own fp32 acid h0 (so that both bakes
    start from the same numbers); returns (gradImage, the bound on its error per cell)."""
    D = I.shape[1]
    P = PO.step_parameters(r.kQuench, r.kLoss, r.acidDiffusionLength, r.quencherDiffusionLength, r.verticalScale, r.bakeTime, thick, D, pixel, S)
    q0 = float(np.float32(r.quencher))
    taped, (_, _, a) = GO.tape(h0, q0, S, **P)
    zero = np.zeros(a.shape)
    gm, ga, gh, gq = (zero if g is None else g.astype(np.float64) for g in (gm, ga, gh, gq))
    abar = ga + GO.inhibitor_vjp(a, r.kAmp, gm)
    hb, _ = GO.bake_vjp(h0, q0, S, gh, gq, abar, **P, taped=taped)
    out = GO.expose_vjp(I, doses, r.C, hb)
    # the bake's vjp within C_GRAD S 2^-24 G; abar formed in fp32 from the device's a (|dm| <= kAmp |da|, |da| within the forward's
    # bound, a handful of roundings on top), which reaches hbar_0 times at most bakeTime; then the exposure's own 2^-22 per term
    G = GO.bound_scale(gh, gq, abar, r.bakeTime)
    d_abar = r.kAmp * float(np.abs(gm).max()) * (r.kAmp * r.bakeTime * C_PEB * S * U * max(1.0, q0) + 8 * U) + 2 * U * float(np.abs(ga).max())
    per_cell = C_GRAD["finite"] * S * U * G + r.bakeTime * d_abar
    gains = [r.C * float(np.float32(d)) for d in doses]
    terms = sum(np.abs(GO.expose_vjp(I, doses[i:i + 1], r.C, hb.reshape((len(doses),) + I.shape)[i])) for i in range(len(doses)))
    return out, sum(gains) * per_cell + 2.0 ** -22 * terms


@pytest.mark.parametrize("n,D", [(17, 4), (32, 2)])
def test_the_chain_equals_the_composition_of_the_oracles(L, peb, dev, n, D):
    """postExposureBakeGradient with all four cotangents, and with the inhibitor's alone, two doses, the default steps."""
    pixel, thick, doses = 10.0, 80.0, (0.8, 1.0)
    r = chain_resist(L)
    I = (TG.line_space(n, D, 16)[None] * np.array([1.0, 0.7], dtype=np.float32)[:, None, None, None]).astype(np.float32)   # F = 2
    rng = np.random.default_rng(n)
    shape = (4, D, n, n)
    gm, gh, gq = (rng.uniform(-1.0, 1.0, shape).astype(np.float32) for _ in range(3))
    ga = (rng.uniform(-1.0, 1.0, shape) / BAKE).astype(np.float32)
    (Id,) = to_dev(dev, I)
    S = L.postExposureBake(Id, r, thick, pixel, doses).steps
    assert S == max(r.minSteps(thick, D, pixel), 8)
    h0 = peb.exposeAcid(Id, r.C, doses).cpu().numpy().astype(np.float64)
    for cots in ((gm, ga, gh, gq), (gm, None, None, None)):
        want, bound = oracle_chain(I.astype(np.float64), r, thick, pixel, doses, S, h0, *cots)
        m, a, h, q = to_dev(dev, *cots)
        got = L.postExposureBakeGradient(Id, r, thick, pixel, doses, gradInhibitor=m, gradAcidDose=a, gradAcid=h, gradQuencher=q)
        assert got.dtype == torch.float32 and tuple(got.shape) == I.shape
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print(f"chain n {n} D {D} S {S} ({sum(c is not None for c in cots)} cotangents): max error {err.max():.2e}, "
              f"{float((err / bound).max()):.3f} of its bound; max |gradImage| {np.abs(want).max():.2e}")
        assert (err <= bound).all() and bound.max() < 1e-2 * np.abs(want).max()
    one = L.postExposureBakeGradient(Id[0], r, thick, pixel, (1.0,), gradInhibitor=to_dev(dev, gm[2:3])[0])   # [D,n,n] in
    both = L.postExposureBakeGradient(Id, r, thick, pixel, (1.0,), gradInhibitor=to_dev(dev, gm[2:4])[0])
    assert tuple(one.shape) == (D, n, n) and torch.equal(one, both[0])


@pytest.mark.parametrize("planes", [1, 2])
def test_the_baked_resist_model_adjoint(L, peb, dev, planes):
    """bakedResistModel at pn = 32: the imager is the device model's image x intensityScale through postExposureBake, and the
    adjoint equals the existing device adjoint applied to the oracles' gradImage (from the device's own scaled intensity) x
    intensityScale.  Only the new part is under test: the optical adjoint is pinned in test_gpu_ilt.py.  It is linear and both
    sides go through it, so the difference is its image of the new part's error, which oracle_chain bounds per cell at ~1e-5 of
    max |gradImage|; the band-limited kernels pass the error no better than the signal, and 1e-3 of the result's maximum leaves
    that two orders while a wrong sign, a forgotten intensityScale or a dropped plane is wrong at 1."""
    from lithographysimulator_amd.ilt import _device_model
    case = SG.device_case(32, "copy", planes, True)
    socs = SG.socs_around(case.kernels, dev, weight_sum=SG.ILT_WEIGHT_SUM)
    r, thick = chain_resist(L), 80.0
    scale = 0.9 / float(case.image0.median())
    imager, adjoint = L.bakedResistModel(socs, r, thick, case.ps, 4 / 32, 193.0, intensityScale=scale)
    optics, optics_adjoint = _device_model(socs, 32, case.ps, 4 / 32, 193.0, True, dev)
    t = case.t0.to(torch.complex64).to(dev)
    I = (optics(t) * scale).reshape(planes, case.n_out, case.n_out)
    bake = L.postExposureBake(I, r, thick, case.ps)
    got_image = imager(t)
    assert tuple(got_image.shape) == (planes, case.n_out, case.n_out) and torch.equal(got_image, 1.0 - bake.inhibitor[0])
    g = np.random.default_rng(planes).uniform(-1.0, 1.0, (planes, case.n_out, case.n_out)).astype(np.float32)
    (gd,) = to_dev(dev, g)
    got = adjoint(gd if planes > 1 else gd[0])
    assert got.dtype == torch.complex64 and tuple(got.shape) == (32, 32)
    h0 = peb.exposeAcid(I, r.C).cpu().numpy().astype(np.float64)
    gI, _ = oracle_chain(I.cpu().numpy().astype(np.float64)[None], r, thick, case.ps, (1.0,), bake.steps, h0, -g[None], None, None, None)
    gI = torch.from_numpy((gI[0] * scale).astype(np.float32)).to(dev)
    want = optics_adjoint(gI if planes > 1 else gI[0])
    e_max = SG.rel_max(got, want)
    print(f"baked model adjoint planes {planes}, S {bake.steps}: max |got - want| / max |want| = {e_max:.2e}")
    assert e_max <= 1e-3


def test_three_iterations_with_the_model_lower_the_loss(L, dev):
    """A 32 x 32 contact target, a real optical setting (annular source, 8 kernels), the bake's dose in intensityScale."""
    pn, pixel, wl, na, thick = 32, 25.0, 193.0, 0.7, 80.0
    source = L.LightSource(0.4, 0.8, pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
    socs = L.socsKernels(pupil, source, kernels=8)
    open_mask = L.Mask(torch.ones((pn, pn), dtype=torch.int16), pixel, dev)
    deltaK = open_mask.deltaK
    clear = L.hopkinsImage(open_mask, open_mask.fraunhofer(wl, True), socs, pixel, deltaK, wl, normalize=True)
    n_out = clear.shape[-1]
    target = torch.zeros((n_out, n_out), dtype=torch.float32, device=dev)
    target[12:20, 12:20] = 1.0                                                  # a 200 nm contact
    r = L.ChemicallyAmplifiedResist(C=4.0, quencher=0.1, kAmp=0.025, kQuench=5.0, kLoss=0.002, acidDiffusionLength=10.0,
                                    quencherDiffusionLength=3.0, verticalScale=1.0, bakeTime=BAKE, mack=TG.mack(L))
    imager, adjoint = L.bakedResistModel(socs, r, thick, pixel, deltaK, wl, intensityScale=1.0 / float(clear[n_out // 2, n_out // 2]))
    res = L.optimizeMask(target, socs, pixel, deltaK, wl, 0.5, iterations=3, step=0.1, resistSteepness=10.0, imager=imager, adjoint=adjoint)
    print("baked-resist ILT, 3 iterations: losses " + " ".join(f"{v:.6f}" for v in res.losses))
    assert len(res.losses) == 4 and all(math.isfinite(v) for v in res.losses) and res.losses[3] < res.losses[0]


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors(L, peb, dev):
    from lithographysimulator_amd import _native as nat
    assert bake_vjp_argument_errors(nat) > 40                                   # every code of the C ABI, before any launch
    r = chain_resist(L)
    h0 = torch.rand((2, 4, 8, 8), device=dev)
    g = torch.rand_like(h0)
    least = r.minSteps(80.0, 4, 10.0)
    for kw in (dict(), dict(gradAcid=g, steps=least - 1), dict(gradAcid=g, steps=65537), dict(gradAcid=g, steps=8, checkpointEvery=0),
               dict(gradAcid=g, steps=8, checkpointEvery=9), dict(gradAcid=g[0]), dict(gradQuencher=g.double()), dict(gradAcidDose=g.cpu())):
        with pytest.raises(ValueError):
            peb.bakeGradient(h0, r, 80.0, 10.0, **kw)
    with pytest.raises(TypeError):
        peb.bakeGradient(h0, TG.mack(L), 80.0, 10.0, gradAcid=g)
    with pytest.raises(ValueError):
        peb.exposeAcidGradient(h0, 1.0, (1.0, 2.0), g)                          # gradAcid must hold both doses
    with pytest.raises(ValueError):
        L.postExposureBakeGradient(h0, r, 80.0, 10.0)
    out = peb.bakeGradient(h0, r, 80.0, 10.0, gradAcidDose=g, steps=least)       # the smallest legal call still runs
    assert all(bool(torch.isfinite(t).all()) for t in out)
