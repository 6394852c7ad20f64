"""Gradients with respect to the resist's own parameters, and a calibration loop on measured CDs; no reference counterpart
(include/litho_abbe.h: "Gradients with respect to the bake's parameters", "... the rate law's parameters"; DESIGN.md section 10;
csrc/peb.hip, csrc/develop_grad.hip).

The adjoint kernels of peb.py and develop.py carry a cotangent on the arrival times T down to the intensity.  This module
carries it to the numbers that define the resist, the resist-side twin of pupilGradient -> aberrationGradient -> fitAberrations:
  bakeStepGradient, bakeParameterGradient   the bake backwards with the sums of adjoint x d(step)/d(theta) per backward step
                                            (litho_peb_bake_vjp_params) and their chain to kQuench, kLoss, the two diffusion
                                            lengths and verticalScale (litho_peb_param_chain), next to the quencher loading
  rateParameterGradient                     the rate law's sums (litho_develop_rate_vjp_params) and their chain to C or kAmp,
                                            rMax, rMin, q, mTh and the surface inhibition (litho_develop_rate_param_chain)
  exposureParameterGradient                 dl/dC of the exposure (litho_peb_expose_vjp_params)
  resistParameterGradient                   the chain of resistProfileGradient with these reductions at each stage
  calibrateResist                           steepest descent with backtracking on CDs measured through dose and focus
  resistArrivalTimes, resistWith            the forward chain at a given step count; a resist with some parameters replaced
Every sum is taken in double in a fixed order without atomics: two calls give the same bits.

The bake's step count is an integer that the caller holds fixed: the derivative with respect to a diffusion length is that of
the step parameters' formulas at that count, the analytic one, not that of their rounding to fp32.

NOT built: the gradients of a MackResist's own Gaussian diffusion lengths, of bakeTime (a process setting) and of
`developedDepth`; bleaching.  calibrateResist(method="lm") is the Levenberg-Marquardt step on tangent.py's Jacobian."""
import ctypes
import math

import torch

from . import _native as nat
from .develop import (MackResist, _development_time, _gains, _like, _positive, _surface_depth, _volume, developmentRate, developmentTimeGradient,
                      latentDiffusion)
from .film import FilmStack
from .peb import ChemicallyAmplifiedResist, _bake_vjp, _steps, amplifiedRate, amplifiedRateGradient, bakeAcid, exposeAcid

STEP_SLOTS = ("lxy_h", "lz_h", "lxy_q", "lz_q", "beta", "fl")
BAKE_PARAMETERS = ("kQuench", "kLoss", "acidDiffusionLength", "quencherDiffusionLength", "verticalScale")
_MACK = ("rMax", "rMin", "q", "mTh", "surfaceRate", "surfaceDepth")                    # the rate law's, behind kappa = C or kAmp
_BAKED = ("C", "quencher", "kAmp") + BAKE_PARAMETERS


def bakeStepGradient(acid, resist, thickness, pixelSize, gradAcid=None, gradQuencher=None, gradAcidDose=None, steps=None, checkpointEvery=None):
    """bakeGradient with the gradient with respect to the six step parameters (litho_peb_bake_vjp_params): returns (gradAcid0,
    gradQuencher0, gradStep), the first two as bakeGradient returns them, bit for bit, and gradStep float64 [B, 6] (or [6] for a
    [D,n,n] input) on the device = dl/d(lxy_h, lz_h, lxy_q, lz_q, beta, fl), the sums over the backward steps and the cells of
    each volume, in double, in a fixed order: the bits depend on neither `checkpointEvery`, nor the other volumes of the batch,
    nor the call.  The slots of a species that does not diffuse are exactly 0, and so is beta's for instantaneous
    neutralisation.  The workspace keeps four volumes per taped step: (2 (ceil(steps / c) - 1) + 4 c + 8) volumes."""
    return _bake_vjp("bakeStepGradient", True, acid, resist, thickness, pixelSize, gradAcid, gradQuencher, gradAcidDose, steps, checkpointEvery)


def _bake_rows(who, what, rows, n_in, n_out, entry, resist, thickness, pixelSize, D, steps):
    """`rows` [..., n_in] -> float64 [..., n_out] on the host, row by row through the host entry `entry` of the bake's step
    parameters (litho_peb_param_chain or its transpose litho_peb_param_tangent) at the fixed step count."""
    t = torch.as_tensor(rows).detach().to(device="cpu", dtype=torch.float64)
    if t.shape[-1:] != (n_in,):
        raise ValueError(f"{who}: {what} must be [..., {n_in}]; got {tuple(t.shape)}")
    flat = t.reshape(-1, n_in)
    out = torch.empty((flat.shape[0], n_out), dtype=torch.float64)
    src, dst = (ctypes.c_double * n_in)(), (ctypes.c_double * n_out)()
    for i in range(flat.shape[0]):
        src[:] = flat[i].tolist()
        nat.check(getattr(nat.lib(), entry)(float(thickness), float(pixelSize), resist.kQuench, resist.kLoss, resist.acidDiffusionLength,
                                            resist.quencherDiffusionLength, resist.verticalScale, resist.bakeTime, int(D), int(steps), src, dst), entry)
        out[i] = torch.tensor(list(dst), dtype=torch.float64)
    return out.reshape(t.shape[:-1] + (n_out,))


def bakeParameterChain(gradStep, resist, thickness, pixelSize, D, steps):
    """gradStep [..., 6] (bakeStepGradient's) -> float64 [..., 5] on the host = dl/d(kQuench, kLoss, acidDiffusionLength,
    quencherDiffusionLength, verticalScale) at the fixed step count `steps` (litho_peb_param_chain, host arithmetic in double):
    the analytic derivative of lambda_xy = sigma^2 / (2 S pixel^2), lambda_z = (v sigma)^2 / (2 S hz^2), beta = kQuench dt and
    fl = exp(-kLoss dt), not the derivative of their rounding to fp32.  kQuench's is 0 for instantaneous neutralisation."""
    return _bake_rows("bakeParameterChain", "gradStep", gradStep, 6, 5, "litho_peb_param_chain", resist, thickness, pixelSize, D, steps)


def bakeParameterGradient(acid, resist, thickness, pixelSize, gradAcid=None, gradQuencher=None, gradAcidDose=None, steps=None, checkpointEvery=None):
    """The bake backwards down to the resist's parameters: returns (gradAcid0, gradQuencher0, params), the first two as
    bakeGradient returns them, bit for bit, and `params` a dict name -> float64 tensor [B] (one number per volume; a [D,n,n]
    input counts as B = 1) for quencher (gradQuencher0 summed over the volume), kQuench, kLoss, acidDiffusionLength,
    quencherDiffusionLength and verticalScale (bakeStepGradient through bakeParameterChain, at the step count of this call).
    bakeTime is a process setting and is not differentiated."""
    gh0, gq0, gs = bakeStepGradient(acid, resist, thickness, pixelSize, gradAcid, gradQuencher, gradAcidDose, steps, checkpointEvery)
    batched = acid.dim() == 4
    D = acid.shape[-3]
    S = _steps("bakeParameterGradient", resist, float(thickness), D, float(pixelSize), steps)
    chain = bakeParameterChain(gs if batched else gs[None], resist, thickness, pixelSize, D, S)
    q = (gq0 if batched else gq0[None]).double().sum(dim=(1, 2, 3)).cpu()
    params = {"quencher": q}
    for i, name in enumerate(BAKE_PARAMETERS):
        params[name] = chain[:, i].clone()
    return gh0, gq0, params


def _rate_sums(who, x, doses, kappa, mack, thickness, gradSlowness):
    """litho_develop_rate_vjp_params on x ([D,n,n] or [F,D,n,n]): float64 [len(doses) F, D, 6] on the device."""
    v, F, D, n, _, dev = _volume(who, x, "x")
    g, count = _gains(who, doses, F, D)
    gs = _like(who, "gradSlowness", gradSlowness, (count * F, D, n, n), dev)
    out = torch.empty((count * F, D, 6), dtype=torch.float64, device=dev)
    nbytes = int(nat.lib().litho_develop_rate_params_work_bytes(F, D, n, count))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nat.call(dev, "litho_develop_rate_vjp_params", nat.ptr(v), F, D, n, g, count, kappa, mack.rMax, mack.rMin, mack.q, mack.mTh, mack.surfaceRate,
             _surface_depth(mack, thickness), thickness, nat.ptr(gs), nat.ptr(out), nat.ptr(work), nbytes, keep=(v, gs, work))
    return out


def rateParameterChain(planeSums, mack, thickness):
    """planeSums float64 [G, D, 6] (the rate law's sums per gained plane) -> float64 [G, 7] on the host = dl/d(kappa, rMax, rMin, q,
    mTh, surfaceRate, surfaceDepth) per gained volume, the planes added in ascending order (litho_develop_rate_param_chain)."""
    s = torch.as_tensor(planeSums).detach().to(device="cpu", dtype=torch.float64).contiguous()
    if s.dim() != 3 or s.shape[-1] != 6:
        raise ValueError(f"rateParameterChain: planeSums must be [G, D, 6]; got {tuple(s.shape)}")
    G, D = int(s.shape[0]), int(s.shape[1])
    thickness = float(thickness)
    src = (ctypes.c_double * (G * D * 6))(*s.reshape(-1).tolist())
    dst = (ctypes.c_double * (G * 7))()
    nat.check(nat.lib().litho_develop_rate_param_chain(mack.rMax, mack.rMin, mack.q, mack.mTh, mack.surfaceRate, _surface_depth(mack, thickness),
                                                       thickness, D, G, src, dst), "litho_develop_rate_param_chain")
    return torch.tensor(list(dst), dtype=torch.float64).reshape(G, 7)


def rateParameterGradient(x, resist, thickness, gradSlowness, doses=(1.0,)):
    """The rate law backwards down to its parameters, for either resist: returns a dict name -> float64 tensor [len(doses) F] on
    the host, one number per gained volume, dose-major.  With a MackResist `x` is the intensity volume that the rate law sees
    ([D,n,n] or [F,D,n,n]; the DIFFUSED image when the resist diffuses) and the names are C, rMax, rMin, q, mTh; with a
    ChemicallyAmplifiedResist `x` is the acid dose, `doses` stays (1.0,) and the names are kAmp and resist.mack's rMax, rMin, q,
    mTh.  surfaceRate and surfaceDepth are added when the surface factor is switched on (surfaceDepth given).  gradSlowness fp32
    [len(doses) F, D, n, n] (a [D,n,n] one with a [D,n,n] x).  A wall contributes 0.  NOT built: the gradients of a MackResist's
    own Gaussian diffusion lengths."""
    who = "rateParameterGradient"
    thickness = _positive(who, "thickness", thickness)
    if isinstance(resist, ChemicallyAmplifiedResist):
        kappa, mack, first, doses = resist.kAmp, resist.mack, "kAmp", (1.0,)
    elif isinstance(resist, MackResist):
        kappa, mack, first = resist.C, resist, "C"
    else:
        raise TypeError(f"{who}: resist must be a MackResist or a ChemicallyAmplifiedResist")
    if isinstance(x, torch.Tensor) and x.dim() == 3 and isinstance(gradSlowness, torch.Tensor) and gradSlowness.dim() == 3:
        gradSlowness = gradSlowness[None]
    table = rateParameterChain(_rate_sums(who, x, doses, kappa, mack, thickness, gradSlowness), mack, thickness)
    out = {first: table[:, 0].clone()}
    for i, name in enumerate(_MACK):
        if name in ("surfaceRate", "surfaceDepth") and mack.surfaceDepth is None:
            continue
        out[name] = table[:, 1 + i].clone()
    return out


def exposureParameterGradient(image, C, doses, gradAcid):
    """dl/dC of exposeAcid (litho_peb_expose_vjp_params): float64 [len(doses) F] on the host, one number per gained volume,
    dose-major -- the sum over its cells of gradAcid (dose I) exp(-C dose I); gradAcid fp32 [len(doses) F, D, n, n] as exposeAcid
    returns the acid.  A cell whose acid is NaN contributes 0."""
    who = "exposureParameterGradient"
    v, F, D, n, _, dev = _volume(who, image)
    g, count = _gains(who, doses, F, D)
    ga = _like(who, "gradAcid", gradAcid, (count * F, D, n, n), dev)
    out = torch.empty(count * F, dtype=torch.float64, device=dev)
    nbytes = int(nat.lib().litho_peb_expose_params_work_bytes(F, D, n, count))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nat.call(dev, "litho_peb_expose_vjp_params", nat.ptr(v), F, D, n, g, count, _positive(who, "C", C), nat.ptr(ga), nat.ptr(out), nat.ptr(work),
             nbytes, keep=(v, ga, work))
    return out.cpu()


# ---- the chain from the arrival times ---------------------------------------------------------------------------------------------
class _Forward:
    """The forward chain of one resist on one intensity stack with everything its backward pass needs."""


def _forward(who, image, resist, stack_or_thickness, pixelSize, doses, focalPlanes, maxIterations, steps):
    thickness = stack_or_thickness.thickness if isinstance(stack_or_thickness, FilmStack) else float(stack_or_thickness)
    F = int(focalPlanes)
    if not isinstance(image, torch.Tensor) or image.dim() != 3 or F < 1 or image.shape[0] % F:
        raise ValueError(f"{who}: image must be [focalPlanes x D, n, n]; got {tuple(getattr(image, 'shape', ()))} with focalPlanes {focalPlanes}")
    f = _Forward()
    f.thickness, f.pixel, f.doses, f.F, f.maxIterations = _positive(who, "thickness", thickness), _positive(who, "pixelSize", pixelSize), tuple(doses), F, maxIterations
    f.D, f.n = image.shape[0] // F, image.shape[-1]
    f.vol = image.reshape(F, f.D, f.n, f.n)
    f.resist = resist
    if isinstance(resist, ChemicallyAmplifiedResist):
        f.h0 = exposeAcid(f.vol, resist.C, f.doses)
        _, _, f.dose, f.steps = bakeAcid(f.h0, resist, f.thickness, f.pixel, steps)
        _, f.slowness = amplifiedRate(f.dose, resist, f.thickness)
    elif isinstance(resist, MackResist):
        diffuses = resist.diffusionLength > 0.0 or resist.verticalDiffusionLength > 0.0
        f.lat = latentDiffusion(f.vol, f.thickness, f.pixel, resist.diffusionLength, resist.verticalDiffusionLength) if diffuses else f.vol
        f.slowness = developmentRate(f.vol, resist, f.thickness, f.pixel, f.doses)
    else:
        raise TypeError(f"{who}: resist must be a MackResist or a ChemicallyAmplifiedResist")
    f.T, _ = _development_time(f.slowness, f.thickness, f.pixel, maxIterations)
    return f


def _backward(who, f, gradT):
    """dict name -> float from the cotangent on f.T ([len(doses) F, D, n, n])."""
    gs = developmentTimeGradient(f.slowness, f.T, gradT, f.thickness, f.pixel, f.maxIterations)
    r = f.resist
    if isinstance(r, MackResist):
        return {k: float(v.sum()) for k, v in rateParameterGradient(f.lat, r, f.thickness, gs, f.doses).items()}
    out = {k: float(v.sum()) for k, v in rateParameterGradient(f.dose, r, f.thickness, gs).items()}
    ga = amplifiedRateGradient(f.dose, r, f.thickness, gs)
    gh0, _, params = bakeParameterGradient(f.h0, r, f.thickness, f.pixel, gradAcidDose=ga, steps=f.steps)
    out.update({k: float(v.sum()) for k, v in params.items()})
    out["C"] = float(exposureParameterGradient(f.vol, r.C, f.doses, gh0).sum())
    return out


def resistParameterGradient(image, resist, stack_or_thickness, pixelSize, gradT, doses=(1.0,), focalPlanes=1, maxIterations=1024, steps=None):
    """resistProfile backwards, from the arrival times to the resist's parameters: for a real loss l on ResistProfile.T with
    gradT = dl/dT, fp32 [doses, F, D, n, n], returns a dict name -> float (summed over doses and focal planes) for every
    differentiable parameter of `resist`: a MackResist's C, rMax, rMin, q, mTh; a ChemicallyAmplifiedResist's C, quencher, kAmp,
    kQuench, kLoss, acidDiffusionLength, quencherDiffusionLength, verticalScale and its mack's rMax, rMin, q, mTh; surfaceRate
    and surfaceDepth when the surface factor is on.  The chain of resistProfileGradient with the parameter reductions at each
    stage: the rate parameters from gradSlowness, the bake's from gradAcidDose, C from gradAcid0.  kAmp comes from the rate stage
    alone: the slowness depends on it only through m = exp(-kAmp a).  `steps`: the bake's step count, held fixed (None: the
    default of postExposureBake, as resistProfile).  gradT is ignored where T is +inf."""
    who = "resistParameterGradient"
    f = _forward(who, image, resist, stack_or_thickness, pixelSize, doses, focalPlanes, maxIterations, steps)
    dev = nat.require_gpu(image.device)
    g = _like(who, "gradT", gradT, (len(f.doses), f.F, f.D, f.n, f.n), dev).reshape(len(f.doses) * f.F, f.D, f.n, f.n)
    return _backward(who, f, g)


def resistArrivalTimes(image, resist, stack_or_thickness, pixelSize, doses=(1.0,), focalPlanes=1, steps=None, maxIterations=1024):
    """The arrival times of resistProfile, fp32 [doses, F, D, n, n], with the bake's step count given: what calibrateResist and
    resistParameterGradient differentiate (steps=None: the default of postExposureBake, and then ResistProfile.T bit for bit).
    ResistProfile(T, None, 0, thickness, pixelSize, developTime, doses).cd(gauges) measures CDs on it."""
    f = _forward("resistArrivalTimes", image, resist, stack_or_thickness, pixelSize, doses, focalPlanes, maxIterations, steps)
    return f.T.reshape(len(f.doses), f.F, f.D, f.n, f.n)


def resistWith(resist, **values):
    """A copy of `resist` (a MackResist or a ChemicallyAmplifiedResist) with the named parameters replaced; the parameters of a
    ChemicallyAmplifiedResist's mack (rMax, rMin, q, mTh, surfaceRate, surfaceDepth) are addressed by their own names."""
    known = (_BAKED + _MACK) if isinstance(resist, ChemicallyAmplifiedResist) else (("C",) + _MACK)
    for name in values:
        if name not in known:
            raise ValueError(f"resistWith: {name!r} is not a parameter of a {type(resist).__name__}; known: {', '.join(known)}")
    return _replace(resist, values)


def resistParameter(resist, name):
    """The value of the named parameter, a ChemicallyAmplifiedResist's mack included."""
    return _get(resist, name)


# ---- calibration ------------------------------------------------------------------------------------------------------------------
_DOMAIN = {"q": (1.0 + 1e-6, math.inf), "mTh": (0.0, 1.0 - 1e-6), "surfaceRate": (1e-6, 1.0)}


def _get(resist, name):
    if isinstance(resist, ChemicallyAmplifiedResist) and name in _MACK:
        return getattr(resist.mack, name)
    return getattr(resist, name)


def _replace(resist, values):
    """A copy of `resist` with the parameters of the dict `values` replaced."""
    def mack(m):
        kw = {k: values.get(k, getattr(m, k)) for k in ("rMax", "rMin", "q", "mTh", "surfaceRate", "surfaceDepth")}
        return MackResist(C=values.get("C", m.C) if isinstance(resist, MackResist) else m.C, diffusionLength=m.diffusionLength,
                          verticalDiffusionLength=m.verticalDiffusionLength, **kw)
    if isinstance(resist, MackResist):
        return mack(resist)
    kw = {k: values.get(k, getattr(resist, k)) for k in _BAKED}
    return ChemicallyAmplifiedResist(bakeTime=resist.bakeTime, mack=mack(resist.mack), **kw)


def _edge_points(who, measurements, nd, F, D, n, pixel, dev):
    """The two edge points of every measured CD as bilinear stencils on T [nd F, D, n, n]: (volume, plane, row, col) index tensors
    [P, 4] and weights [P, 4]."""
    vol, pl, rows, cols, wts = [], [], [], [], []
    for m in measurements:
        di, fi, zi, gauge, cd = m
        row, col, axis = float(gauge[0]), float(gauge[1]), int(gauge[2])
        cd = float(cd)
        if not (0 <= int(di) < nd and 0 <= int(fi) < F and 0 <= int(zi) < D and 0 <= row <= n - 1 and 0 <= col <= n - 1 and axis in (0, 1)
                and cd > 0.0 and math.isfinite(cd)):
            raise ValueError(f"{who}: a measurement is (dose index, focal index, depth index, (row, col, axis), CD in nm) inside the "
                             f"stack, with a positive CD; got {m}")
        for sign in (-1.0, 1.0):
            y, x = row, col
            if axis == 0:
                x += sign * 0.5 * cd / pixel
            else:
                y += sign * 0.5 * cd / pixel
            y, x = min(max(y, 0.0), n - 1.0), min(max(x, 0.0), n - 1.0)
            y0, x0 = min(int(math.floor(y)), max(n - 2, 0)), min(int(math.floor(x)), max(n - 2, 0))
            fy, fx = y - y0, x - x0
            y1, x1 = min(y0 + 1, n - 1), min(x0 + 1, n - 1)
            vol.append([int(di) * F + int(fi)] * 4)
            pl.append([int(zi)] * 4)
            rows.append([y0, y0, y1, y1])
            cols.append([x0, x1, x0, x1])
            wts.append([(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx])
    ix = [torch.tensor(a, dtype=torch.long, device=dev) for a in (vol, pl, rows, cols)]
    return ix, torch.tensor(wts, dtype=torch.float32, device=dev)


def _edge_residuals(T, t, ix, w):
    """(residuals [P], live [P, 4]): min(T~, 2 t) / t - 1 per edge point, and which of its four cells take a derivative."""
    reached = ~torch.isposinf(T)
    near = torch.where(reached, T, torch.full_like(T, 2.0 * t + 1.0))[ix[0], ix[1], ix[2], ix[3]]      # [P, 4]
    sample = (near * w).sum(dim=1)
    res = torch.clamp(sample, max=2.0 * t) / t - 1.0
    live = (sample < 2.0 * t)[:, None] & reached[ix[0], ix[1], ix[2], ix[3]]
    return res, live


def _edge_loss(T, developTime, ix, w):
    """(loss, dl/dT): the mean over the edge points of (min(T~, 2 t) / t - 1)^2, T~ the bilinear sample of T with +inf read as
    2 t + 1 (ResistProfile.clampedT, what the CDs were measured on).  No gradient goes to a cell that was never reached."""
    t = float(developTime)
    res, live = _edge_residuals(T, t, ix, w)
    loss = float((res.double() ** 2).mean())
    coef = (2.0 / (res.numel() * t)) * res[:, None] * w * live
    grad = torch.zeros_like(T).index_put_(tuple(i.reshape(-1) for i in ix), coef.reshape(-1).to(T.dtype), accumulate=True)
    return loss, grad


def _levenberg_marquardt(who, run, measurements, t, names, start, lo, hi, logs, iterations, dev):
    """calibrateResist's method="lm": (best values or None, history).  run(values) is the forward chain at those values."""
    import numpy as np

    from .tangent import _jacobian
    to_z = lambda k, v: math.log(v) if logs[k] else v                             # noqa: E731
    from_z = lambda k, z: math.exp(z) if logs[k] else z                           # noqa: E731
    values, best, best_values, points, history, mu, moved = dict(start), None, None, None, [], 1e-3, 0.0
    A = g = None
    for it in range(iterations + 1):
        f = run(values)
        if points is None:
            points = _edge_points(who, measurements, len(f.doses), f.F, f.D, f.n, f.pixel, dev)
        loss = _edge_loss(f.T, t, *points)[0]
        accepted = math.isfinite(loss) and (best is None or loss < best)
        history.append(dict(loss=loss, parameters=dict(values), step=moved, accepted=accepted, damping=mu))
        if accepted:
            best, best_values = loss, dict(values)
            r, J = _jacobian(who, f, t, points, names, logs)
            J, r = J.numpy(), r.numpy()
            A, g = J.T @ J, J.T @ r
            if it:
                mu = max(mu / 10.0, 1e-12)
        else:
            mu *= 10.0
        if it == iterations or best is None or mu > 1e12 or not np.isfinite(A).all() or not np.any(g != 0.0):
            break
        diag = np.diag(A)
        move = diag > 0.0                                                         # a parameter whose column is zero does not move
        delta = np.zeros(len(names))
        delta[move] = np.linalg.solve((A + mu * np.diag(diag))[np.ix_(move, move)], -g[move])
        moved = float(np.abs(delta).max())
        for i, k in enumerate(names):
            z = min(max(to_z(k, best_values[k]) + delta[i], to_z(k, lo[k])), to_z(k, hi[k]))        # clipped in z: exp cannot overflow
            values[k] = min(max(from_z(k, z), lo[k]), hi[k])
    return best_values, history


def calibrateResist(image, resist, stack_or_thickness, pixelSize, developTime, measurements, parameters=None, bounds=None, doses=(1.0,),
                    focalPlanes=1, iterations=20, steps=None, step=0.1, maxIterations=1024, method="descent"):
    """Fit resist parameters to measured CDs through dose and focus by steepest descent with backtracking, the resist-side twin of
    fitAberrations.  Returns (resist, history): the resist with the lowest loss and one record per evaluated iterate,
    dict(loss, parameters, step, accepted).

    `image` fp32 [focalPlanes x D, n, n] as resistProfile takes it, `resist` the starting point (a MackResist or a
    ChemicallyAmplifiedResist).  `measurements`: a list of (dose index, focal index, depth index, gauge, CD in nm), the gauge a
    (row, col, axis) triple as ResistProfile.cd takes it; here row and col may be fractional, the centre of the measured feature
    in pixels.  Each measured CD gives two edge points on its gauge, that centre -/+ CD / 2 along its axis.  Loss: the mean over the edge points of (min(T~, 2 developTime) / developTime - 1)^2, T~ the
    bilinear sample of T at the point (+inf read as 2 developTime + 1, as ResistProfile.cd does) -- it says that the printed contour
    T = developTime passes through the measured edges, and it is 0 for the resist that printed them.
    dl/dT is the bilinear scatter of the residuals (torch on the device), and resistParameterGradient's chain takes it to the
    parameters.

    `parameters`: the names to fit (None: kAmp and acidDiffusionLength of a ChemicallyAmplifiedResist, C and rMax of a MackResist).
    `bounds`: dict name -> (low, high); a name left out gets (value / 2, 2 value) inside the parameter's domain.  The descent
    runs on the logarithm of a parameter that starts positive and on the value itself of one that starts at 0:
    z <- clip(z - step . grad_z / max|grad_z|), so `step` is a relative change.  An iterate whose loss is not below the best so
    far is not accepted: the loop returns to the best iterate and halves `step`; an accepted one doubles it again, up to
    the value given.  The bake's step count is one integer for the
    whole fit: `steps`, or max(8, minSteps at the upper bounds of the diffusion lengths and of verticalScale).

    method="lm": Levenberg-Marquardt on the same coordinates z, bounds and step count, with the Jacobian J of the residuals from
    the forward mode (tangent.py: one forward run and one tangent sweep per accepted iterate, no tape).  delta solves
    (J^T J + mu diag(J^T J)) delta = -J^T r in float64 on the host, a parameter whose column is zero does not move, and
    z <- clip(z + delta).  mu starts at 1e-3 and is divided by 10 on an accepted iterate (floor 1e-12); on a rejected one it is
    multiplied by 10 and the loop returns to the best iterate.  It stops after `iterations`, on J^T r = 0, or when mu exceeds
    1e12.  Each record also carries `damping`, the mu the iterate was computed with; `step` is max |delta| of that move.  Any
    other `method` raises ValueError.

    Raises ValueError for kQuench of a resist with instantaneous neutralisation, for a parameter the resist class does not have,
    and for surfaceRate or surfaceDepth with the surface factor switched off."""
    who = "calibrateResist"
    if method not in ("descent", "lm"):
        raise ValueError(f"{who}: method must be 'descent' or 'lm'; got {method!r}")
    car = isinstance(resist, ChemicallyAmplifiedResist)
    if not car and not isinstance(resist, MackResist):
        raise TypeError(f"{who}: resist must be a MackResist or a ChemicallyAmplifiedResist")
    names = list(parameters) if parameters is not None else (["kAmp", "acidDiffusionLength"] if car else ["C", "rMax"])
    known = (_BAKED + _MACK) if car else (("C",) + _MACK)
    mack = resist.mack if car else resist
    if not names or len(set(names)) != len(names):
        raise ValueError(f"{who}: parameters must name at least one parameter, each once; got {names}")
    for name in names:
        if name not in known:
            raise ValueError(f"{who}: {name!r} is not a differentiable parameter of a {type(resist).__name__}; known: {', '.join(known)}")
        if name in ("surfaceRate", "surfaceDepth") and mack.surfaceDepth is None:
            raise ValueError(f"{who}: {name} cannot be fitted with the surface factor switched off (surfaceDepth is None)")
        if name == "kQuench" and math.isinf(resist.kQuench):
            raise ValueError(f"{who}: kQuench of a resist with instantaneous neutralisation (kQuench = inf) cannot be fitted")
    iterations, step, t = int(iterations), float(step), float(developTime)
    if iterations < 1 or not step > 0 or not (t > 0.0 and math.isfinite(t)):
        raise ValueError(f"{who}: iterations >= 1, step > 0 and a positive finite developTime; got {iterations}, {step}, {developTime}")
    if not measurements:
        raise ValueError(f"{who}: give at least one measurement")
    start = {name: float(_get(resist, name)) for name in names}
    lo, hi, logs = {}, {}, {}
    for name in names:
        v = start[name]
        d_lo, d_hi = _DOMAIN.get(name, (0.0, math.inf))
        low, high = (bounds or {}).get(name, (0.5 * v, 2.0 * v) if v > 0.0 else (0.0, 1.0))
        lo[name], hi[name] = max(float(low), d_lo), min(float(high), d_hi)
        if not lo[name] <= v <= hi[name]:
            raise ValueError(f"{who}: {name} = {v} starts outside its bounds ({lo[name]}, {hi[name]})")
        logs[name] = v > 0.0 and lo[name] > 0.0
    thickness = stack_or_thickness.thickness if isinstance(stack_or_thickness, FilmStack) else float(stack_or_thickness)
    if car and steps is None:
        top = _replace(resist, {k: hi[k] for k in ("acidDiffusionLength", "quencherDiffusionLength", "verticalScale") if k in hi})
        steps = max(8, top.minSteps(thickness, image.shape[0] // int(focalPlanes), float(pixelSize)))
    dev = nat.require_gpu(image.device)
    doses = tuple(doses)
    if method == "lm":
        run = lambda values: _forward(who, image, _replace(resist, values), thickness, pixelSize, doses, focalPlanes, maxIterations,   # noqa: E731
                                      steps if car else None)
        best_values, history = _levenberg_marquardt(who, run, measurements, t, names, start, lo, hi, logs, iterations, dev)
        if best_values is None:
            raise RuntimeError(f"{who}: the loss at the starting point is not finite")
        return _replace(resist, best_values), history
    values, best, best_values, points, history, direction, first_step = dict(start), None, None, None, [], None, step
    for it in range(iterations + 1):
        trial = _replace(resist, values)
        f = _forward(who, image, trial, thickness, pixelSize, doses, focalPlanes, maxIterations, steps if car else None)
        if points is None:
            points = _edge_points(who, measurements, len(doses), f.F, f.D, f.n, f.pixel, dev)
        loss, gradT = _edge_loss(f.T, t, *points)
        accepted = math.isfinite(loss) and (best is None or loss < best)
        history.append(dict(loss=loss, parameters=dict(values), step=step, accepted=accepted))
        if accepted:
            best, best_values = loss, dict(values)
            g = _backward(who, f, gradT)
            direction = {k: g[k] * (best_values[k] if logs[k] else 1.0) for k in names}
            if it:
                step = min(2.0 * step, first_step)                              # the next trial starts longer again
        else:
            step *= 0.5
        if it == iterations or best is None:
            break
        top = max(abs(d) for d in direction.values())
        if not (top > 0.0 and math.isfinite(top)):
            break
        for k in names:
            move = step * direction[k] / top
            v = best_values[k] * math.exp(-move) if logs[k] else best_values[k] - move
            values[k] = min(max(v, lo[k]), hi[k])
    if best is None:
        raise RuntimeError(f"{who}: the loss at the starting point is not finite")
    return _replace(resist, best_values), history
