"""Forward mode (tangents) of the resist chain: how the exposure, the bake, the rate and the development front move when the
resist's parameters, or the image, move; no reference counterpart (include/litho_abbe.h: "Forward mode (tangents) of the resist
chain"; csrc/peb.hip, csrc/develop_grad.hip).

The adjoint calls of peb.py, develop.py and calibrate.py give one ROW of a Jacobian per sweep, with a tape.  These give one COLUMN
per direction, without a tape, and up to 16 directions share one primal run in one launch -- what a Gauss-Newton or
Levenberg-Marquardt step on a handful of parameters and many residuals needs:
  exposeAcidTangent                            litho_peb_expose_jvp
  bakeTangent, bakeParameterTangent            litho_peb_bake_jvp; the host chain kQuench, kLoss, ... -> the six step parameters
  developmentRateTangent, amplifiedRateTangent litho_develop_rate_jvp for kappa = C and kappa = kAmp
  rateParameterTangent                         the host chain kappa, rMax, ... -> the six slots of the rate law per plane
  developmentTimeTangent                       litho_develop_time_jvp, the tangent of the Godunov fixed point
  resistProfileTangent                         their chain: dT / d(direction), fp32 [P, doses, F, D, n, n], for either resist
  calibrationJacobian                          the residuals of calibrateResist's loss and their Jacobian
Tangent volumes are direction-major, [P, ...].  A direction alone has the bits it has inside a batch of P; two calls give the same
bits.  The bake's step count is held fixed, as in calibrate.py.

NOT built: forward mode through the optics (mask -> image: `imageTangent` is taken as given), dCD / d(theta) as its own call (it
follows from dT at the edge points; calibrationJacobian does that for its residuals), a fused multi-step tangent kernel."""
import ctypes

import torch

from . import _native as nat
from .calibrate import _BAKED, _MACK, BAKE_PARAMETERS, _bake_rows, _edge_points, _edge_residuals, _forward
from .develop import MackResist, _gains, _like, _positive, _surface_depth, _volume, latentDiffusion
from .peb import ChemicallyAmplifiedResist, _bake_scalars, _steps

MAX_DIRECTIONS = 16
RATE_PARAMETERS = ("kappa",) + _MACK


def _directions(who, name, t, P, shape, dev):
    """None, or a float32 tensor [P, *shape] on dev, detached and contiguous."""
    if t is None:
        return None
    return _like(who, name, t, (P,) + tuple(shape), dev)


def _count(who, P, planes):
    if not 1 <= P <= MAX_DIRECTIONS:
        raise ValueError(f"{who}: between 1 and {MAX_DIRECTIONS} directions per call; got {P}")
    if P * planes > 65535:
        raise ValueError(f"{who}: directions x volumes x planes exceeds 65535")


def _doubles(who, name, values, shape):
    """Host doubles of exactly `shape` as a flat ctypes array."""
    t = torch.as_tensor(values, dtype=torch.float64).detach().cpu()
    if tuple(t.shape) != tuple(shape) or not bool(torch.isfinite(t).all()):
        raise ValueError(f"{who}: {name} must be finite numbers of shape {tuple(shape)}; got shape {tuple(t.shape)}")
    flat = t.reshape(-1).tolist()
    return (ctypes.c_double * len(flat))(*flat)


def exposeAcidTangent(image, C, doses, dC, dImage=None):
    """The tangent of exposeAcid (litho_peb_expose_jvp): for the P directions (dC[p], dImage[p]) returns dAcid fp32
    [P, len(doses) F, D, n, n] = exp(-C dose I) ((dose I) dC + (C dose) dImage), dose-major inside a direction as exposeAcid's
    acid; exactly 0 where the acid is NaN.  `dC`: P numbers; `dImage`: fp32 [P, F, D, n, n] ([P, D, n, n] with a [D,n,n] image)
    or None = zero."""
    who = "exposeAcidTangent"
    v, F, D, n, batched, dev = _volume(who, image)
    g, count = _gains(who, doses, F, D)
    P = len(dC)
    _count(who, P, count * F * D)
    dc = _doubles(who, "dC", dC, (P,))
    dI = _directions(who, "dImage", dImage, P, v.shape if batched else v.shape[1:], dev)
    out = torch.empty((P, count * F, D, n, n), dtype=torch.float32, device=dev)
    nat.call(dev, "litho_peb_expose_jvp", nat.ptr(v), F, D, n, g, count, _positive(who, "C", C), P, dc, nat.ptr(dI) if dI is not None else None,
             nat.ptr(out), keep=(v, dI))
    return out


def bakeParameterTangent(dParam, resist, thickness, pixelSize, D, steps):
    """dParam [..., 5] = d(kQuench, kLoss, acidDiffusionLength, quencherDiffusionLength, verticalScale) -> float64 [..., 6] on the
    host = d(lxy_h, lz_h, lxy_q, lz_q, beta, fl) at the fixed step count `steps` (litho_peb_param_tangent): the transpose of
    bakeParameterChain.  0 for a zero length or scale and for instantaneous neutralisation."""
    return _bake_rows("bakeParameterTangent", "dParam", dParam, 5, 6, "litho_peb_param_tangent", resist, thickness, pixelSize, D, steps)


def bakeTangent(acid, resist, thickness, pixelSize, dAcid=None, dQuencher=None, dStep=None, steps=None, returnPrimal=False):
    """The bake with its tangent (litho_peb_bake_jvp): returns (dAcid, dQuencher, dAcidDose), each fp32 [P, B, D, n, n] ([P, D, n, n]
    for a [D,n,n] input), the derivatives of bakeAcid's three outputs along P directions.  A direction is (dAcid[p], the initial
    acid's, fp32 [P, *acid.shape] or None = zero; dQuencher[p], the quencher loading's, P numbers or None; dStep[p], fp32-rounded
    d(lxy_h, lz_h, lxy_q, lz_q, beta, fl), [P, 6] or None -- bakeParameterTangent makes them from the physical parameters).  At
    least one of the three is given; P is its leading length.  No tape: the workspace is 5 + 2 P volumes whatever `steps`.
    returnPrimal=True appends (acid, quencher, acidDose), which are bakeAcid's bits."""
    who = "bakeTangent"
    if not isinstance(resist, ChemicallyAmplifiedResist):
        raise TypeError(f"{who}: resist must be a ChemicallyAmplifiedResist")
    v, B, D, n, batched, dev = _volume(who, acid, "acid")
    thickness, h = _positive(who, "thickness", thickness), _positive(who, "pixelSize", pixelSize)
    S = _steps(who, resist, thickness, D, h, steps)
    given = [len(x) for x in (dAcid, dQuencher, dStep) if x is not None]
    if not given or len(set(given)) != 1:
        raise ValueError(f"{who}: give at least one of dAcid, dQuencher, dStep, all with the same number of directions")
    P = given[0]
    _count(who, P, B * D)
    dh = _directions(who, "dAcid", dAcid, P, v.shape if batched else v.shape[1:], dev)
    dq = _doubles(who, "dQuencher", dQuencher if dQuencher is not None else [0.0] * P, (P,))
    ds = _doubles(who, "dStep", dStep if dStep is not None else [[0.0] * 6] * P, (P, 6))
    prim = [torch.empty_like(v) for _ in range(3)] if returnPrimal else [None] * 3
    out = [torch.empty((P,) + tuple(v.shape), dtype=torch.float32, device=dev) for _ in range(3)]
    nbytes = int(nat.lib().litho_peb_jvp_work_bytes(B, D, n, P))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    opt = lambda t: nat.ptr(t) if t is not None else None                       # noqa: E731
    nat.call(dev, "litho_peb_bake_jvp", nat.ptr(v), B, D, n, thickness, h, *_bake_scalars(resist), S, P, opt(dh), dq, ds, opt(prim[0]),
             opt(prim[1]), opt(prim[2]), nat.ptr(out[0]), nat.ptr(out[1]), nat.ptr(out[2]), nat.ptr(work), nbytes, keep=(v, dh, work))
    if not batched:
        out, prim = [t[:, 0] for t in out], [t[0] if t is not None else None for t in prim]
    return tuple(out) + (tuple(prim) if returnPrimal else ())


def rateParameterTangent(dParam, mack, thickness, D):
    """dParam [P, 7] = d(kappa, rMax, rMin, q, mTh, surfaceRate, surfaceDepth) -> float64 [P, D, 6] on the host: the directions of
    the rate law's six slots per plane (litho_develop_rate_param_tangent), the transpose of rateParameterChain.  kappa is C of a
    MackResist and kAmp of a ChemicallyAmplifiedResist."""
    who = "rateParameterTangent"
    d = torch.as_tensor(dParam).detach().to(device="cpu", dtype=torch.float64)
    if d.dim() != 2 or d.shape[1] != 7:
        raise ValueError(f"{who}: dParam must be [P, 7]; got {tuple(d.shape)}")
    thickness, D = float(thickness), int(D)
    delta = _surface_depth(mack, thickness)
    out = torch.empty((d.shape[0], D, 6), dtype=torch.float64)
    src, dst = (ctypes.c_double * 7)(), (ctypes.c_double * (max(D, 1) * 6))()
    for i in range(d.shape[0]):
        src[:] = d[i].tolist()
        nat.check(nat.lib().litho_develop_rate_param_tangent(mack.rMax, mack.rMin, mack.q, mack.mTh, mack.surfaceRate, delta, thickness, D, src,
                                                             dst), "litho_develop_rate_param_tangent")
        out[i] = torch.tensor(list(dst), dtype=torch.float64).reshape(D, 6)
    return out


def _rate_jvp(who, x, doses, kappa, mack, thickness, dX, dPhi):
    v, F, D, n, batched, dev = _volume(who, x, "x")
    g, count = _gains(who, doses, F, D)
    given = [len(t) for t in (dX, dPhi) if t is not None]
    if not given or len(set(given)) != 1:
        raise ValueError(f"{who}: give at least one of the volume's direction and dPhi, with the same number of directions")
    P = given[0]
    _count(who, P, count * F * D)
    dx = _directions(who, "the volume's direction", dX, P, v.shape if batched else v.shape[1:], dev)
    phi = torch.zeros((P, D, 6), dtype=torch.float64) if dPhi is None else torch.as_tensor(dPhi).detach().to(device="cpu", dtype=torch.float64)
    if tuple(phi.shape) != (P, D, 6) or not bool(torch.isfinite(phi).all()):
        raise ValueError(f"{who}: dPhi must be finite numbers [P, D, 6] = {(P, D, 6)}; got {tuple(phi.shape)}")
    phi = phi.contiguous().to(dev)
    out = torch.empty((P, count * F, D, n, n), dtype=torch.float32, device=dev)
    nat.call(dev, "litho_develop_rate_jvp", nat.ptr(v), F, D, n, g, count, kappa, mack.rMax, mack.rMin, mack.q, mack.mTh, mack.surfaceRate,
             _surface_depth(mack, thickness), thickness, P, nat.ptr(dx) if dx is not None else None, nat.ptr(phi), nat.ptr(out), keep=(v, dx, phi))
    return out


def developmentRateTangent(x, resist, thickness, doses=(1.0,), dX=None, dPhi=None):
    """The tangent of a MackResist's rate law (litho_develop_rate_jvp, kappa = C): dSlowness fp32 [P, len(doses) F, D, n, n].  `x` is
    the intensity volume the rate law sees ([D,n,n] or [F,D,n,n]; the DIFFUSED image when the resist diffuses), `dX` its
    directions, fp32 [P, *x.shape] or None; `dPhi` float64 [P, D, 6], the directions of the six slots (rateParameterTangent), or
    None.  A wall gives exactly 0."""
    who = "developmentRateTangent"
    if not isinstance(resist, MackResist):
        raise TypeError(f"{who}: resist must be a MackResist")
    return _rate_jvp(who, x, doses, resist.C, resist, _positive(who, "thickness", thickness), dX, dPhi)


def amplifiedRateTangent(acidDose, resist, thickness, dAcidDose=None, dPhi=None):
    """The tangent of amplifiedRate's slowness (litho_develop_rate_jvp with kappa = kAmp and a single gain of 1): dSlowness fp32
    [P, B, D, n, n] from dAcidDose fp32 [P, *acidDose.shape] (or None) and dPhi float64 [P, D, 6] (or None)."""
    who = "amplifiedRateTangent"
    if not isinstance(resist, ChemicallyAmplifiedResist):
        raise TypeError(f"{who}: resist must be a ChemicallyAmplifiedResist")
    return _rate_jvp(who, acidDose, [1.0], resist.kAmp, resist.mack, _positive(who, "thickness", thickness), dAcidDose, dPhi)


def developmentTimeTangent(slowness, T, dSlowness, thickness, pixelSize, maxIterations=1024, returnLaunches=False):
    """The tangent of developmentTime (litho_develop_time_jvp): dT fp32 [P, *slowness.shape] from dSlowness alike.  `T` must be what
    developmentTime returned for this slowness, thickness and pixelSize.  Every reached cell takes sigma dSlowness of its own and
    the dT of the upwind cells of its update with the weights alpha of developmentTimeGradient -- its transpose; a wall or a cell
    the front never reached gets exactly 0 whatever its dSlowness holds.  Iterates to a bitwise fixed point and waits for the
    device while it does; RuntimeError if `maxIterations` launches do not reach it.  Deterministic: the same bits in two calls,
    for a direction alone or among P, for a volume alone or in a batch.  returnLaunches=True returns (dT, launches)."""
    who = "developmentTimeTangent"
    s, B, D, n, batched, dev = _volume(who, slowness, "slowness")
    thickness, h = _positive(who, "thickness", thickness), _positive(who, "pixelSize", pixelSize)
    maxIterations = int(maxIterations)
    if not 1 <= maxIterations <= 65536:
        raise ValueError(f"{who}: maxIterations must be 1 ... 65536; got {maxIterations}")
    Tv = _like(who, "T", T, slowness.shape, dev).reshape(s.shape)
    if not isinstance(dSlowness, torch.Tensor) or dSlowness.dim() != slowness.dim() + 1:
        raise ValueError(f"{who}: dSlowness must be a float32 tensor [P, *slowness.shape]")
    P = int(dSlowness.shape[0])
    _count(who, P, B * D)
    ds = _directions(who, "dSlowness", dSlowness, P, slowness.shape, dev)
    out = torch.empty((P,) + tuple(s.shape), dtype=torch.float32, device=dev)
    nbytes = int(nat.lib().litho_develop_jvp_work_bytes(B, D, n, P, maxIterations))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    launches = ctypes.c_int(0)
    nat.call(dev, "litho_develop_time_jvp", nat.ptr(s), nat.ptr(Tv), nat.ptr(ds), B, D, n, P, thickness, h, maxIterations, nat.ptr(out),
             nat.ptr(work), nbytes, ctypes.byref(launches), keep=(s, Tv, ds, work),
             noconv=f"{who}: the tangent iteration did not reach its fixed point within the launch cap (maxIterations = {maxIterations}); "
                    "the tangent is not a result")
    out = out if batched else out[:, 0]
    return (out, launches.value) if returnLaunches else out


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
def _names(resist):
    """The parameter names resistParameterGradient returns for this resist."""
    car = isinstance(resist, ChemicallyAmplifiedResist)
    mack = resist.mack if car else resist
    law = tuple(k for k in _MACK if mack.surfaceDepth is not None or k not in ("surfaceRate", "surfaceDepth"))
    return (_BAKED if car else ("C",)) + law


def _tangent_slice(f, directions, imageTangent):
    """dT [P, doses F, D, n, n] of the forward run f for at most MAX_DIRECTIONS directions."""
    r, P = f.resist, len(directions)
    col = lambda names: [[float(d.get(k, 0.0)) for k in names] for d in directions]      # noqa: E731
    if isinstance(r, ChemicallyAmplifiedResist):
        dI = imageTangent.reshape(P, f.F, f.D, f.n, f.n) if imageTangent is not None else None
        dh0 = exposeAcidTangent(f.vol, r.C, f.doses, [d.get("C", 0.0) for d in directions], dI)
        dstep = bakeParameterTangent(col(BAKE_PARAMETERS), r, f.thickness, f.pixel, f.D, f.steps)
        _, _, da = bakeTangent(f.h0, r, f.thickness, f.pixel, dAcid=dh0, dQuencher=[d.get("quencher", 0.0) for d in directions], dStep=dstep,
                               steps=f.steps)
        dphi = rateParameterTangent(col(("kAmp",) + _MACK), r.mack, f.thickness, f.D)
        ds = amplifiedRateTangent(f.dose, r, f.thickness, dAcidDose=da, dPhi=dphi)
    else:
        dlat = None
        if imageTangent is not None:
            dlat = imageTangent.reshape(P * f.F, f.D, f.n, f.n)
            if r.diffusionLength > 0.0 or r.verticalDiffusionLength > 0.0:                # the diffusion is linear
                dlat = latentDiffusion(dlat, f.thickness, f.pixel, r.diffusionLength, r.verticalDiffusionLength)
            dlat = dlat.reshape(P, f.F, f.D, f.n, f.n)
        dphi = rateParameterTangent(col(("C",) + _MACK), r, f.thickness, f.D)
        ds = developmentRateTangent(f.lat, r, f.thickness, f.doses, dX=dlat, dPhi=dphi)
    return developmentTimeTangent(f.slowness, f.T, ds, f.thickness, f.pixel, f.maxIterations)


def _profile_tangent(who, f, directions, imageTangent):
    names = _names(f.resist)
    directions = list(directions)
    if not directions:
        raise ValueError(f"{who}: give at least one direction")
    for d in directions:
        for k in d:
            if k not in names:
                raise ValueError(f"{who}: {k!r} is not a differentiable parameter of this {type(f.resist).__name__}; known: {', '.join(names)}")
    P = len(directions)
    if imageTangent is not None:
        dev = nat.require_gpu(f.vol.device)
        imageTangent = _like(who, "imageTangent", imageTangent, (P, f.F * f.D, f.n, f.n), dev)
    per = min(MAX_DIRECTIONS, 65535 // (len(f.doses) * f.F * f.D))
    if per < 1:
        raise ValueError(f"{who}: doses x focal planes x planes exceeds 65535")
    parts = [_tangent_slice(f, directions[i:i + per], imageTangent[i:i + per] if imageTangent is not None else None)
             for i in range(0, P, per)]
    dT = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
    return dT.reshape(P, len(f.doses), f.F, f.D, f.n, f.n)


def resistProfileTangent(image, resist, stack_or_thickness, pixelSize, directions, imageTangent=None, doses=(1.0,), focalPlanes=1, steps=None,
                         maxIterations=1024):
    """How the arrival times of resistProfile move: dT fp32 [P, doses, F, D, n, n], one per direction.  `directions`: a list of
    dicts {parameter name: d value} over the names resistParameterGradient returns for `resist` (a name left out is 0), so
    [{"kAmp": 1.0}] is dT / dkAmp; `imageTangent` fp32 [P, focalPlanes x D, n, n] or None: a direction of the intensity stack
    per direction (with a MackResist it goes through latentDiffusion, which is linear).  The forward chain runs once and is
    shared; more than 16 directions are run in slices.  `steps`: the bake's step count, held fixed (None: postExposureBake's
    default).  For a cotangent gradT on T, sum(gradT dT[k]) is resistParameterGradient(gradT)'s entry for direction k -- the
    two are transposes, stage by stage.  dT is exactly 0 where T is +inf."""
    who = "resistProfileTangent"
    f = _forward(who, image, resist, stack_or_thickness, pixelSize, doses, focalPlanes, maxIterations, steps)
    return _profile_tangent(who, f, directions, imageTangent)


def _jacobian(who, f, developTime, points, names, logs=None):
    """(residuals float64 [N], J float64 [N, P]) of the edge residuals of the forward run f; with `logs`, the columns of the
    parameters it marks are with respect to the logarithm of the parameter."""
    from .calibrate import _get
    t = float(developTime)
    ix, w = points
    res, live = _edge_residuals(f.T, t, ix, w)
    dT = _profile_tangent(who, f, [{k: 1.0} for k in names], None).reshape((len(names),) + tuple(f.T.shape))
    near = dT[:, ix[0], ix[1], ix[2], ix[3]].double()                                  # [P, N, 4]
    J = ((near * (w * live).double()[None]).sum(dim=2) / t).T.contiguous().cpu()
    if logs is not None:
        J = J * torch.tensor([float(_get(f.resist, k)) if logs[k] else 1.0 for k in names], dtype=torch.float64)[None]
    return res.double().cpu(), J


def calibrationJacobian(image, resist, stack_or_thickness, pixelSize, developTime, measurements, parameters, doses=(1.0,), focalPlanes=1,
                        steps=None, maxIterations=1024):
    """The residuals of calibrateResist's loss at `resist` and their Jacobian: (r float64 [2 M], J float64 [2 M, P]) on the host for
    the M measurements (two edge points each, in the order given) and the P names of `parameters`, J = dr / d(parameter).  r_i =
    min(T~_i, 2 developTime) / developTime - 1 with T~ the bilinear sample of T at the edge point; the stencils and the mask that
    takes a clamped sample and an unreached cell out of the derivative are those of the loss, so loss = mean(r^2) and
    (2 / len(r)) J^T r is resistParameterGradient of the loss's dl/dT.  One forward run and P tangents in one sweep."""
    who = "calibrationJacobian"
    names = list(parameters)
    if not names or len(set(names)) != len(names):
        raise ValueError(f"{who}: parameters must name at least one parameter, each once; got {names}")
    if not measurements:
        raise ValueError(f"{who}: give at least one measurement")
    t = _positive(who, "developTime", developTime)
    f = _forward(who, image, resist, stack_or_thickness, pixelSize, doses, focalPlanes, maxIterations, steps)
    points = _edge_points(who, measurements, len(f.doses), f.F, f.D, f.n, f.pixel, nat.require_gpu(image.device))
    return _jacobian(who, f, t, points, names)
