"""Post-exposure bake of a chemically amplified resist: acid-quencher reaction-diffusion; no reference counterpart
(include/litho_abbe.h; csrc/peb.hip).

Exposure releases acid, h0 = 1 - exp(-C dose I) relative to the initial photo-acid generator.  During the bake the acid diffuses,
is neutralised by the base quencher (which may diffuse too, usually far less), is lost, and catalyses the deprotection that lets
the developer in: with a = the time integral of the acid, the inhibitor left is m = exp(-kAmp a), and Mack's rate of m gives the
slowness volume that `developmentTime` takes -- everything downstream of `developmentRate` is unchanged.  The bake is an explicit
scheme of `steps` steps on the grid of develop.py (plane d at depth (d + 1/2) thickness / D, lateral pitch `pixelSize`) with no
flux through any of the six faces: unlike `latentDiffusion`, which puts zeros outside the grid laterally, the bake mirrors, so
acid minus quencher is conserved exactly and a bake does not drain acid out of the picture.

Gradients: `bakeGradient`, `exposeAcidGradient` and their chain `postExposureBakeGradient` are the discrete adjoint of exactly this
scheme, for a loss on the acid, the quencher, the acid dose or the inhibitor after the bake (litho_peb_bake_vjp: a checkpointed
forward sweep, then one backward step per launch); `ilt.bakedResistModel` hands them to `optimizeMask`.  `amplifiedRateGradient` is amplifiedRate backwards, the link from
develop.py's gradients through development (`resistProfileGradient`, `ilt.developedResistModel`) to the bake's.

Gradients with respect to the resist's own parameters (kQuench, kLoss, the diffusion lengths, verticalScale, kAmp, C) and the
calibration loop built on them are in calibrate.py.

NOT built: bleaching, a diffusivity that depends on the deprotection."""
import math

import torch

from . import _native as nat
from .develop import MackResist, _gains, _positive, _surface_depth, _volume

MAX_STEPS = 65536


class ChemicallyAmplifiedResist:
    """A chemically amplified resist, a plain value class (normalised concentrations, nm, s).

    `C` > 0: Dill C, acid h0 = 1 - exp(-C dose I).  `quencher` >= 0: the base loading q0 relative to the initial PAG.  `kAmp` > 0:
    amplification rate, m = exp(-kAmp integral of h dt).  `kQuench` >= 0 (1 / s per unit concentration; float('inf') =
    instantaneous neutralisation), `kLoss` >= 0 (1 / s).  `acidDiffusionLength`, `quencherDiffusionLength` >= 0: the customary
    sigma = sqrt(2 D bakeTime) in nm; the vertical one is `verticalScale` (>= 0) times the lateral.  `bakeTime` > 0 s.  `mack`:
    the MackResist whose rMax, rMin, q, mTh and surface inhibition develop the baked resist; its C is not used and its own
    diffusionLength fields must be 0 (the bake is the diffusion)."""

    def __init__(self, C, quencher, kAmp, kQuench, kLoss, acidDiffusionLength, quencherDiffusionLength, verticalScale=1.0, *, bakeTime,
                 mack):
        self.C, self.quencher, self.kAmp, self.kQuench, self.kLoss = float(C), float(quencher), float(kAmp), float(kQuench), float(kLoss)
        self.acidDiffusionLength, self.quencherDiffusionLength = float(acidDiffusionLength), float(quencherDiffusionLength)
        self.verticalScale, self.bakeTime, self.mack = float(verticalScale), float(bakeTime), mack
        pos = lambda v: v > 0.0 and math.isfinite(v)                              # noqa: E731
        if not (pos(self.C) and pos(self.kAmp) and pos(self.bakeTime)):
            raise ValueError("ChemicallyAmplifiedResist: C, kAmp and bakeTime must be positive and finite")
        for name in ("quencher", "kLoss", "acidDiffusionLength", "quencherDiffusionLength", "verticalScale"):
            v = getattr(self, name)
            if not (v >= 0.0 and math.isfinite(v)):
                raise ValueError(f"ChemicallyAmplifiedResist: {name} must be finite and >= 0; got {v}")
        if not self.kQuench >= 0.0:
            raise ValueError(f"ChemicallyAmplifiedResist: kQuench must be >= 0 (inf: instantaneous); got {kQuench}")
        if not isinstance(mack, MackResist):
            raise TypeError("ChemicallyAmplifiedResist: mack must be a MackResist")
        if mack.diffusionLength != 0.0 or mack.verticalDiffusionLength != 0.0:
            raise ValueError("ChemicallyAmplifiedResist: the MackResist's own diffusion lengths must be 0; the bake is the diffusion")

    def minSteps(self, thickness, D, pixelSize):
        """The smallest number of bake steps at which every diffusion update is a convex combination (litho_peb_min_steps)."""
        S = int(nat.lib().litho_peb_min_steps(self.acidDiffusionLength, self.quencherDiffusionLength, self.verticalScale, float(thickness),
                                              int(D), float(pixelSize)))
        if S == 0:
            raise ValueError(f"ChemicallyAmplifiedResist: the diffusion lengths need more than {MAX_STEPS} bake steps on this grid "
                             f"(thickness {thickness} nm at {D} planes, pixel {pixelSize} nm), or the grid is invalid")
        return S

    def __repr__(self):
        return (f"ChemicallyAmplifiedResist(C={self.C}, quencher={self.quencher}, kAmp={self.kAmp}, kQuench={self.kQuench}, kLoss={self.kLoss}, "
                f"acidDiffusionLength={self.acidDiffusionLength}, quencherDiffusionLength={self.quencherDiffusionLength}, "
                f"verticalScale={self.verticalScale}, bakeTime={self.bakeTime}, mack={self.mack!r})")


class BakeResult:
    """What postExposureBake returns, all fp32 [len(doses) F, D, n, n], dose-major: `acid` and `quencher` after the bake,
    `acidDose` a = the time integral of the acid in s, `inhibitor` m = exp(-kAmp a), `slowness` 1 / r in s / nm (NaN: a wall to
    developmentTime); `steps`: the bake steps that ran."""

    def __init__(self, acid, quencher, acidDose, inhibitor, slowness, steps):
        self.acid, self.quencher, self.acidDose, self.inhibitor, self.slowness, self.steps = acid, quencher, acidDose, inhibitor, slowness, steps


def _bake_scalars(resist):
    """The bake's physical numbers in the order every litho_peb_bake* entry takes them between the pixel size and the step count."""
    return (resist.quencher, resist.kQuench, resist.kLoss, resist.acidDiffusionLength, resist.quencherDiffusionLength, resist.verticalScale,
            resist.bakeTime)


def _steps(who, resist, thickness, D, pixel, steps):
    least = resist.minSteps(thickness, D, pixel)
    S = max(least, 8) if steps is None else int(steps)
    if not least <= S <= MAX_STEPS:
        raise ValueError(f"{who}: steps must be {least} (the smallest stable number on this grid) ... {MAX_STEPS}; got {steps}")
    return S


def exposeAcid(image, C, doses=(1.0,)):
    """The acid released by exposure (litho_peb_expose): h0 = 1 - exp(-C dose I) for the intensity volume `image`, fp32 [D,n,n] or
    [F,D,n,n] on the GPU; returns [len(doses) F, D, n, n], dose-major, at most 64 doses; NaN where dose x intensity is negative
    or NaN."""
    who = "exposeAcid"
    v, F, D, n, _, dev = _volume(who, image)
    g, count = _gains(who, doses, F, D)
    out = torch.empty((count * F, D, n, n), dtype=torch.float32, device=dev)
    nat.call(dev, "litho_peb_expose", nat.ptr(v), F, D, n, g, count, _positive(who, "C", C), nat.ptr(out), keep=(v,))
    return out


def bakeAcid(acid, resist, thickness, pixelSize, steps=None, stepsPerLaunch=0):
    """The bake alone (litho_peb_bake) from the acid volume `acid`, fp32 [D,n,n] or [B,D,n,n] on the GPU, with the quencher uniform
    at resist.quencher: returns (acid, quencher, acidDose, steps), the volumes shaped like the input.  `steps` and
    `stepsPerLaunch` as in postExposureBake."""
    who = "bakeAcid"
    if not isinstance(resist, ChemicallyAmplifiedResist):
        raise TypeError(f"{who}: resist must be a ChemicallyAmplifiedResist")
    v, B, D, n, batched, dev = _volume(who, acid, "acid")
    thickness, h = _positive(who, "thickness", thickness), _positive(who, "pixelSize", pixelSize)
    S = _steps(who, resist, thickness, D, h, steps)
    spl = int(stepsPerLaunch)
    if not 0 <= spl <= 4:
        raise ValueError(f"{who}: stepsPerLaunch must be 0 (automatic) ... 4; got {stepsPerLaunch}")
    out_h, out_q, out_a = (torch.empty_like(v) for _ in range(3))
    nbytes = int(nat.lib().litho_peb_work_bytes(B, D, n))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nat.call(dev, "litho_peb_bake", nat.ptr(v), B, D, n, thickness, h, *_bake_scalars(resist), S, spl, nat.ptr(out_h), nat.ptr(out_q),
             nat.ptr(out_a), nat.ptr(work), nbytes, keep=(v, work))
    if not batched:
        out_h, out_q, out_a = out_h[0], out_q[0], out_a[0]
    return out_h, out_q, out_a, S


def amplifiedRate(acidDose, resist, thickness):
    """(inhibitor, slowness) of the baked resist (litho_peb_rate) from the acid dose a, fp32 [D,n,n] or [B,D,n,n] on the GPU:
    m = exp(-kAmp a) and 1 / (Mack's rate of m x the surface factor) with resist.mack's parameters.  A NaN or negative a gives a
    NaN slowness, a wall to developmentTime."""
    who = "amplifiedRate"
    if not isinstance(resist, ChemicallyAmplifiedResist):
        raise TypeError(f"{who}: resist must be a ChemicallyAmplifiedResist")
    v, B, D, n, batched, dev = _volume(who, acidDose, "acidDose")
    thickness, mack = _positive(who, "thickness", thickness), resist.mack
    slow, m = torch.empty_like(v), torch.empty_like(v)
    nat.call(dev, "litho_peb_rate", nat.ptr(v), B, D, n, resist.kAmp, mack.rMax, mack.rMin, mack.q, mack.mTh, mack.surfaceRate,
             _surface_depth(mack, thickness), thickness, nat.ptr(slow), nat.ptr(m), keep=(v,))
    return (m, slow) if batched else (m[0], slow[0])


def amplifiedRateGradient(acidDose, resist, thickness, gradSlowness):
    """amplifiedRate backwards (litho_develop_rate_vjp with kappa = kAmp and a single gain of 1): gradAcidDose = dl/d acidDose from
    gradSlowness = dl/d slowness, both shaped like `acidDose` ([D,n,n] or [B,D,n,n]).  A cell whose slowness is NaN contributes 0.
    What postExposureBakeGradient(gradAcidDose=) takes."""
    who = "amplifiedRateGradient"
    if not isinstance(resist, ChemicallyAmplifiedResist):
        raise TypeError(f"{who}: resist must be a ChemicallyAmplifiedResist")
    from .develop import _rate_vjp
    if isinstance(acidDose, torch.Tensor) and acidDose.dim() == 3 and isinstance(gradSlowness, torch.Tensor) and gradSlowness.dim() == 3:
        gradSlowness = gradSlowness[None]                                         # one volume: the single gain's cotangent
    return _rate_vjp(who, acidDose, [1.0], resist.kAmp, resist.mack, _positive(who, "thickness", thickness), gradSlowness)


def postExposureBake(image, resist, thickness, pixelSize, doses=(1.0,), steps=None, stepsPerLaunch=0):
    """Exposure, bake and rate of `resist` (a ChemicallyAmplifiedResist) on the intensity volume `image`, fp32 [D,n,n] or [F,D,n,n]
    on the GPU, in a layer of `thickness` nm: exposeAcid, bakeAcid, amplifiedRate.  Returns a BakeResult, [len(doses) F, D, n, n];
    at most 64 doses.  Where dose x intensity is negative or NaN the acid starts as NaN, which the bake spreads one cell per
    step.

    `steps`: None takes max(resist.minSteps(...), 8); a value below minSteps raises (the explicit diffusion would lose its
    maximum principle), the cap is 65536.  The reaction terms are first order in the step length: RAISE `steps` for a stiff
    finite kQuench (kQuench x bakeTime / steps well above 1) until the result stops moving.  `stepsPerLaunch`: 0 lets the
    library choose between its direct kernel (1) and its fused kernel (2 ... 4 steps per launch); the result does not depend
    on it, bit for bit."""
    if not isinstance(resist, ChemicallyAmplifiedResist):
        raise TypeError("postExposureBake: resist must be a ChemicallyAmplifiedResist")
    h0 = exposeAcid(image, resist.C, doses)
    acid, quencher, dose, S = bakeAcid(h0, resist, thickness, pixelSize, steps, stepsPerLaunch)
    m, slow = amplifiedRate(dose, resist, thickness)
    return BakeResult(acid, quencher, dose, m, slow, S)


# ---- gradients through the bake ----------------------------------------------------------------------------------------------------
def _cotangent(who, name, g, like, batched):
    """A cotangent shaped like the volume it belongs to, as contiguous fp32 [B,D,n,n] on its device; None stays None."""
    if g is None:
        return None
    want = tuple(like.shape) if batched else tuple(like.shape[1:])
    if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or tuple(g.shape) != want or g.device != like.device:
        raise ValueError(f"{who}: {name} must be a float32 tensor {want} on {like.device}; got {getattr(g, 'dtype', type(g))} "
                         f"{tuple(getattr(g, 'shape', ()))} on {getattr(g, 'device', None)}")
    g = g.detach().contiguous()
    return g if batched else g[None]


def bakeGradient(acid, resist, thickness, pixelSize, gradAcid=None, gradQuencher=None, gradAcidDose=None, steps=None, checkpointEvery=None):
    """The bake backwards (litho_peb_bake_vjp): for a real loss l on bakeAcid's outputs with gradAcid = dl/d acid, gradQuencher =
    dl/d quencher, gradAcidDose = dl/d acidDose (each shaped like `acid`, None = zero, at least one given), returns
    (gradAcid0, gradQuencher0) = (dl/d h0, qbar_0), shaped like `acid` ([D,n,n] or [B,D,n,n]).  The initial quencher is one number
    per volume, so dl/d resist.quencher of a volume is gradQuencher0.sum() over it.  `steps` as in bakeAcid -- the same default,
    so that forward and backward describe one function.  The discrete adjoint of the explicit scheme, step by step (the header's
    "Gradients through the bake"); the call runs its own forward sweep and keeps the state every `checkpointEvery` steps (1 ...
    steps; None: ceil(sqrt(steps))), re-running each segment once: the result does not depend on it, bit for bit, only the
    workspace does, (2 (ceil(steps / c) - 1) + 2 c + 8) volumes.  With instantaneous neutralisation the loss is differentiable
    only where acid and quencher do not tie; a tie takes the forward's branch."""
    return _bake_vjp("bakeGradient", False, acid, resist, thickness, pixelSize, gradAcid, gradQuencher, gradAcidDose, steps, checkpointEvery)


def _bake_vjp(who, withStep, acid, resist, thickness, pixelSize, gradAcid, gradQuencher, gradAcidDose, steps, checkpointEvery):
    """bakeGradient (litho_peb_bake_vjp) and, withStep, calibrate.bakeStepGradient (litho_peb_bake_vjp_params: one more output,
    float64 [B, 6], and its own workspace size) behind one set of checks."""
    if not isinstance(resist, ChemicallyAmplifiedResist):
        raise TypeError(f"{who}: resist must be a ChemicallyAmplifiedResist")
    v, B, D, n, batched, dev = _volume(who, acid, "acid")
    thickness, h = _positive(who, "thickness", thickness), _positive(who, "pixelSize", pixelSize)
    S = _steps(who, resist, thickness, D, h, steps)
    c = math.isqrt(S - 1) + 1 if checkpointEvery is None else int(checkpointEvery)    # ceil(sqrt(S))
    if not 1 <= c <= S:
        raise ValueError(f"{who}: checkpointEvery must be 1 ... steps ({S}); got {checkpointEvery}")
    gh, gq, ga = (_cotangent(who, name, g, v, batched) for name, g in (("gradAcid", gradAcid), ("gradQuencher", gradQuencher),
                                                                        ("gradAcidDose", gradAcidDose)))
    if gh is None and gq is None and ga is None:
        raise ValueError(f"{who}: give at least one of gradAcid, gradQuencher, gradAcidDose")
    entry, sizer = ("litho_peb_bake_vjp_params", "litho_peb_vjp_params_work_bytes") if withStep else ("litho_peb_bake_vjp", "litho_peb_vjp_work_bytes")
    outs = [torch.empty_like(v), torch.empty_like(v)] + ([torch.empty((B, 6), dtype=torch.float64, device=dev)] if withStep else [])
    nbytes = int(getattr(nat.lib(), sizer)(B, D, n, S, c))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    opt = lambda t: nat.ptr(t) if t is not None else None                       # noqa: E731
    nat.call(dev, entry, nat.ptr(v), B, D, n, thickness, h, *_bake_scalars(resist), S, c, opt(gh), opt(gq), opt(ga), *(nat.ptr(t) for t in outs),
             nat.ptr(work), nbytes, keep=(v, gh, gq, ga, work))
    return tuple(outs) if batched else tuple(t[0] for t in outs)


def exposeAcidGradient(image, C, doses, gradAcid):
    """exposeAcid backwards (litho_peb_expose_vjp): gradImage = sum over the doses of (C dose) exp(-C dose I) gradAcid[dose],
    shaped like `image` ([D,n,n] or [F,D,n,n]); gradAcid fp32 [len(doses) F, D, n, n], dose-major, as exposeAcid returns."""
    who = "exposeAcidGradient"
    v, F, D, n, batched, dev = _volume(who, image)
    g, count = _gains(who, doses, F, D)
    want = (count * F, D, n, n)
    if not isinstance(gradAcid, torch.Tensor) or gradAcid.dtype != torch.float32 or tuple(gradAcid.shape) != want or gradAcid.device != dev:
        raise ValueError(f"{who}: gradAcid must be a float32 tensor {want} on {dev}; got {getattr(gradAcid, 'dtype', type(gradAcid))} "
                         f"{tuple(getattr(gradAcid, 'shape', ()))} on {getattr(gradAcid, 'device', None)}")
    ga = gradAcid.detach().contiguous()
    out = torch.empty_like(v)
    nat.call(dev, "litho_peb_expose_vjp", nat.ptr(v), F, D, n, g, count, _positive(who, "C", C), nat.ptr(ga), nat.ptr(out), keep=(v, ga))
    return out if batched else out[0]


def postExposureBakeGradient(image, resist, thickness, pixelSize, doses=(1.0,), gradInhibitor=None, gradAcidDose=None, gradAcid=None,
                             gradQuencher=None, steps=None, checkpointEvery=None):
    """postExposureBake backwards, down to the intensity: gradImage shaped like `image` for a real loss on the BakeResult's
    `inhibitor`, `acidDose`, `acid` and `quencher` (cotangents [len(doses) F, D, n, n], dose-major; None = zero, at least one
    given).  The chain of three pieces: the inhibitor m = exp(-kAmp a) gives abar = gradAcidDose - kAmp m gradInhibitor (pointwise,
    torch on the device, m from the forward bake that this call runs), then bakeGradient, then exposeAcidGradient.  `steps`:
    the default of postExposureBake.  The slowness is not differentiated here: develop.resistProfileGradient carries a cotangent on
    the arrival times through development and the rate and enters this call through gradAcidDose."""
    who = "postExposureBakeGradient"
    if not isinstance(resist, ChemicallyAmplifiedResist):
        raise TypeError(f"{who}: resist must be a ChemicallyAmplifiedResist")
    if gradInhibitor is None and gradAcidDose is None and gradAcid is None and gradQuencher is None:
        raise ValueError(f"{who}: give at least one of gradInhibitor, gradAcidDose, gradAcid, gradQuencher")
    h0 = exposeAcid(image, resist.C, doses)
    ga = gradAcidDose
    if gradInhibitor is not None:
        _, _, a, _ = bakeAcid(h0, resist, thickness, pixelSize, steps)
        if (not isinstance(gradInhibitor, torch.Tensor) or gradInhibitor.dtype != torch.float32 or gradInhibitor.shape != a.shape
                or gradInhibitor.device != a.device):
            raise ValueError(f"{who}: gradInhibitor must be a float32 tensor {tuple(a.shape)} on {a.device}; got "
                             f"{getattr(gradInhibitor, 'dtype', type(gradInhibitor))} {tuple(getattr(gradInhibitor, 'shape', ()))}")
        from_m = (-resist.kAmp) * torch.exp(-resist.kAmp * a) * gradInhibitor.detach()
        ga = from_m if ga is None else ga + from_m
    gh0, _ = bakeGradient(h0, resist, thickness, pixelSize, gradAcid, gradQuencher, ga, steps, checkpointEvery)
    return exposeAcidGradient(image, resist.C, doses, gh0)
