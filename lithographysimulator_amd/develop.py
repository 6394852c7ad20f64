"""Resist development: Mack's dissolution rate and the propagation of the development front; no reference counterpart
(include/litho_abbe.h; csrc/develop.hip).

`vectorSocsKernels(film=, depths=)` gives the intensity at D depths inside the resist.  This module turns such a [D, n, n] stack
into a resist PROFILE: the latent image is diffused (lateral and vertical acid diffusion, the vertical one with no flux through
the layer faces -- what removes the standing-wave scallops a post-exposure bake removes), exposure and Mack's model give a
dissolution rate per cell, and the arrival time T of the development front is the first-order upwind solution of |grad T| = 1 / r
with T = 0 on the resist top.  The planes of T are [planes, n, n] fp32 like any image: `measureCD`, `measureEPE`, `traceContours`,
`processVariationBand` and the GDSII writer take them unchanged, with the threshold = the development time and exposed=False
(developed = T below the threshold).

Grid: plane d of D sits at depth (d + 1/2) thickness / D, `FilmStack.depths(D)`; the lateral pitch is the image's pixel size.
A batch is [B, D, n, n] with B = doses x focal planes, dose-major.

A chemically amplified resist (peb.py: ChemicallyAmplifiedResist) takes the place of the Gaussian blur and of developmentRate with a
reaction-diffusion post-exposure bake with quencher, `postExposureBake`; resistProfile accepts either kind of resist.

Gradients: `developmentTimeGradient` differentiates the solver itself -- the adjoint of the Godunov fixed point, an iteration
of the same tiled kind as the forward (litho_develop_time_vjp) -- `developmentRateGradient` the rate law and the latent-image
diffusion, and `resistProfileGradient` chains them from a cotangent on the arrival times T down to the intensity stack, for
either kind of resist; `ilt.developedResistModel` hands that to `optimizeMask`.  On the symmetry line of a symmetric pattern,
where the two neighbours of an axis tie, the gradient is a valid but one-sided subgradient (the tie goes to the lower index).

NOT built: bleaching (Dill A, B: the intensity is taken as given), development of anything but one layer, the gradient of
`developedDepth`, the gradients of a MackResist's own Gaussian diffusion lengths (the other resist parameters: calibrate.py), a
fused or coarser-grained backward solver."""
import ctypes
import math

import numpy as np
import torch

from . import _native as nat
from .film import FilmStack

MAX_PLANES = 32


class MackResist:
    """Dill C exposure and Mack's dissolution model, a plain value class.

    m = exp(-C dose I) is the inhibitor left after exposure; r = rMax (a + 1)(1 - m)^q / (a + (1 - m)^q) + rMin in nm / s with
    a = (q + 1) / (q - 1) (1 - mTh)^q.  C > 0 (per unit of dose x intensity), rMax > 0, rMin > 0, q > 1, 0 <= mTh < 1.
    `surfaceRate` r0 in (0, 1] and `surfaceDepth` delta > 0 (nm; None: the factor is switched off) give the surface inhibition
    factor 1 - (1 - r0) exp(-z / delta).  `diffusionLength` / `verticalDiffusionLength` (nm, >= 0) are the lateral and vertical
    standard deviations of the latent-image diffusion."""

    def __init__(self, C, rMax, rMin, q, mTh, surfaceRate=1.0, surfaceDepth=None, diffusionLength=0.0, verticalDiffusionLength=0.0):
        self.C, self.rMax, self.rMin, self.q, self.mTh = float(C), float(rMax), float(rMin), float(q), float(mTh)
        self.surfaceRate = float(surfaceRate)
        self.surfaceDepth = None if surfaceDepth is None else float(surfaceDepth)
        self.diffusionLength, self.verticalDiffusionLength = float(diffusionLength), float(verticalDiffusionLength)
        pos = lambda v: v > 0.0 and math.isfinite(v)                              # noqa: E731
        if not (pos(self.C) and pos(self.rMax) and pos(self.rMin)):
            raise ValueError("MackResist: C, rMax and rMin must be positive and finite")
        if not (self.q > 1.0 and math.isfinite(self.q)):
            raise ValueError(f"MackResist: q > 1 is required; got {q}")
        if not 0.0 <= self.mTh < 1.0:
            raise ValueError(f"MackResist: 0 <= mTh < 1 is required; got {mTh}")
        if not 0.0 < self.surfaceRate <= 1.0:
            raise ValueError(f"MackResist: 0 < surfaceRate <= 1 is required; got {surfaceRate}")
        if self.surfaceDepth is not None and not pos(self.surfaceDepth):
            raise ValueError(f"MackResist: surfaceDepth must be positive and finite (nm), or None; got {surfaceDepth}")
        if self.surfaceDepth is None and self.surfaceRate != 1.0:
            raise ValueError("MackResist: a surfaceRate below 1 needs a surfaceDepth (nm)")
        for name in ("diffusionLength", "verticalDiffusionLength"):
            v = getattr(self, name)
            if not (v >= 0.0 and math.isfinite(v)):
                raise ValueError(f"MackResist: {name} must be finite and >= 0 nm; got {v}")

    def rate(self, m):
        """Mack's rate at inhibitor concentration m (host, float64): rMin at m = 1, rMax + rMin at m = 0."""
        a = (self.q + 1.0) / (self.q - 1.0) * (1.0 - self.mTh) ** self.q
        x = (1.0 - np.asarray(m, dtype=np.float64)) ** self.q
        return (self.rMax * (a + 1.0)) * x / (a + x) + self.rMin

    def __repr__(self):
        return (f"MackResist(C={self.C}, rMax={self.rMax}, rMin={self.rMin}, q={self.q}, mTh={self.mTh}, surfaceRate={self.surfaceRate}, "
                f"surfaceDepth={self.surfaceDepth}, diffusionLength={self.diffusionLength}, "
                f"verticalDiffusionLength={self.verticalDiffusionLength})")


def _volume(who, t, what="image"):
    """A float32 GPU tensor [D,n,n] or [B,D,n,n] as contiguous [B,D,n,n]; returns (tensor, B, D, n, batched, device)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() not in (3, 4) or t.shape[-1] != t.shape[-2]:
        raise ValueError(f"{who}: {what} must be a float32 tensor [D,n,n] or [B,D,n,n]; got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    dev = nat.require_gpu(t.device)
    batched = t.dim() == 4
    v = t.detach().contiguous()
    if not batched:
        v = v[None]
    B, D, n = int(v.shape[0]), int(v.shape[1]), int(v.shape[-1])
    if not (1 <= D <= MAX_PLANES and 1 <= n <= 16384 and B >= 1 and B * D <= 65535):
        raise ValueError(f"{who}: 1 <= D <= {MAX_PLANES} planes, 1 <= n <= 16384 and B D <= 65535 are required; got B {B}, D {D}, n {n}")
    return v, B, D, n, batched, dev


def _positive(who, name, v):
    v = float(v)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"{who}: {name} must be positive and finite; got {v}")
    return v


def _gains(who, doses, F, D):
    """The doses of a call on F volumes of D planes as the C ABI takes them: (float array, count)."""
    gains = [float(d) for d in doses]
    if not 1 <= len(gains) <= 64:
        raise ValueError(f"{who}: between 1 and 64 doses per call; got {len(gains)}")
    if len(gains) * F * D > 65535:
        raise ValueError(f"{who}: doses x volumes x planes exceeds 65535")
    return (ctypes.c_float * len(gains))(*gains), len(gains)


def _surface_depth(mack, thickness):
    """The depth of the surface-inhibition factor as the C ABI takes it: the layer's thickness where the factor is switched off."""
    return mack.surfaceDepth if mack.surfaceDepth is not None else thickness


def latentDiffusion(image, thickness, pixelSize, diffusionLength=0.0, verticalDiffusionLength=0.0):
    """The intensity volume [D,n,n] or [B,D,n,n] convolved with a separable Gaussian (litho_latent_diffuse): standard deviation
    `diffusionLength` nm along x and y with zeros outside the grid -- the taps of resistContour(diffusionLength=) -- and
    `verticalDiffusionLength` nm along z with the layer faces mirrored.  4 sigma may span at most 32 cells on an axis; a length
    of 0 leaves that axis untouched bit for bit."""
    who = "latentDiffusion"
    v, B, D, n, batched, dev = _volume(who, image)
    thickness, h = _positive(who, "thickness", thickness), _positive(who, "pixelSize", pixelSize)
    sxy, sz = float(diffusionLength) / h, float(verticalDiffusionLength) / (thickness / D)
    for name, s in (("diffusionLength", sxy), ("verticalDiffusionLength", sz)):
        if not (0.0 <= s <= 8.0):
            raise ValueError(f"{who}: {name} must be >= 0 and span at most 8 cells (4 sigma <= 32 cells); got {s:g} cells")
    out = torch.empty_like(v)
    passes = (2 if sxy > 0 else 0) + (1 if sz > 0 else 0)
    work = torch.empty_like(v) if passes >= 2 else None
    nat.call(dev, "litho_latent_diffuse", nat.ptr(v), B, D, n, sxy, sz, nat.ptr(out), nat.ptr(work) if work is not None else None,
             work.numel() * 4 if work is not None else 0, keep=(work,))
    return out if batched else out[0]


def developmentRate(image, resist, thickness, pixelSize, doses=(1.0,)):
    """The slowness 1 / r in s / nm of `resist` (a MackResist) exposed by the intensity volume `image`, fp32 [D,n,n] or [F,D,n,n]
    on the GPU, through a layer of `thickness` nm: the latent-image diffusion of `resist` first (latentDiffusion), then
    litho_develop_rate.  Returns [len(doses) F, D, n, n], dose-major; at most 64 doses.  Where dose x intensity is negative or
    NaN the slowness is NaN (written explicitly by the kernel, whatever q), a wall to developmentTime."""
    who = "developmentRate"
    if not isinstance(resist, MackResist):
        raise TypeError(f"{who}: resist must be a MackResist")
    v, F, D, n, _, dev = _volume(who, image)
    thickness, h = _positive(who, "thickness", thickness), _positive(who, "pixelSize", pixelSize)
    g, count = _gains(who, doses, F, D)
    if resist.diffusionLength > 0.0 or resist.verticalDiffusionLength > 0.0:
        v = latentDiffusion(v, thickness, h, resist.diffusionLength, resist.verticalDiffusionLength)
    out = torch.empty((count * F, D, n, n), dtype=torch.float32, device=dev)
    nat.call(dev, "litho_develop_rate", nat.ptr(v), F, D, n, g, count, resist.C, resist.rMax, resist.rMin, resist.q, resist.mTh,
             resist.surfaceRate, _surface_depth(resist, thickness), thickness, nat.ptr(out), keep=(v,))
    return out


def _development_time(slowness, thickness, pixelSize, maxIterations):
    who = "developmentTime"
    s, B, D, n, batched, dev = _volume(who, slowness, "slowness")
    thickness, h = _positive(who, "thickness", thickness), _positive(who, "pixelSize", pixelSize)
    maxIterations = int(maxIterations)
    if not 1 <= maxIterations <= 65536:
        raise ValueError(f"{who}: maxIterations must be 1 ... 65536; got {maxIterations}")
    T = torch.empty_like(s)
    nbytes = int(nat.lib().litho_develop_work_bytes(B, D, n, maxIterations))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    launches = ctypes.c_int(0)
    nat.call(dev, "litho_develop_time", nat.ptr(s), B, D, n, thickness, h, maxIterations, nat.ptr(T), nat.ptr(work), nbytes, ctypes.byref(launches))
    return (T if batched else T[0]), launches.value


def developmentTime(slowness, thickness, pixelSize, maxIterations=1024, returnLaunches=False):
    """The arrival time T in seconds of the development front (litho_develop_time): the first-order upwind solution of
    |grad T| = slowness with T = 0 on the resist top, half a plane spacing above plane 0.  `slowness` fp32 [D,n,n] or [B,D,n,n] in
    s / nm on the GPU; a cell whose slowness is not finite and positive is a wall and keeps T = +inf, as does every cell the front
    cannot reach.  The solver iterates to its fixed point and waits for the device while it does; if `maxIterations` launches do
    not reach it, RuntimeError is raised -- an unconverged field is never returned.  Deterministic: the same bits on every call,
    and a batch equals its volumes solved one at a time.  returnLaunches=True returns (T, launches)."""
    T, launches = _development_time(slowness, thickness, pixelSize, maxIterations)
    return (T, launches) if returnLaunches else T


def developedDepth(T, thickness, developTime):
    """How deep each column is developed after `developTime` seconds (litho_developed_depth): fp32 [n,n] or [B,n,n] in nm below the
    resist top, the first crossing of T = developTime going down, linear between planes; `thickness` where the column has cleared
    to the bottom of the layer.  The remaining resist height is thickness - depth."""
    who = "developedDepth"
    v, B, D, n, batched, dev = _volume(who, T, "T")
    thickness = _positive(who, "thickness", thickness)
    t = float(developTime)
    if not (t >= 0.0 and math.isfinite(t)):
        raise ValueError(f"{who}: developTime must be finite and >= 0; got {developTime}")
    out = torch.empty((B, n, n), dtype=torch.float32, device=dev)
    nat.call(dev, "litho_developed_depth", nat.ptr(v), B, D, n, thickness, t, nat.ptr(out), keep=(v,))
    return out if batched else out[0]


class ResistProfile:
    """What resistProfile returns.  `T` fp32 [doses, F, D, n, n]: arrival times in seconds (+inf where the developer never
    arrives); `depth` fp32 [doses, F, n, n]: developed depth in nm; `launches`: solver launches; `thickness`, `pixelSize`,
    `developTime`, `doses` as given.

    For the metrology helpers +inf in T is replaced by the finite value 2 developTime + 1 (`clampedT`), because measureCD and
    traceContours interpolate linearly between samples: an edge next to a cell the developer never reaches then lies where a
    cell of that arrival time would put it, not at a NaN."""

    def __init__(self, T, depth, launches, thickness, pixelSize, developTime, doses):
        self.T, self.depth, self.launches = T, depth, launches
        self.thickness, self.pixelSize, self.developTime, self.doses = thickness, pixelSize, developTime, tuple(doses)

    @property
    def clampedT(self):
        return torch.where(torch.isposinf(self.T), torch.full_like(self.T, 2.0 * self.developTime + 1.0), self.T)

    def cd(self, gauges, exposed=False):
        """measureCD on every plane of T with threshold developTime: fp32 [doses, F D, G, 5] = (cd_nm, x_lo, x_hi, ils_lo,
        ils_hi).  exposed=False (the default) measures the developed run through the gauge -- a space or a contact."""
        from .imageformation import measureCD
        nd, F, D, n = self.T.shape[0], self.T.shape[1], self.T.shape[2], self.T.shape[-1]
        out = measureCD(self.clampedT.reshape(nd * F * D, n, n), self.developTime, gauges, self.pixelSize, exposed=exposed)
        return out.reshape(nd, F * D, out.shape[2], 5)

    def sidewallAngle(self, gauge, exposed=False):
        """Side-wall angles in degrees at one gauge (row, col, axis), float64 [doses, F, 2]: a least-squares line through the edge
        positions x_lo(z_d) and x_hi(z_d) of `cd` over the depths where the feature exists, on the host.  The angle is measured
        inside the resist from the substrate plane: 90 is a vertical wall, below 90 a developed space that narrows with depth;
        NaN with fewer than two usable depths."""
        nd, F, D = self.T.shape[0], self.T.shape[1], self.T.shape[2]
        table = self.cd([tuple(int(v) for v in gauge)], exposed=exposed).cpu().numpy().astype(np.float64).reshape(nd, F, D, 5)
        z = self.thickness * (np.arange(D) + 0.5) / D
        out = np.full((nd, F, 2), np.nan)
        for i in range(nd):
            for f in range(F):
                for e, sign in ((0, -1.0), (1, 1.0)):
                    x = table[i, f, :, 1 + e] * self.pixelSize
                    ok = np.isfinite(x) & (table[i, f, :, 0] > 0)
                    if ok.sum() >= 2:
                        slope = np.polyfit(z[ok], x[ok], 1)[0]                       # d(edge) / dz, nm per nm
                        out[i, f, e] = 90.0 + sign * math.degrees(math.atan(slope))
        return out

    def contours(self, depth_index, exposed=False):
        """traceContours of T at plane `depth_index` with threshold developTime: result[dose][focal plane] is a Contours."""
        from .contours import traceContours
        nd, F, n = self.T.shape[0], self.T.shape[1], self.T.shape[-1]
        planes = self.clampedT[:, :, int(depth_index)].reshape(nd * F, n, n).contiguous()
        flat = traceContours(planes, self.developTime, exposed=exposed)[0]
        return [flat[i * F:(i + 1) * F] for i in range(nd)]


def resistProfile(image, resist, stack_or_thickness, pixelSize, developTime, doses=(1.0,), focalPlanes=1, maxIterations=1024):
    """The chain developmentRate -> developmentTime -> developedDepth on an intensity stack; with a ChemicallyAmplifiedResist
    (peb.py) the slowness comes from postExposureBake (its default steps) instead of developmentRate.  `image` fp32 [F D, n, n] in the plane
    order hopkinsImage returns for vectorSocsKernels(film=, depths=stack.depths(D)) (plane f D + d), F = `focalPlanes`;
    `stack_or_thickness` the FilmStack (its resist layer is developed) or the thickness in nm.  Returns a ResistProfile; before
    its T goes to measureCD or traceContours, +inf is clamped to 2 developTime + 1 (ResistProfile)."""
    who = "resistProfile"
    thickness = stack_or_thickness.thickness if isinstance(stack_or_thickness, FilmStack) else float(stack_or_thickness)
    F = int(focalPlanes)
    if not isinstance(image, torch.Tensor) or image.dim() != 3 or F < 1 or image.shape[0] % F:
        raise ValueError(f"{who}: image must be [focalPlanes x D, n, n]; got {tuple(getattr(image, 'shape', ()))} with focalPlanes {focalPlanes}")
    t = float(developTime)
    if not (t > 0.0 and math.isfinite(t)):
        raise ValueError(f"{who}: developTime must be positive and finite; got {developTime}")
    D, n = image.shape[0] // F, image.shape[-1]
    from .peb import ChemicallyAmplifiedResist, postExposureBake
    if isinstance(resist, ChemicallyAmplifiedResist):
        s = postExposureBake(image.reshape(F, D, n, n), resist, thickness, pixelSize, doses).slowness
    else:
        s = developmentRate(image.reshape(F, D, n, n), resist, thickness, pixelSize, doses)
    T, launches = _development_time(s, thickness, pixelSize, maxIterations)
    depth = developedDepth(T, thickness, t)
    nd = len(tuple(doses))
    return ResistProfile(T.reshape(nd, F, D, n, n), depth.reshape(nd, F, n, n), launches, thickness, float(pixelSize), t, doses)


# ---- gradients through development -----------------------------------------------------------------------------------------------
def _like(who, name, g, shape, dev):
    """A float32 tensor of exactly `shape` on `dev`, detached and contiguous."""
    if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or tuple(g.shape) != tuple(shape) or g.device != dev:
        raise ValueError(f"{who}: {name} must be a float32 tensor {tuple(shape)} on {dev}; got {getattr(g, 'dtype', type(g))} "
                         f"{tuple(getattr(g, 'shape', ()))} on {getattr(g, 'device', None)}")
    return g.detach().contiguous()


def developmentTimeGradient(slowness, T, gradT, thickness, pixelSize, maxIterations=1024, returnLaunches=False):
    """developmentTime backwards (litho_develop_time_vjp): for a real loss l on the arrival times with gradT = dl/dT, returns
    gradSlowness = dl/d slowness, shaped like `slowness` ([D,n,n] or [B,D,n,n], fp32 on the GPU).  `T` must be what
    developmentTime returned for this slowness, thickness and pixelSize.  The adjoint of the Godunov fixed point: every reached
    cell hands its lambda on to the upwind cells of its update with the weights alpha = w (T - a) / P, and dl/ds = lambda s / P
    (the header's "Gradients through development").  A wall or a cell the front never reached gets 0 and its gradT is ignored,
    NaN and inf included.  Where the two neighbours of an axis tie -- the symmetry line of a symmetric pattern -- the lower-index
    one is taken: a valid but one-sided subgradient.  The solver iterates to a bitwise fixed point and waits for the device while
    it does; if `maxIterations` launches do not reach it, RuntimeError is raised -- an unconverged gradient is never returned.
    Deterministic: the same bits on every call, and a batch equals its volumes solved one at a time.  returnLaunches=True returns
    (gradSlowness, launches)."""
    who = "developmentTimeGradient"
    s, B, D, n, batched, dev = _volume(who, slowness, "slowness")
    thickness, h = _positive(who, "thickness", thickness), _positive(who, "pixelSize", pixelSize)
    maxIterations = int(maxIterations)
    if not 1 <= maxIterations <= 65536:
        raise ValueError(f"{who}: maxIterations must be 1 ... 65536; got {maxIterations}")
    Tv = _like(who, "T", T, slowness.shape, dev).reshape(s.shape)
    g = _like(who, "gradT", gradT, slowness.shape, dev).reshape(s.shape)
    out = torch.empty_like(s)
    nbytes = int(nat.lib().litho_develop_vjp_work_bytes(B, D, n, maxIterations))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    launches = ctypes.c_int(0)
    nat.call(dev, "litho_develop_time_vjp", nat.ptr(s), nat.ptr(Tv), nat.ptr(g), B, D, n, thickness, h, maxIterations, nat.ptr(out), nat.ptr(work),
             nbytes, ctypes.byref(launches), keep=(s, Tv, g, work),
             noconv=f"{who}: the adjoint iteration did not reach its fixed point within the launch cap (maxIterations = {maxIterations}); "
                    "the gradient is not a result")
    out = out if batched else out[0]
    return (out, launches.value) if returnLaunches else out


def _rate_vjp(who, x, doses, kappa, mack, thickness, gradSlowness):
    """litho_develop_rate_vjp on the volume x ([D,n,n] or [F,D,n,n]) with Mack's parameters of `mack`; shaped like x."""
    v, F, D, n, batched, dev = _volume(who, x)
    g, count = _gains(who, doses, F, D)
    gs = _like(who, "gradSlowness", gradSlowness, (count * F, D, n, n), dev)
    out = torch.empty_like(v)
    nat.call(dev, "litho_develop_rate_vjp", nat.ptr(v), F, D, n, g, count, kappa, mack.rMax, mack.rMin, mack.q, mack.mTh, mack.surfaceRate,
             _surface_depth(mack, thickness), thickness, nat.ptr(gs), nat.ptr(out), keep=(v, gs))
    return out if batched else out[0]


def developmentRateGradient(image, resist, thickness, pixelSize, doses, gradSlowness):
    """developmentRate backwards: gradImage = dl/d image, shaped like `image` ([D,n,n] or [F,D,n,n]), from gradSlowness =
    dl/d slowness, fp32 [len(doses) F, D, n, n], dose-major, as developmentRate returns it.  The rate law backwards
    (litho_develop_rate_vjp, evaluated on the diffused image when `resist` diffuses) and then latentDiffusion on the result: the
    diffusion is its own adjoint (symmetric taps with zeros outside the grid laterally, and the half-sample mirror in z has a
    symmetric matrix).  A cell whose slowness is NaN (a wall) contributes 0."""
    who = "developmentRateGradient"
    if not isinstance(resist, MackResist):
        raise TypeError(f"{who}: resist must be a MackResist")
    vv, _, _, _, batched, _ = _volume(who, image)
    v = vv if batched else vv[0]
    thickness, h = _positive(who, "thickness", thickness), _positive(who, "pixelSize", pixelSize)
    diffuses = resist.diffusionLength > 0.0 or resist.verticalDiffusionLength > 0.0
    lat = latentDiffusion(v, thickness, h, resist.diffusionLength, resist.verticalDiffusionLength) if diffuses else v
    out = _rate_vjp(who, lat, doses, resist.C, resist, thickness, gradSlowness)
    return latentDiffusion(out, thickness, h, resist.diffusionLength, resist.verticalDiffusionLength) if diffuses else out


def resistProfileGradient(image, resist, stack_or_thickness, pixelSize, gradT, doses=(1.0,), focalPlanes=1, maxIterations=1024):
    """resistProfile backwards, from the arrival times down to the intensity: gradImage = dl/d image, shaped like `image`
    ([focalPlanes x D, n, n]), for a real loss l on ResistProfile.T with gradT = dl/dT, fp32 [doses, F, D, n, n].  The call runs
    its own forward (the slowness and developmentTime), then developmentTimeGradient, then the rate backwards: with a MackResist
    developmentRateGradient, with a ChemicallyAmplifiedResist amplifiedRateGradient into postExposureBakeGradient(gradAcidDose=)
    (its default steps, as resistProfile).  gradT is ignored where T is +inf; the developed depth is not differentiated."""
    who = "resistProfileGradient"
    thickness = stack_or_thickness.thickness if isinstance(stack_or_thickness, FilmStack) else float(stack_or_thickness)
    F = int(focalPlanes)
    if not isinstance(image, torch.Tensor) or image.dim() != 3 or F < 1 or image.shape[0] % F:
        raise ValueError(f"{who}: image must be [focalPlanes x D, n, n]; got {tuple(getattr(image, 'shape', ()))} with focalPlanes {focalPlanes}")
    D, n = image.shape[0] // F, image.shape[-1]
    doses = tuple(doses)
    vol = image.reshape(F, D, n, n)
    dev = nat.require_gpu(image.device)
    g = _like(who, "gradT", gradT, (len(doses), F, D, n, n), dev).reshape(len(doses) * F, D, n, n)
    from .peb import ChemicallyAmplifiedResist, amplifiedRateGradient, postExposureBake, postExposureBakeGradient
    if isinstance(resist, ChemicallyAmplifiedResist):
        bake = postExposureBake(vol, resist, thickness, pixelSize, doses)
        s = bake.slowness
    else:
        s = developmentRate(vol, resist, thickness, pixelSize, doses)
    T, _ = _development_time(s, thickness, pixelSize, maxIterations)
    gs = developmentTimeGradient(s, T, g, thickness, pixelSize, maxIterations)
    if isinstance(resist, ChemicallyAmplifiedResist):
        ga = amplifiedRateGradient(bake.acidDose, resist, thickness, gs)
        out = postExposureBakeGradient(vol, resist, thickness, pixelSize, doses, gradAcidDose=ga)
    else:
        out = developmentRateGradient(vol, resist, thickness, pixelSize, doses, gs)
    return out.reshape(image.shape)
