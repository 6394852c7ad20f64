"""Source gradients of Abbe imaging, source optimisation and the alternating source-mask loop; no reference counterpart.

The weighted Abbe sum I = sum_s w_s |E_s|^2 (abbeIntensity(weights=)) is linear in the weights.  For a real loss l with
G = dl/dI,

    dl/dw_s = <G, |E_s|^2> = sum_q G[q] |E_s[q]|^2,        E_s = L(roll(P, d_s) . M),

with L the engine's chain at shift (0,0) (ilt.py) and roll(P, d) = torch.roll(P, (dy, dx), (0, 1)), the reference's
imageformation.py:63.  One number per source point, independent of the weights, and no adjoint transform: a source gradient is
one forward field per point and a reduction (measured: LABNOTES.md).  `sourceSensitivities` computes the list on the device (litho_source_sensitivity, csrc/socs_grad.hip: a
source point is a coherent kernel of the SOCS field code, read rolled and reduced against G instead of stored), `sourceGradient`
scatters it onto the source grid, `optimizeSource` descends the weights of a fixed candidate list with optimizeMask's loss, and
`optimizeSourceMask` alternates it with socsKernels and optimizeMask.  Source gradients only: the pupil is a constant here, and the
weights stay real and non-negative."""
import math
from functools import partial

import torch

from . import _descent
from . import _native as nat
from . import socs as _socs

WORK_BYTES = 256 << 20            # default ceiling of sourceSensitivities' workspace (the coverage rasteriser's default as well)


_pow2_size = partial(_descent.pow2_size, entry="litho_source_sensitivity")


def sourceSensitivities(maskFT, pupilF, shifts, N, gradIntensity, pupilsPerPlane=1, batch=None):
    """sens[s] = sum_planes sum_k <gradIntensity[plane], |L(roll(pupilF[plane K + k], shifts[s]) . maskFT)|^2>: fp32 [S], the
    derivative of a real loss with respect to the weight of every row of `shifts` ([S,2] (dy,dx), sourceShifts' list), given
    gradIntensity = dl/dI on abbeIntensity's raw image ([pn,pn], or [planes,pn,pn] for a pupil stack).  `pupilF` is [pn,pn],
    [planes,pn,pn] or, with pupilsPerPlane = K, [planes K,pn,pn]: K pupils that share one image plane (the effective pupils of
    vectorAbbeIntensity).  pn and N powers of two, 16 ... 4096.

    The list is walked in chunks of `batch` points inside one call; the workspace holds one chunk (batch planes K fields of pn^2,
    never S of them).  batch=None picks the largest chunk whose workspace stays within WORK_BYTES (256 MiB).  No atomics: sens[s]
    depends on point s alone, bit for bit, whatever the batch and the rest of the list."""
    from .imageformation import ShapeError
    who = "sourceSensitivities"
    if not isinstance(maskFT, torch.Tensor) or maskFT.dim() != 2 or maskFT.shape[0] != maskFT.shape[1]:
        raise ShapeError(f"{who}: maskFT must be a square 2-D tensor; got {tuple(getattr(maskFT, 'shape', ()))}")
    pn, N, K = int(maskFT.shape[0]), int(N), int(pupilsPerPlane)
    if K < 1:
        raise ValueError(f"{who}: pupilsPerPlane >= 1; got {K}")
    if (not isinstance(pupilF, torch.Tensor) or pupilF.dim() not in (2, 3) or tuple(pupilF.shape[-2:]) != (pn, pn)
            or (pupilF.dim() == 2 and K != 1) or (pupilF.dim() == 3 and (pupilF.shape[0] < 1 or pupilF.shape[0] % K))):
        raise ShapeError(f"{who}: pupilF must be [{pn},{pn}] or [planes * {K},{pn},{pn}] to match maskFT and pupilsPerPlane; got "
                         f"{tuple(getattr(pupilF, 'shape', ()))}")
    stacked = pupilF.dim() == 3
    planes = pupilF.shape[0] // K if stacked else 1
    if not isinstance(shifts, torch.Tensor) or shifts.dim() != 2 or shifts.shape[1] != 2 or shifts.is_floating_point():
        raise ShapeError(f"{who}: shifts must be an integer [S,2] tensor of (dy,dx) pairs; got {tuple(getattr(shifts, 'shape', ()))}")
    shapes = ((planes, pn, pn),) + (((pn, pn),) if planes == 1 else ())
    if (not isinstance(gradIntensity, torch.Tensor) or tuple(gradIntensity.shape) not in shapes or gradIntensity.is_complex()):
        raise ShapeError(f"{who}: gradIntensity must be a real tensor of shape {shapes[-1] if planes == 1 else shapes[0]} "
                         f"(abbeIntensity's image); got {tuple(getattr(gradIntensity, 'shape', ()))}")
    _pow2_size(who, "pn", pn)
    _pow2_size(who, "N", N)
    if N < pn:
        nat.check(nat.E_NSMALL, who)
    dev = nat.require_gpu(maskFT.device)
    if gradIntensity.device != dev:
        raise ShapeError(f"{who}: gradIntensity lives on {gradIntensity.device}, the mask spectrum on {dev}")
    S = int(shifts.shape[0])
    sens = torch.empty(S, dtype=torch.float32, device=dev)
    if S == 0:
        return sens
    lib = nat.lib()
    if batch is None:
        per_point = int(lib.litho_source_sensitivity_work_bytes(planes, K, 1, pn)) - planes * pn * pn * 4
        batch = max(1, min(S, (WORK_BYTES - planes * pn * pn * 4) // per_point))
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"{who}: batch >= 1; got {batch}")
    nbytes = int(lib.litho_source_sensitivity_work_bytes(planes, K, batch, pn))
    if nbytes == 0:
        raise ValueError(f"{who}: batch {batch} x {planes * K} pupils x pn {pn} exceeds the 2^31 - 1 lines of one chunk")
    m = maskFT.detach().to(torch.complex64).contiguous()
    p = pupilF.detach().to(device=dev, dtype=torch.complex64).contiguous()
    G = gradIntensity.detach().to(torch.float32).contiguous()
    sh = shifts.to(device=dev, dtype=torch.int32).contiguous()
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nat.check(lib.litho_source_sensitivity(nat.ptr(p), nat.ptr(m), nat.ptr(G), planes, K, nat.ptr(sh), S, pn, N, nat.ptr(sens),
                                               batch, nat.ptr(work), nbytes, nat.stream_ptr(dev)), "litho_source_sensitivity")
    return sens


def _candidate_mask(who, candidates, pn):
    if (not isinstance(candidates, torch.Tensor) or tuple(candidates.shape) != (pn, pn) or candidates.is_complex()):
        from .imageformation import ShapeError
        raise ShapeError(f"{who}: candidates must be a real map [{pn},{pn}] on the source grid (the mask's pixelNumber); got "
                         f"{tuple(getattr(candidates, 'shape', ()))}")
    return candidates != 0


def sourceGradient(maskFT, pupilF, candidates, N, gradIntensity):
    """The sensitivities of the lit pixels of `candidates` (a bitmap or a floating map [pn,pn], non-zero = candidate) as a map on
    the source grid: fp32 [pn,pn], dl/dw at every candidate in argwhere order -- sourceShifts' order -- and zero elsewhere."""
    pn = int(maskFT.shape[-1]) if isinstance(maskFT, torch.Tensor) else 0
    lit = _candidate_mask("sourceGradient", candidates, pn)
    dev = nat.require_gpu(maskFT.device)
    lit = lit.to(dev)
    from .lightsource import sourceShifts
    sens = sourceSensitivities(maskFT, pupilF, sourceShifts(lit, pn), N, gradIntensity)
    out = torch.zeros((pn, pn), dtype=torch.float32, device=dev)
    out[lit] = sens                                                        # boolean-mask assignment runs in argwhere order
    return out


class SourceResult:
    """What optimizeSource returns.  `losses[i]` is the loss of iterate i (0 = the start); `best` the index of the lowest;
    `source` (fp32 [pn,pn]) is that iterate's weight map, as abbeImage(weighted=True) and socsKernels take it, and `weights`
    (fp32 [S]) the same numbers on the candidate list in argwhere order."""

    def __init__(self, source, weights, losses, best):
        self.source, self.weights, self.losses, self.best = source, weights, losses, best


def sourceLossGradient(weights, target, imager, sensitivity, threshold, dose, resistSteepness, normalize=True, gradient=True):
    """(loss, dl/dw) of optimizeSource at `weights` [S], in the precision of what the hooks return: image = imager(weights), the
    un-normalised post-processed image of sum_s w_s |E_s|^2; with `normalize` it is divided by sum(w); resist =
    sigmoid(a_r (dose image - threshold)); loss = mean((resist - target)^2) over pixels and planes; G = dl/d image in closed form;
    g = sensitivity(G), one <G, image of point s> per point.  Without normalisation that is the gradient; with it,
    (g_s - <G, image>) / sum(w), the quotient rule on image / sum(w) -- <G, image> taken on the post-processed grid, where it
    equals the pairing of the adjoint-processed G with the normalised raw image.  The loss is a 0-dim tensor: nothing is read on
    the host here.  gradient=False stops after the loss and returns (loss, None)."""
    image = imager(weights)
    wsum = weights.sum()
    if normalize:
        image = image / wsum.to(image.dtype)
    loss, G = _descent.resist_loss(image, target, resistSteepness, dose, threshold, gradient)
    if not gradient:
        return loss, None
    g = sensitivity(G)
    if normalize:
        g = (g - (G * image).sum().to(g.dtype)) / wsum.to(g.dtype)
    return loss, g


def projectedStep(weights, grad, step):
    """w <- max(w - step max(w) grad / max|grad|, 0): optimizeMask's scale-free step in units of the largest weight, projected onto
    w >= 0."""
    return torch.clamp(weights - float(step) * weights.max() * grad / _descent.peak(grad), min=0)


def _device_source_model(transmission, pupilF, shifts, pn, pixelSize, deltaK, wavelength, dev):
    """(imager, sensitivity) of optimizeSource on the HIP path: the weighted Abbe sum of the fixed list through one PlanCache and
    postProcess; postProcessAdjoint and sourceSensitivities."""
    from .ilt import _Optics
    from .imageformation import abbeIntensity
    o = _Optics(pn, pixelSize, deltaK, wavelength, dev)
    M = o.spectrum(transmission)

    def imager(w):
        return o.image(abbeIntensity(M, pupilF, shifts, o.N, plan=o.cache, weights=w.contiguous())[0])

    def sensitivity(gradImage):
        return sourceSensitivities(M, pupilF, shifts, o.N, o.raw_gradient(gradImage))

    return imager, sensitivity


def optimizeSource(target, transmission, pupilF, candidates, pixelSize, deltaK, wavelength, threshold, dose=1.0, iterations=20,
                   step=0.25, resistSteepness=None, initial=None, normalize=True, imager=None, sensitivity=None):
    """Source optimisation by projected steepest descent: the non-negative weights on the lit pixels of `candidates` (a bitmap or
    a floating map [pn,pn]) under which the fixed mask `transmission` ([pn,pn], real or complex) prints closest to `target`.

    The loss is optimizeMask's: post-processed image -> resist = sigmoid(resistSteepness (dose I - threshold)) (default
    25 / |threshold|) -> mean((resist - target)^2) over the pixels and, for a pupil stack [planes,pn,pn], over the planes.
    `target`: float [n_out,n_out] on the post-processed grid.  The weights start at `initial` (a real map [pn,pn], read at the
    candidates) or at the candidates' own values.  Forward: abbeIntensity(weights=w) on the fixed candidate list through one
    PlanCache (a zero weight is legal there, so the list never changes), then postProcess; backward: postProcessAdjoint, then
    sourceSensitivities.  With `normalize` the image is divided by sum(w) and the gradient is (g_s - <G, I>) / sum(w)
    (sourceLossGradient).  Update: projectedStep.  The loss is read on the host once per iterate; an iterate whose weights are all
    zero ends the loop.  Returns a SourceResult holding the iterate with the lowest loss.

    `imager(w fp32 [S]) -> un-normalised image [n_out,n_out] or [planes,n_out,n_out]` and `sensitivity(gradient on that image) ->
    [S]` replace the device model together (then transmission and pupilF are not looked at, and the loop runs wherever `target`
    lives)."""
    who = "optimizeSource"
    if (imager is None) != (sensitivity is None):
        raise ValueError(f"{who}: imager and sensitivity replace the model and its backward pass together; give both or neither")
    iterations = int(iterations)
    if resistSteepness is None:
        resistSteepness = _descent.default_resist_steepness(threshold)
    if iterations < 1 or not float(step) > 0 or not float(resistSteepness) > 0:
        raise ValueError(f"{who}: iterations >= 1 and step, resistSteepness > 0; got {iterations}, {step}, {resistSteepness}")
    if not isinstance(target, torch.Tensor) or target.dim() != 2 or target.shape[0] != target.shape[1] or target.is_complex():
        raise ValueError(f"{who}: target must be a real [n_out,n_out] tensor; got {tuple(getattr(target, 'shape', ()))}")
    if not isinstance(candidates, torch.Tensor) or candidates.dim() != 2:
        raise ValueError(f"{who}: candidates must be a real map [pn,pn]; got {tuple(getattr(candidates, 'shape', ()))}")
    pn = int(candidates.shape[0])
    lit = _candidate_mask(who, candidates, pn)
    if imager is None:
        from .imageformation import ShapeError
        from .lightsource import sourceShifts
        _pow2_size(who, "pn", pn)
        if not isinstance(transmission, torch.Tensor) or tuple(transmission.shape) != (pn, pn):
            raise ShapeError(f"{who}: transmission must be [{pn},{pn}] like candidates; got {tuple(getattr(transmission, 'shape', ()))}")
        if not isinstance(pupilF, torch.Tensor) or pupilF.dim() not in (2, 3) or tuple(pupilF.shape[-2:]) != (pn, pn):
            raise ShapeError(f"{who}: pupilF must be [{pn},{pn}] or [planes,{pn},{pn}]; got {tuple(getattr(pupilF, 'shape', ()))}")
        dev = nat.require_gpu(pupilF.device)
        epsilon, N = nat.epsilon_n(deltaK, pixelSize, wavelength)
        _pow2_size(who, "N", int(N))
        _descent.check_image_grid(who, "target", target, pn, epsilon)
        lit = lit.to(dev)
        shifts = sourceShifts(lit, pn)
        imager, sensitivity = _device_source_model(transmission.to(dev), pupilF, shifts, pn, pixelSize, deltaK, wavelength, dev)
    else:
        dev = target.device
        lit = lit.to(dev)
    if not bool(lit.any()):
        raise ValueError(f"{who}: candidates has no lit point")
    target = target.detach().to(device=dev, dtype=torch.float32)
    start = candidates if initial is None else initial
    if not isinstance(start, torch.Tensor) or tuple(start.shape) != (pn, pn) or start.is_complex():
        raise ValueError(f"{who}: initial must be a real [{pn},{pn}] map; got {tuple(getattr(start, 'shape', ()))}")
    w = start.detach().to(device=dev, dtype=torch.float32)[lit].clone()
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or not bool((w > 0).any()):
        raise ValueError(f"{who}: the starting weights must be finite, non-negative and not all zero")
    threshold, dose, a_r = float(threshold), float(dose), float(resistSteepness)

    losses, best, best_w = [], 0, w.clone()
    for it in range(iterations + 1):
        last = it == iterations
        loss, grad = sourceLossGradient(w, target, imager, sensitivity, threshold, dose, a_r, normalize, gradient=not last)
        w_next = w if last else projectedStep(w, grad.to(w.dtype), step)
        # the one host read of this iterate: its loss, and whether the next iterate keeps a lit point
        value, lit_next = torch.stack([loss.double(), (w_next > 0).any().double()]).tolist()
        losses.append(value)
        if losses[-1] < losses[best]:
            best, best_w = it, w.clone()
        if last or not math.isfinite(losses[-1]) or not lit_next:                 # nothing lit: no image to go on with
            break
        w = w_next
    source = torch.zeros((pn, pn), dtype=torch.float32, device=dev)
    source[lit] = best_w
    return SourceResult(source, best_w, losses, best)


def optimizeSourceMask(target, pupilF, candidates, pixelSize, deltaK, wavelength, threshold, rounds=2, kernels=64, oversample=16,
                       socsIterations=2, seed=0, dose=1.0, sourceIterations=20, maskIterations=20, sourceStep=0.25, maskStep=0.25,
                       maskSteepness=4.0, resistSteepness=None, background=0, feature=1, initialSource=None, initialTheta=None,
                       normalize=True):
    """Alternating source-mask optimisation: `rounds` times [optimizeSource on the current mask; socsKernels(pupilF, weights,
    kernels=...) of the new source; optimizeMask(initial=theta) on those kernels], carrying theta and the weights from round to
    round.  Plumbing over those three calls -- every argument goes to the call that documents it (kernels, oversample,
    socsIterations, seed: socsKernels) -- with no gradient code of its own; `normalize` must stay on for the two stages to share
    one image scale when the kernel set is truncated.  theta starts at `initialTheta` or at +-1 from the target, as in
    optimizeMask.  Returns (SourceResult, ILTResult) of the last round."""
    from .ilt import optimizeMask
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError(f"optimizeSourceMask: rounds >= 1; got {rounds}")
    if not isinstance(candidates, torch.Tensor) or candidates.dim() != 2:
        raise ValueError(f"optimizeSourceMask: candidates must be a real map [pn,pn]; got {tuple(getattr(candidates, 'shape', ()))}")
    pn = int(candidates.shape[0])
    dev = nat.require_gpu(pupilF.device)
    bg, span = complex(background), complex(feature) - complex(background)
    if initialTheta is not None:
        theta = initialTheta.detach().to(device=dev, dtype=torch.float32)
    else:
        theta = torch.full((pn, pn), -1.0, dtype=torch.float32, device=dev)
        k = min(pn, target.shape[0])
        theta[:k, :k] = torch.where(target.to(dev)[:k, :k] > 0.5, 1.0, -1.0)
    weights = initialSource
    for _ in range(rounds):
        transmission = (bg + span * torch.sigmoid(float(maskSteepness) * theta)).to(torch.complex64)
        src = optimizeSource(target, transmission, pupilF, candidates, pixelSize, deltaK, wavelength, threshold, dose=dose,
                             iterations=sourceIterations, step=sourceStep, resistSteepness=resistSteepness, initial=weights,
                             normalize=normalize)
        weights = src.source
        socs = _socs.socsKernels(pupilF, weights, kernels=kernels, oversample=oversample, iterations=socsIterations, seed=seed)
        ilt = optimizeMask(target, socs, pixelSize, deltaK, wavelength, threshold, dose=dose, iterations=maskIterations,
                           step=maskStep, maskSteepness=maskSteepness, resistSteepness=resistSteepness, background=background,
                           feature=feature, initial=theta, normalize=normalize)
        theta = ilt.theta
    return src, ilt
