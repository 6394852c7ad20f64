"""Pupil gradients of Abbe imaging, wavefront and Zernike sensitivities, and aberration retrieval; no reference counterpart.

With E_{s,j} = L(roll(P_j, d_s) . M) and I_g = sum_s w_s sum_{k < K} |E_{s,g K + k}|^2 (abbeIntensity(weights=), L and roll as in
smo.py), a real loss l with G_g = dl/dI_g has, in torch's convention for a complex leaf (dl = Re <g, dP>),

    g_j[r][c] = 2 sum_s w_s conj(M[r'][c']) A_{s,j}[r'][c'],   r' = (r + dy_s) mod pn, c' = (c + dx_s) mod pn,
    A_{s,j} = L^H(G_{j / K} . E_{s,j}):

one forward and one adjoint field per source point (`pupilGradient`: litho_pupil_vjp, csrc/socs_grad.hip).  SOCS cannot serve
here, its kernels come from a TCC that depends on the pupil.  Where P = a . exp(2 pi i W) with a real and independent of W, the
wavefront gradient is dl/dW = 2 pi Im(g . conj(P)) (`wavefrontGradient`), and for W_p = W0_p + sum_j c_j B_j with real basis maps
shared by all planes, dl/dc_j = sum_p sum_cells (dl/dW_p) . B_j (`aberrationGradient`: litho_pupil_project).  `zernikeBasis` gives
the B_j of OSA indices, `fitAberrations` descends the coefficients of a scanner from measured images of a known mask.

This is the fp32 wavefront model: W is summed in fp32 and goes through generatePhi.  The reference's fp16 Zernike sum
(Pupil(...), litho_pupil) rounds W to fp16 after every term and is not differentiable at that granularity; it keeps its parity
path untouched.  K > 1 returns the gradient with respect to each given pupil and stops there: the chain from effective vector or
film pupils back to Zernikes is not built."""
import math
from functools import partial

import torch

from . import _descent
from . import _native as nat
from . import smo as _smo


_pow2_size = partial(_descent.pow2_size, entry="litho_pupil_vjp")


def pupilGradient(maskFT, pupilF, shifts, N, gradIntensity, weights=None, pupilsPerPlane=1, batch=None, out=None):
    """g = dl/dRe P + i dl/dIm P of the head of the file: complex64 with `pupilF`'s shape ([pn,pn], [planes,pn,pn] or, with
    pupilsPerPlane = K, [planes K,pn,pn]), given gradIntensity = dl/dI on abbeIntensity's raw image ([pn,pn], or [planes,pn,pn]
    for a stack), the rows of `shifts` ([S,2] (dy,dx), sourceShifts' list) and their `weights` (real [S]; None = all 1).  pn and N
    powers of two, 16 ... 4096.

    The list is walked in chunks of `batch` points inside one call; the workspace holds one chunk (batch planes K fields of pn^2,
    never S of them).  batch=None picks the largest chunk whose workspace stays within smo.WORK_BYTES (256 MiB).  No atomics, and
    every cell sums the points in list order: the result's bits do not depend on `batch`; `out` (complex64, pupilF's shape) is
    added to instead of started from zero, so a list split over two calls gives the bits of one.  An empty list gives zeros (or
    leaves `out` alone)."""
    from .imageformation import ShapeError
    who = "pupilGradient"
    if not isinstance(maskFT, torch.Tensor) or maskFT.dim() != 2 or maskFT.shape[0] != maskFT.shape[1]:
        raise ShapeError(f"{who}: maskFT must be a square 2-D tensor; got {tuple(getattr(maskFT, 'shape', ()))}")
    pn, N, K = int(maskFT.shape[0]), int(N), int(pupilsPerPlane)
    if K < 1:
        raise ValueError(f"{who}: pupilsPerPlane >= 1; got {K}")
    if (not isinstance(pupilF, torch.Tensor) or pupilF.dim() not in (2, 3) or tuple(pupilF.shape[-2:]) != (pn, pn)
            or (pupilF.dim() == 2 and K != 1) or (pupilF.dim() == 3 and (pupilF.shape[0] < 1 or pupilF.shape[0] % K))):
        raise ShapeError(f"{who}: pupilF must be [{pn},{pn}] or [planes * {K},{pn},{pn}] to match maskFT and pupilsPerPlane; got "
                         f"{tuple(getattr(pupilF, 'shape', ()))}")
    planes = pupilF.shape[0] // K if pupilF.dim() == 3 else 1
    if not isinstance(shifts, torch.Tensor) or shifts.dim() != 2 or shifts.shape[1] != 2 or shifts.is_floating_point():
        raise ShapeError(f"{who}: shifts must be an integer [S,2] tensor of (dy,dx) pairs; got {tuple(getattr(shifts, 'shape', ()))}")
    S = int(shifts.shape[0])
    shapes = ((planes, pn, pn),) + (((pn, pn),) if planes == 1 else ())
    if (not isinstance(gradIntensity, torch.Tensor) or tuple(gradIntensity.shape) not in shapes or gradIntensity.is_complex()):
        raise ShapeError(f"{who}: gradIntensity must be a real tensor of shape {shapes[-1] if planes == 1 else shapes[0]} "
                         f"(abbeIntensity's image); got {tuple(getattr(gradIntensity, 'shape', ()))}")
    if weights is not None and (not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (S,) or weights.is_complex()):
        raise ShapeError(f"{who}: weights must be a real tensor of shape ({S},), one per row of shifts; got "
                         f"{tuple(getattr(weights, 'shape', ()))}")
    _pow2_size(who, "pn", pn)
    _pow2_size(who, "N", N)
    if N < pn:
        nat.check(nat.E_NSMALL, who)
    dev = nat.require_gpu(maskFT.device)
    if gradIntensity.device != dev:
        raise ShapeError(f"{who}: gradIntensity lives on {gradIntensity.device}, the mask spectrum on {dev}")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.complex64 or tuple(out.shape) != tuple(pupilF.shape)
                            or out.device != dev or not out.is_contiguous()):
        raise ShapeError(f"{who}: out must be a contiguous complex64 tensor of shape {tuple(pupilF.shape)} on {dev}; got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))}")
    lib = nat.lib()
    if batch is None:
        batch = max(1, min(S, _smo.WORK_BYTES // (planes * K * pn * pn * 8)))
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"{who}: batch >= 1; got {batch}")
    nbytes = int(lib.litho_pupil_vjp_work_bytes(planes, K, batch, pn))
    if nbytes == 0:
        raise ValueError(f"{who}: batch {batch} x {planes * K} pupils x pn {pn} exceeds the 2^31 - 1 lines of one chunk")
    m = maskFT.detach().to(torch.complex64).contiguous()
    p = pupilF.detach().to(device=dev, dtype=torch.complex64).contiguous()
    G = gradIntensity.detach().to(torch.float32).contiguous()
    sh = shifts.to(device=dev, dtype=torch.int32).contiguous()
    w = None if weights is None else weights.detach().to(device=dev, dtype=torch.float32).contiguous()
    grad = out if out is not None else torch.empty(tuple(pupilF.shape), dtype=torch.complex64, device=dev)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nat.check(lib.litho_pupil_vjp(nat.ptr(p), nat.ptr(m), nat.ptr(G), planes, K, nat.ptr(sh), None if w is None else nat.ptr(w),
                                      S, pn, N, nat.ptr(grad), 0 if out is None else 1, batch, nat.ptr(work), nbytes,
                                      nat.stream_ptr(dev)), "litho_pupil_vjp")
    return grad


def wavefrontGradient(pupilGrad, pupilF):
    """dl/dW = 2 pi Im(g . conj(P)) for P = a . exp(2 pi i W), a real and independent of W: the real map (or maps) with the
    pupils' shape and the precision of the inputs, W in waves.  Elementwise, wherever the tensors live."""
    if (not isinstance(pupilGrad, torch.Tensor) or not isinstance(pupilF, torch.Tensor) or tuple(pupilGrad.shape) != tuple(pupilF.shape)
            or not pupilGrad.is_complex() or not pupilF.is_complex()):
        from .imageformation import ShapeError
        raise ShapeError(f"wavefrontGradient: pupilGrad and pupilF must be complex tensors of one shape; got "
                         f"{tuple(getattr(pupilGrad, 'shape', ()))} and {tuple(getattr(pupilF, 'shape', ()))}")
    return 2.0 * math.pi * (pupilGrad * pupilF.conj()).imag


def zernikeBasis(indices, pixelNumber, device):
    """fp32 [J,pn,pn]: generateZ(m, n, pn, 1.0) of every OSA index in `indices` (OSAindexToMN), converted to fp32 -- the terms
    of the pupil's own Zernike sum at coefficient 1, in waves, zero outside the unit disc."""
    from .pupil import OSAindexToMN, generateZ
    indices = [int(j) for j in indices]
    if not indices or min(indices) < 0:
        raise ValueError(f"zernikeBasis: at least one OSA index, none negative; got {indices}")
    dev = nat.require_gpu(device)
    return torch.stack([generateZ(*OSAindexToMN(j), int(pixelNumber), 1.0, dev).to(torch.float32) for j in indices])


def aberrationGradient(pupilGrad, pupilF, basis):
    """dl/dc_j = sum_planes sum_cells 2 pi Im(g . conj(P)) . basis[j]: fp32 [J] from pupilGrad and pupilF (complex64 [pn,pn] or
    [planes,pn,pn]) and basis (real [J,pn,pn], shared by the planes), on the device (litho_pupil_project: a two-stage reduction of
    fixed order without atomics -- two calls give the same bits)."""
    from .imageformation import ShapeError
    who = "aberrationGradient"
    if (not isinstance(pupilF, torch.Tensor) or pupilF.dim() not in (2, 3) or pupilF.shape[-1] != pupilF.shape[-2]
            or not isinstance(pupilGrad, torch.Tensor) or tuple(pupilGrad.shape) != tuple(pupilF.shape)):
        raise ShapeError(f"{who}: pupilGrad and pupilF must share one shape [pn,pn] or [planes,pn,pn]; got "
                         f"{tuple(getattr(pupilGrad, 'shape', ()))} and {tuple(getattr(pupilF, 'shape', ()))}")
    pn = int(pupilF.shape[-1])
    planes = int(pupilF.shape[0]) if pupilF.dim() == 3 else 1
    if (not isinstance(basis, torch.Tensor) or basis.dim() != 3 or tuple(basis.shape[-2:]) != (pn, pn) or basis.shape[0] < 1
            or basis.is_complex()):
        raise ShapeError(f"{who}: basis must be a real [J,{pn},{pn}] tensor; got {tuple(getattr(basis, 'shape', ()))}")
    _pow2_size(who, "pn", pn)
    J = int(basis.shape[0])
    dev = nat.require_gpu(pupilGrad.device)
    lib = nat.lib()
    nbytes = int(lib.litho_pupil_project_work_bytes(planes, J, pn))
    if nbytes == 0:
        raise ValueError(f"{who}: {J} basis maps x {planes} planes x pn {pn} is outside litho_pupil_project's sizes")
    g = pupilGrad.detach().to(torch.complex64).contiguous()
    p = pupilF.detach().to(device=dev, dtype=torch.complex64).contiguous()
    b = basis.detach().to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty(J, dtype=torch.float32, device=dev)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nat.check(lib.litho_pupil_project(nat.ptr(g), nat.ptr(p), planes, nat.ptr(b), J, pn, nat.ptr(out), nat.ptr(work), nbytes,
                                          nat.stream_ptr(dev)), "litho_pupil_project")
    return out


class AberrationResult:
    """What fitAberrations returns.  `losses[i]` is the loss of iterate i (0 = the start) and `steps[i]` the step length that led
    to it from the best iterate before it (steps[0] = 0); `best` is the index of the lowest loss and `coefficients` (fp32 [J], in
    waves) that iterate's."""

    def __init__(self, coefficients, losses, best, steps):
        self.coefficients, self.losses, self.best, self.steps = coefficients, losses, best, steps


def _device_aberration_model(transmission, shifts, weights, basis, baseWavefront, pn, pixelSize, deltaK, wavelength, normalize, dev):
    """(imager, gradient) of fitAberrations on the HIP path."""
    from .ilt import _Optics
    from .imageformation import abbeIntensity
    from .pupil import generatePhi
    o = _Optics(pn, pixelSize, deltaK, wavelength, dev, 1.0 / float(weights.double().sum()) if normalize else 1.0)
    M = o.spectrum(transmission)

    def pupils(c):
        W = torch.tensordot(c.to(torch.float32), basis, dims=1)             # the fp32 wavefront, in waves
        if baseWavefront is None:
            return generatePhi(W, pn, dev)
        return torch.stack([generatePhi(W0 + W, pn, dev) for W0 in baseWavefront])

    def imager(c):
        return o.image(abbeIntensity(M, pupils(c), shifts, o.N, plan=o.cache, weights=weights)[0])

    def gradient(c, gradImage):
        P = pupils(c)
        return aberrationGradient(pupilGradient(M, P, shifts, o.N, o.raw_gradient(gradImage), weights=weights), P, basis)

    return imager, gradient


def fitAberrations(measured, transmission, source, basis, pixelSize, deltaK, wavelength, baseWavefront=None, initial=None,
                   iterations=20, step=0.02, normalize=True, imager=None, gradient=None):
    """Aberration retrieval by steepest descent: the coefficients c (fp32 [J], in waves) of the wavefront basis `basis`
    ([J,pn,pn], zernikeBasis) under which the known mask `transmission` ([pn,pn], real or complex) images closest to `measured`
    ([n_out,n_out], or [planes,n_out,n_out] for a through-focus stack, on the post-processed grid).

    The device model, per iterate: W_p = baseWavefront_p + sum_j c_j B_j in fp32 (`baseWavefront` [planes,pn,pn]: the defocus
    planes of a through-focus stack, in waves; None: one plane with W0 = 0) -> generatePhi -> abbeIntensity(weights=) on the fixed
    shift list of `source`'s lit pixels ([pn,pn], a bitmap or a weight map) through one PlanCache -> postProcess, divided by
    sum(w) with `normalize` -> loss = mean((image - measured)^2) over pixels and planes.  Backward: G = 2 (image - measured) /
    count in closed form -> postProcessAdjoint -> pupilGradient -> aberrationGradient.  This is the fp32 wavefront model (head of
    the file), not the fp16 sum of Pupil(...).

    Update: c <- c - step . grad / max|grad|, `step` in waves.  When an iterate's loss is not below the best so far, the loop
    returns to the best iterate and halves `step`.  The loss is read on the host once per iterate.  `c` starts at `initial`
    ([J]) or at zero.  Returns an AberrationResult holding the iterate with the lowest loss.

    `imager(c fp32 [J]) -> image like measured` and `gradient(c, dl/d image) -> dl/dc [J]` replace the device model together
    (then transmission, source and baseWavefront are not looked at, `basis` gives J alone, and the loop runs wherever `measured`
    lives)."""
    who = "fitAberrations"
    if (imager is None) != (gradient is None):
        raise ValueError(f"{who}: imager and gradient replace the model and its backward pass together; give both or neither")
    iterations = int(iterations)
    if iterations < 1 or not float(step) > 0:
        raise ValueError(f"{who}: iterations >= 1 and step > 0; got {iterations}, {step}")
    if (not isinstance(measured, torch.Tensor) or measured.dim() not in (2, 3) or measured.shape[-1] != measured.shape[-2]
            or measured.is_complex()):
        raise ValueError(f"{who}: measured must be a real [n_out,n_out] or [planes,n_out,n_out] tensor; got "
                         f"{tuple(getattr(measured, 'shape', ()))}")
    if not isinstance(basis, torch.Tensor) or basis.dim() != 3 or basis.shape[0] < 1 or basis.shape[1] != basis.shape[2] or basis.is_complex():
        raise ValueError(f"{who}: basis must be a real [J,pn,pn] tensor; got {tuple(getattr(basis, 'shape', ()))}")
    J, pn = int(basis.shape[0]), int(basis.shape[-1])
    if imager is None:
        from .imageformation import ShapeError
        from .lightsource import sourceShifts
        _pow2_size(who, "pn", pn)
        if not isinstance(transmission, torch.Tensor) or tuple(transmission.shape) != (pn, pn):
            raise ShapeError(f"{who}: transmission must be [{pn},{pn}] like the basis maps; got {tuple(getattr(transmission, 'shape', ()))}")
        if not isinstance(source, torch.Tensor) or tuple(source.shape) != (pn, pn) or source.is_complex():
            raise ShapeError(f"{who}: source must be a real map [{pn},{pn}] on the source grid; got {tuple(getattr(source, 'shape', ()))}")
        lit = source != 0
        planes = measured.shape[0] if measured.dim() == 3 else 1
        if baseWavefront is None and measured.dim() == 3:
            raise ShapeError(f"{who}: a stack of measured images needs baseWavefront [planes,{pn},{pn}]")
        if baseWavefront is not None and (not isinstance(baseWavefront, torch.Tensor) or baseWavefront.is_complex() or measured.dim() != 3
                                          or tuple(baseWavefront.shape) != (planes, pn, pn)):
            raise ShapeError(f"{who}: baseWavefront must be a real [planes,{pn},{pn}] tensor with measured [planes,n_out,n_out]; got "
                             f"{tuple(getattr(baseWavefront, 'shape', ()))} and {tuple(measured.shape)}")
        dev = nat.require_gpu(measured.device)
        epsilon, N = nat.epsilon_n(deltaK, pixelSize, wavelength)
        _pow2_size(who, "N", int(N))
        _descent.check_image_grid(who, "measured", measured, pn, epsilon, per_plane=True)
        lit = lit.to(dev)
        if not bool(lit.any()):
            raise ValueError(f"{who}: source has no lit point")
        weights = source.to(device=dev, dtype=torch.float32)[lit].contiguous()
        if not bool(torch.isfinite(weights).all()) or bool((weights < 0).any()):
            raise ValueError(f"{who}: the source weights must be finite and non-negative")
        basis = basis.detach().to(device=dev, dtype=torch.float32).contiguous()
        W0 = None if baseWavefront is None else baseWavefront.detach().to(device=dev, dtype=torch.float32)
        imager, gradient = _device_aberration_model(transmission.to(dev), sourceShifts(lit, pn), weights, basis, W0, pn, pixelSize,
                                                    deltaK, wavelength, normalize, dev)
    else:
        dev = measured.device
    measured = measured.detach().to(device=dev, dtype=torch.float32)
    if initial is None:
        c = torch.zeros(J, dtype=torch.float32, device=dev)
    elif not isinstance(initial, torch.Tensor) or tuple(initial.shape) != (J,) or initial.is_complex():
        raise ValueError(f"{who}: initial must be a real [{J}] tensor; got {tuple(getattr(initial, 'shape', ()))}")
    else:
        c = initial.detach().to(device=dev, dtype=torch.float32).clone()

    step = float(step)
    losses, steps, best, best_c, direction, taken = [], [], 0, c, None, 0.0
    for it in range(iterations + 1):
        image = imager(c)
        diff = image - measured.to(image.dtype)
        losses.append(float((diff * diff).mean()))                             # the one host read of this iterate
        steps.append(taken)
        if not math.isfinite(losses[-1]):
            break
        improved = it == 0 or losses[-1] < losses[best]
        if improved:
            best, best_c = it, c
        if it == iterations:
            break
        if improved:
            grad = gradient(c, (2.0 / diff.numel()) * diff).to(c.dtype)
            direction = grad / _descent.peak(grad)
        else:
            step *= 0.5                                                        # back to the best iterate with half the step
        c, taken = best_c - step * direction, step
    return AberrationResult(best_c.clone(), losses, best, steps)
