"""Mask gradients through Hopkins imaging and a pixel-based inverse-lithography loop; no reference counterpart (the reference's
README lists a "2D solver for lithography recipe generation" among its open goals).

With F[q,i] = exp(+2 pi i (i - c)(q - c) / N), c = pn / 2, the engine's chain at shift (0,0) is L(X) = F X F^T, the coherent fields
of a SOCS kernel set are E_k = L(phi_k . M) and hopkinsIntensity returns I = sum_k |E_k|^2.  For a real loss l with G = dl/dI,

    g = dl/dRe M + i dl/dIm M = 2 sum_p sum_k conj(phi_pk) . L^H(G_p . E_pk),        L^H(Y) = conj(F) Y conj(F)^T,

torch's convention for the gradient of a complex leaf (dl = Re <g, dM>).  `hopkinsGradient` computes g on the device
(litho_socs_vjp: K fields and K adjoint fields per call, csrc/socs_grad.hip); `maskSpectrumAdjoint` and `postProcessAdjoint` are
the adjoints of the two linear bookends (mask transmission -> spectrum, raw intensity -> image), and `optimizeMask` descends a
pixel mask through all of it; `bakedResistModel` replaces its constant-threshold resist by the post-exposure bake of a chemically
amplified resist and its adjoint (peb.py), through optimizeMask's imager= / adjoint= pair.  Mask gradients only: the source and the pupil are constants here (source gradients: smo.py;
DESIGN.md section 10)."""
import math

import numpy as np
import torch

from . import _descent
from . import _native as nat
from . import socs as _socs
from .imageformation import PlanCache, postProcess
from .mask import Mask
from .socs import SOCSKernels

MAX_N = _socs.MAX_PN              # litho_fft2_c2c's and litho_socs_fields' largest transform: one limit, stated in socs.py


def _checked(what, maskFT, socs):
    """socs._check_socs, and the spectrum as the kernels take it: (maskFT as contiguous complex64, device)."""
    dev = _socs._check_socs(what, maskFT, socs)
    return maskFT.detach().to(torch.complex64).contiguous(), dev


def hopkinsFields(maskFT, socs, N):
    """The coherent fields E_k = L(phi_k . maskFT) behind hopkinsIntensity: complex64 [K,pn,pn], or [planes,K,pn,pn] for the
    kernels of a pupil stack (litho_socs_fields).  sum_k |E_k|^2 is hopkinsIntensity's image; the engine keeps that sum only."""
    m, dev = _checked("hopkinsFields", maskFT, socs)
    kernels = socs.kernels.contiguous()
    fields = torch.empty_like(kernels)
    with torch.cuda.device(dev):
        nat.check(nat.lib().litho_socs_fields(nat.ptr(kernels), nat.ptr(m), socs.planes * socs.K, socs.pn, int(N), nat.ptr(fields),
                                              nat.stream_ptr(dev)), "litho_socs_fields")
    return fields


def hopkinsGradient(maskFT, socs, N, gradIntensity, out=None, kernelChunk=None):
    """g = dl/dRe maskFT + i dl/dIm maskFT of a real loss l, given gradIntensity = dl/dI on hopkinsIntensity's image (real,
    [pn,pn], or [planes,pn,pn] for the kernels of a pupil stack): complex64 [pn,pn], by the formula at the head of this file.
    Each chunk of kernels is one litho_socs_vjp call -- its fields, G . E, L^H, and the sum over the chunk in ascending order with
    one running fp32 sum per element (no atomics: two calls give the same bits).  `kernelChunk` bounds the field stack,
    chunk * planes * pn^2 * 8 bytes (default: the whole set, or what keeps it under socs.STACK_BYTES); the result depends on it
    only through the order of the fp32 sum.  `out`: accumulated into when given, as hopkinsIntensity does."""
    from .imageformation import ShapeError
    m, dev = _checked("hopkinsGradient", maskFT, socs)
    pn, planes = socs.pn, socs.planes
    want = (planes, pn, pn) if socs.stacked else (pn, pn)
    if (not isinstance(gradIntensity, torch.Tensor) or tuple(gradIntensity.shape) != want or gradIntensity.is_complex()
            or gradIntensity.device != dev):
        raise ShapeError(f"gradIntensity must be a real tensor of shape {want} on {dev} (hopkinsIntensity's image); got "
                         f"{getattr(gradIntensity, 'dtype', type(gradIntensity).__name__)} "
                         f"{tuple(getattr(gradIntensity, 'shape', ()))} on {getattr(gradIntensity, 'device', None)}")
    size = _socs._kernel_chunk("hopkinsGradient", kernelChunk, socs, 8)
    out, given = _socs._accumulate_into(out, (pn, pn), torch.complex64, dev)
    G = gradIntensity.detach().to(torch.float32).contiguous()
    work = None
    for i, (stack, _, k) in enumerate(socs.chunks(size)):
        nbytes = int(nat.lib().litho_socs_vjp_work_bytes(planes, k, pn))
        if work is None or work.numel() < nbytes:
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            nat.check(nat.lib().litho_socs_vjp(nat.ptr(stack), nat.ptr(m), nat.ptr(G), planes, k, pn, int(N), nat.ptr(out),
                                               1 if (given or i > 0) else 0, nat.ptr(work), work.numel(), nat.stream_ptr(dev)),
                      "litho_socs_vjp")
    return out


def hopkinsGradientBatch(maskFTs, socs, N, gradIntensities, out=None, tileChunk=None):
    """hopkinsGradient for MANY mask spectra: complex64 [B,pn,pn] from `maskFTs` complex [B,pn,pn] and `gradIntensities` real
    [B,pn,pn] (or [B,planes,pn,pn] for the kernels of a pupil stack), the layout of hopkinsIntensityBatch's image -- the windows
    of a tiled inverse-lithography loop (tiling.optimizeMaskTiled).  Each chunk of `tileChunk` spectra is ONE litho_socs_vjp_batch
    call on the whole kernel set (csrc/socs_grad.hip): the fields of every (spectrum, kernel) are left transposed, the adjoint
    transform runs on (G . E)^T, and the sum over the kernels is folded into its last row pass (pn <= 2048; at 4096 the adjoints
    are stored and reduced spectrum by spectrum).  `tileChunk` bounds the workspace, chunk * planes * (K * 8 + 4) * pn^2 bytes
    (default: what keeps it under socs.STACK_BYTES, at least 1).  A spectrum's bits depend on that spectrum, its gradient and the
    kernels alone: not on B, on its place in the batch or on `tileChunk`.  The sum runs in another order of transforms than
    hopkinsGradient's, so the two agree to rounding and not bit for bit.  `out`: accumulated into when given."""
    from .imageformation import ShapeError
    if not isinstance(socs, SOCSKernels):
        raise TypeError("hopkinsGradientBatch: socs must be the SOCSKernels socsKernels returned")
    pn, planes, K = socs.pn, socs.planes, socs.K
    if (not isinstance(maskFTs, torch.Tensor) or not maskFTs.is_complex() or maskFTs.dim() != 3 or maskFTs.shape[0] < 1
            or tuple(maskFTs.shape[-2:]) != (pn, pn)):
        raise ShapeError(f"maskFTs must be a complex tensor [B,{pn},{pn}] to match the kernels; got "
                         f"{getattr(maskFTs, 'dtype', type(maskFTs).__name__)} {tuple(getattr(maskFTs, 'shape', ()))}")
    if socs.kernels.device != maskFTs.device:
        raise ShapeError(f"the kernels live on {socs.kernels.device}, the mask spectra on {maskFTs.device}")
    dev = nat.require_gpu(maskFTs.device)
    B = int(maskFTs.shape[0])
    want = (B, planes, pn, pn) if socs.stacked else (B, pn, pn)
    if (not isinstance(gradIntensities, torch.Tensor) or tuple(gradIntensities.shape) != want or gradIntensities.is_complex()
            or gradIntensities.device != dev):
        raise ShapeError(f"gradIntensities must be a real tensor of shape {want} on {dev} (hopkinsIntensityBatch's image); got "
                         f"{getattr(gradIntensities, 'dtype', type(gradIntensities).__name__)} "
                         f"{tuple(getattr(gradIntensities, 'shape', ()))} on {getattr(gradIntensities, 'device', None)}")
    if tileChunk is None:
        tileChunk = max(1, _socs.STACK_BYTES // (planes * (K * 8 + 4) * pn * pn))
    tileChunk = int(tileChunk)
    if tileChunk < 1:
        raise ValueError(f"hopkinsGradientBatch: tileChunk must be >= 1; got {tileChunk}")
    tileChunk = min(tileChunk, B)
    out, given = _socs._accumulate_into(out, (B, pn, pn), torch.complex64, dev)
    m = maskFTs.detach().to(torch.complex64).contiguous()
    G = gradIntensities.detach().to(torch.float32).contiguous().reshape(B, planes, pn, pn)
    kernels = socs.kernels.contiguous()
    lib = nat.lib()
    work = None
    for b0 in range(0, B, tileChunk):
        nb = min(tileChunk, B - b0)
        nbytes = int(lib.litho_socs_vjp_batch_work_bytes(nb, planes, K, pn))
        if nbytes == 0:
            raise ValueError(f"hopkinsGradientBatch: {nb} spectra x {planes} planes x {K} kernels at pn {pn} are more lines than one "
                             "call takes; pass a smaller tileChunk")
        if work is None or work.numel() < nbytes:
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            nat.check(lib.litho_socs_vjp_batch(nat.ptr(kernels), nat.ptr(m[b0]), nat.ptr(G[b0]), nb, planes, K, pn, int(N),
                                               nat.ptr(out[b0]), 1 if given else 0, nat.ptr(work), work.numel(), nat.stream_ptr(dev)),
                      "litho_socs_vjp_batch")
    return out


class _HopkinsIntensityAD(torch.autograd.Function):
    @staticmethod
    def forward(ctx, maskFT, socs, N):
        ctx.save_for_backward(maskFT)
        ctx.socs, ctx.N = socs, N
        return _socs.hopkinsIntensity(maskFT.detach(), socs, N)

    @staticmethod
    def backward(ctx, gradIntensity):
        (maskFT,) = ctx.saved_tensors
        return hopkinsGradient(maskFT, ctx.socs, ctx.N, gradIntensity), None, None


def hopkinsIntensityAD(maskFT, socs, N):
    """hopkinsIntensity as a differentiable torch function of maskFT: the forward is the unchanged hopkinsIntensity, the backward
    hopkinsGradient, so loss.backward() reaches a complex `maskFT` leaf.  It adds no arithmetic of its own; the kernels, the
    source and the pupil behind them are constants.  maskFT must be complex64, the precision both directions compute in: a
    complex128 leaf would get a gradient of fp32 accuracy in a float64 dtype, so it is refused (ShapeError)."""
    from .imageformation import ShapeError
    if not isinstance(maskFT, torch.Tensor) or maskFT.dtype != torch.complex64:
        raise ShapeError(f"hopkinsIntensityAD: maskFT must be a complex64 tensor; got {getattr(maskFT, 'dtype', type(maskFT).__name__)}")
    return _HopkinsIntensityAD.apply(maskFT, socs, N)


# ---- the linear bookends ---------------------------------------------------------------------------------------------------------
def resizeMatrix(n_in, scale):
    """(R fp32 [n_out, n_in], n_out): the bilinear resize of the mask-spectrum pre-step and of the post-process along one axis, so
    that the 2-D resize is R t R^T.  torch's rule (F.interpolate, bilinear, align_corners=False, scale_factor given), restated as
    the forward kernels restate it: n_out = floor(n_in * scale); the reciprocal scale is kept in fp32; source coordinate
    src = max(fl32(rs * (dst + 0.5) - 0.5), 0), one rounding; i0 = floor(src), i1 = min(i0 + 1, n_in - 1), weights
    l1 = src - i0 and l0 = 1 - l1 in fp32 (two per row, summed where i0 = i1).  Equal sizes are a copy: None."""
    n_in, scale = int(n_in), float(scale)
    n_out = int(math.floor(n_in * scale))
    if n_out == n_in:
        return None, n_out
    if n_out < 1:
        raise ValueError(f"resizeMatrix: scale {scale} leaves no sample of {n_in}")
    rs = np.float32(1.0 / scale)
    dst = np.arange(n_out, dtype=np.float64)
    src = np.maximum((np.float64(rs) * (dst + 0.5) - 0.5).astype(np.float32), np.float32(0.0))   # the product is exact in double
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1.0) - l1).astype(np.float32)
    R = np.zeros((n_out, n_in), dtype=np.float32)
    rows = np.arange(n_out)
    R[rows, i0] = l0
    R[rows, i1] += l1
    return torch.from_numpy(R), n_out


def _unpad(z, lead, n):
    """Adjoint of `pad with `lead` samples in front` (negative: a crop) on the last two axes of z [.., P, P], back to [.., n, n]:
    out[s] = z[s + lead] where that exists, zero elsewhere."""
    P = z.shape[-1]
    lo, hi = max(0, -lead), min(n, P - lead)
    if lo == 0 and hi == n:
        return z[..., lead:lead + n, lead:lead + n]
    out = torch.zeros(z.shape[:-2] + (n, n), dtype=z.dtype, device=z.device)
    out[..., lo:hi, lo:hi] = z[..., lo + lead:hi + lead, lo + lead:hi + lead]
    return out


def _resize_adjoint(z, R):
    """R^T z R on the last two axes (z real or complex, R real); the copy when R is None."""
    if R is None:
        return z
    R = R.to(z.device)
    if z.is_complex():
        return torch.complex(R.T @ z.real @ R, R.T @ z.imag @ R)
    return R.T @ z @ R


def maskSpectrumAdjoint(gradSpectrum, pn, epsilon, N, transform=None):
    """S^H of the mask-spectrum chain S (Mask.fraunhofer / litho_mask_spectrum_complex: bilinear resize by epsilon, pad or crop
    to N, centred forward DFT, centre pn x pn): complex64 [pn,pn] from gradSpectrum complex [pn,pn].  If g is the gradient of a
    real loss with respect to the spectrum (hopkinsGradient), S^H g is its gradient with respect to the complex transmission.
    In order: the centre pn x pn embedded in N x N zeros; the adjoint of fftshift . fft2 . fftshift, which is the same shifts
    around the unscaled inverse DFT (litho_fft2_c2c); the adjoint of the pad or crop; the transposed resize R^T z R with the dense
    matrix of `resizeMatrix` (torch matmuls on the device).  N: a power of two, 16 ... 4096 (the transform's limit), >= pn.
    `transform`: a callable replacing the device's inverse DFT on a complex [N,N] tensor (then nothing needs a GPU)."""
    pn, N = int(pn), int(N)
    if N < 16 or N > MAX_N or N & (N - 1):
        raise ValueError(f"maskSpectrumAdjoint: N must be a power of two, 16 ... {MAX_N} (litho_fft2_c2c); got {N}")
    if pn < 2 or pn % 2 or N < pn or not float(epsilon) > 0:
        raise ValueError(f"maskSpectrumAdjoint: pn even, 2 ... N, and epsilon > 0; got pn {pn}, N {N}, epsilon {epsilon}")
    if not isinstance(gradSpectrum, torch.Tensor) or tuple(gradSpectrum.shape) != (pn, pn):
        from .imageformation import ShapeError
        raise ShapeError(f"gradSpectrum must be [{pn},{pn}]; got {tuple(getattr(gradSpectrum, 'shape', ()))}")
    if transform is None:
        nat.require_gpu(gradSpectrum.device)
        transform = lambda x: _socs._device_fft2(x, inverse=True)               # noqa: E731
    g = gradSpectrum.detach().to(torch.complex64)
    trim = (N - pn) // 2
    z = torch.zeros((N, N), dtype=torch.complex64, device=g.device)
    z[trim:trim + pn, trim:trim + pn] = g
    z = torch.fft.ifftshift(transform(torch.fft.fftshift(z).contiguous()))      # N is even: both shifts are the roll by N / 2
    R, ns = resizeMatrix(pn, float(epsilon))
    return _resize_adjoint(_unpad(z, (N - ns) // 2, ns), R).contiguous()


def postProcessAdjoint(gradImage, pn, epsilon):
    """The adjoint of postProcess: fp32 [pn,pn] (or [planes,pn,pn]) from the gradient on the post-processed grid [n_out,n_out]
    (or [planes,n_out,n_out]; n_out = litho_postprocess_size) -- the zero pad undone, then the transposed resize R^T z R for the
    resample by 1 / epsilon.  postProcess also takes |raw|; on a sum of squares that is the identity, and it is ignored here."""
    pn = int(pn)
    scale = 1.0 / float(epsilon)
    R, ns = resizeMatrix(pn, scale)
    lead = (pn - round(pn / float(epsilon))) // 2
    n_out = ns + 2 * lead + ns % 2
    if (not isinstance(gradImage, torch.Tensor) or gradImage.dim() not in (2, 3) or gradImage.is_complex()
            or tuple(gradImage.shape[-2:]) != (n_out, n_out)):
        from .imageformation import ShapeError
        raise ShapeError(f"gradImage must be [{n_out},{n_out}] or [planes,{n_out},{n_out}] (the post-processed grid of pn {pn}, "
                         f"epsilon {epsilon}); got {tuple(getattr(gradImage, 'shape', ()))}")
    g = gradImage.detach().to(torch.float32)
    return _resize_adjoint(_unpad(g, lead, ns), R).contiguous()


# ---- pixel-based inverse lithography ---------------------------------------------------------------------------------------------
class ILTResult:
    """What optimizeMask returns.  `losses[i]` is the loss of iterate i (0 = the start, `iterations` = after the last update);
    `best` the index of the lowest; `theta` (fp32 [pn,pn]), `transmission` (complex64 [pn,pn], the continuous mask
    background + (feature - background) sigmoid(maskSteepness theta)) and `mask` (bool [pn,pn], theta > 0) are that iterate's."""

    def __init__(self, theta, transmission, losses, best):
        self.theta, self.transmission, self.mask = theta, transmission, theta > 0
        self.losses, self.best = losses, best


class _Optics:
    """What the device models of optimizeMask, optimizeSource and fitAberrations build around their intensity call: `epsilon` and
    `N` of the grid, the spectrum `M` of the transmission last given to `spectrum`, a PlanCache (`cache`) for Abbe calls on a
    fixed source list, and the two linear bookends with the normalisation `gain` folded in: raw intensity -> image, and the
    gradient on the image -> the gradient on the raw intensity.  The gain multiplies in place and is skipped at 1.0; the bits of
    the loops depend on both."""

    def __init__(self, pn, pixelSize, deltaK, wavelength, dev, gain=1.0):
        self.pn, self.pixelSize, self.dev, self.gain = pn, pixelSize, dev, gain
        self.epsilon, self.N = nat.epsilon_n(deltaK, pixelSize, wavelength)
        self.M, self.cache = None, PlanCache()

    def spectrum(self, transmission):
        self.M = Mask(transmission=transmission, pixelSize=self.pixelSize, device=self.dev)._ffFraunhofer(self.epsilon, self.N)
        return self.M

    def image(self, raw):
        if self.gain != 1.0:
            raw *= self.gain
        return postProcess(raw, self.epsilon)

    def raw_gradient(self, gradImage):
        graw = postProcessAdjoint(gradImage, self.pn, self.epsilon)
        if self.gain != 1.0:
            graw *= self.gain
        return graw


def _device_model(socs, pn, pixelSize, deltaK, wavelength, normalize, dev):
    """(imager, adjoint) of optimizeMask on the HIP path."""
    o = _Optics(pn, pixelSize, deltaK, wavelength, dev, 1.0 / float(socs.weight_sum) if normalize and socs.weight_sum > 0 else 1.0)

    def imager(transmission):
        return o.image(_socs.hopkinsIntensity(o.spectrum(transmission), socs, o.N))

    def adjoint(gradImage):
        return maskSpectrumAdjoint(hopkinsGradient(o.M, socs, o.N, o.raw_gradient(gradImage)), pn, o.epsilon, o.N)

    return imager, adjoint


def bakedResistModel(socs, resist, thickness, pixelSize, deltaK, wavelength, intensityScale=1.0, normalize=True, steps=None):
    """(imager, adjoint) for optimizeMask(imager=, adjoint=): inverse lithography against a chemically amplified resist instead of
    a constant threshold.  imager(t) is the device model's image (spectrum -> hopkinsIntensity -> postProcess) x `intensityScale`
    -> postExposureBake, and returns the deprotection 1 - m after the bake as [planes, n_out, n_out]; the planes of `socs` are the
    depths of the resist, top first, as vectorSocsKernels(film=, depths=) makes them (a single kernel set is one plane).
    adjoint(g) is postExposureBakeGradient with gradInhibitor = -g, x `intensityScale`, then the device model's adjoint.  With it
    optimizeMask's `threshold` is a deprotection level (for example 1 - mTh of the Mack resist that develops it), its `dose`
    stays 1 and the exposure dose rides in `intensityScale` (the image is in the engine's units: intensityScale = dose / clear
    field puts C in units of the clear-field dose).  `resist`: a ChemicallyAmplifiedResist; `steps`: postExposureBake's.
    Development is not differentiated here: the loss sits on the latent image that development thresholds.  developedResistModel
    is the model whose loss sits on the developed profile."""
    from .peb import ChemicallyAmplifiedResist, postExposureBake, postExposureBakeGradient
    if not isinstance(socs, SOCSKernels):
        raise TypeError("bakedResistModel: socs must be the SOCSKernels socsKernels returned")
    if not isinstance(resist, ChemicallyAmplifiedResist):
        raise TypeError("bakedResistModel: resist must be a ChemicallyAmplifiedResist")
    scale = float(intensityScale)
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError(f"bakedResistModel: intensityScale must be positive and finite; got {intensityScale}")
    dev = nat.require_gpu(socs.kernels.device)
    optics, optics_adjoint = _device_model(socs, int(socs.pn), pixelSize, deltaK, wavelength, normalize, dev)
    state = {}

    def imager(transmission):
        image = optics(transmission) * scale
        state["I"] = image if image.dim() == 3 else image[None]
        return 1.0 - postExposureBake(state["I"], resist, thickness, pixelSize, steps=steps).inhibitor[0]

    def adjoint(gradDeprotection):
        g = gradDeprotection.detach().to(torch.float32).reshape(state["I"].shape)
        gI = postExposureBakeGradient(state["I"], resist, thickness, pixelSize, gradInhibitor=-g[None], steps=steps) * scale
        return optics_adjoint(gI if socs.stacked else gI[0])

    return imager, adjoint


def developedResistModel(socs, resist, thickness, pixelSize, deltaK, wavelength, developTime, intensityScale=1.0, normalize=True,
                         steps=None, maxIterations=1024):
    """(imager, adjoint) for optimizeMask(imager=, adjoint=): inverse lithography against the DEVELOPED profile.  imager(t) is the
    device model's image x `intensityScale` -> the slowness of `resist` (a MackResist: developmentRate; a
    ChemicallyAmplifiedResist: postExposureBake with `steps`) -> developmentTime, and returns the development margin
    1 - min(T, 2 developTime) / developTime as [planes, n_out, n_out]: positive where the plane is developed at `developTime`, -1
    where the developer arrives late or never.  The planes of `socs` are the depths of the resist, top first, as in
    bakedResistModel.  adjoint(g) carries g through the margin (zero where it is clamped), developmentTimeGradient, the rate and,
    for a chemically amplified resist, the bake backwards, x `intensityScale`, then the device model's adjoint.  Use it with
    optimizeMask(threshold=0), whose default resistSteepness is then 25 (per unit of margin), and dose 1; the exposure dose rides
    in `intensityScale`.  `maxIterations` caps the launches of the forward and of the adjoint solver alike."""
    from .develop import (MackResist, _development_time, developmentRate, developmentRateGradient, developmentTimeGradient)
    from .peb import ChemicallyAmplifiedResist, amplifiedRateGradient, postExposureBake, postExposureBakeGradient
    who = "developedResistModel"
    if not isinstance(socs, SOCSKernels):
        raise TypeError(f"{who}: socs must be the SOCSKernels socsKernels returned")
    if not isinstance(resist, (MackResist, ChemicallyAmplifiedResist)):
        raise TypeError(f"{who}: resist must be a MackResist or a ChemicallyAmplifiedResist")
    scale, t_dev = float(intensityScale), float(developTime)
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError(f"{who}: intensityScale must be positive and finite; got {intensityScale}")
    if not (t_dev > 0.0 and math.isfinite(t_dev)):
        raise ValueError(f"{who}: developTime must be positive and finite; got {developTime}")
    if not 1 <= int(maxIterations) <= 65536:
        raise ValueError(f"{who}: maxIterations must be 1 ... 65536; got {maxIterations}")
    amplified = isinstance(resist, ChemicallyAmplifiedResist)
    dev = nat.require_gpu(socs.kernels.device)
    optics, optics_adjoint = _device_model(socs, int(socs.pn), pixelSize, deltaK, wavelength, normalize, dev)
    state = {}

    def imager(transmission):
        image = optics(transmission) * scale
        I = state["I"] = image if image.dim() == 3 else image[None]
        if amplified:
            bake = postExposureBake(I, resist, thickness, pixelSize, steps=steps)
            state["a"], s = bake.acidDose, bake.slowness
        else:
            s = developmentRate(I, resist, thickness, pixelSize)
        state["s"] = s
        state["T"] = _development_time(s, thickness, pixelSize, maxIterations)[0]
        return 1.0 - torch.clamp(state["T"][0], max=2.0 * t_dev) / t_dev

    def adjoint(gradMargin):
        T = state["T"]
        g = gradMargin.detach().to(torch.float32).reshape(T.shape)
        gT = torch.where(T < 2.0 * t_dev, g * (-1.0 / t_dev), torch.zeros_like(g))
        gs = developmentTimeGradient(state["s"], T, gT, thickness, pixelSize, maxIterations)
        if amplified:
            ga = amplifiedRateGradient(state["a"], resist, thickness, gs)
            gI = postExposureBakeGradient(state["I"], resist, thickness, pixelSize, gradAcidDose=ga, steps=steps)
        else:
            gI = developmentRateGradient(state["I"], resist, thickness, pixelSize, (1.0,), gs)
        gI = gI * scale
        return optics_adjoint(gI if socs.stacked else gI[0])

    return imager, adjoint


def optimizeMask(target, socs, pixelSize, deltaK, wavelength, threshold, dose=1.0, iterations=20, step=0.25, maskSteepness=4.0,
                 resistSteepness=None, background=0, feature=1, initial=None, normalize=True, imager=None, adjoint=None):
    """Pixel-based inverse lithography by steepest descent: the mask whose printed resist image is closest to `target`.

    theta real [pn,pn] (+-1 from the target, or `initial`); transmission t = background + (feature - background) .
    sigmoid(maskSteepness theta) -- complex values allowed, so an attenuated phase-shift mask works; then spectrum ->
    hopkinsIntensity -> postProcess -> resist = sigmoid(resistSteepness (dose I - threshold)) (resistSteepness in inverse image
    units; default 25 / |threshold|), and the loss is
    mean((resist - target)^2) over the pixels and, for the kernels of a through-focus stack, over the planes (process-window ILT:
    the gradient on the image is per plane).  `target`: float [n_out,n_out] on the post-processed grid (litho_postprocess_size).
    The backward pass is postProcessAdjoint, hopkinsGradient, maskSpectrumAdjoint; the pointwise loss and sigmoid arithmetic is
    torch on the device.  Update: theta <- theta - step grad / max|grad| (no learning rate to tune against an unknown gradient
    scale); the loss is read on the host once per iterate.  `normalize` divides the image by the sum of the source weights, as
    hopkinsImage does.  Returns an ILTResult holding the iterate with the lowest loss.

    `imager(transmission complex64 [pn,pn]) -> image [n_out,n_out] or [planes,n_out,n_out]` and `adjoint(gradient on that
    image) -> complex gradient [pn,pn] on the transmission last imaged` replace the device model together (then `socs` needs
    only `.pn`, and the loop runs wherever `target` lives)."""
    if (imager is None) != (adjoint is None):
        raise ValueError("optimizeMask: imager and adjoint replace the model and its backward pass together; give both or neither")
    iterations = int(iterations)
    if resistSteepness is None:
        resistSteepness = _descent.default_resist_steepness(threshold)
    if iterations < 1 or not float(step) > 0 or not float(maskSteepness) > 0 or not float(resistSteepness) > 0:
        raise ValueError(f"optimizeMask: iterations >= 1 and step, maskSteepness, resistSteepness > 0; got {iterations}, {step}, "
                         f"{maskSteepness}, {resistSteepness}")
    if complex(feature) == complex(background):
        raise ValueError("optimizeMask: feature and background transmissions are equal; nothing to optimise")
    pn = int(socs.pn)
    if not isinstance(target, torch.Tensor) or target.dim() != 2 or target.shape[0] != target.shape[1] or target.is_complex():
        raise ValueError(f"optimizeMask: target must be a real [n_out,n_out] tensor; got {tuple(getattr(target, 'shape', ()))}")
    if imager is None:
        if not isinstance(socs, SOCSKernels):
            raise TypeError("optimizeMask: socs must be the SOCSKernels socsKernels returned")
        dev = nat.require_gpu(socs.kernels.device)
        _descent.check_image_grid("optimizeMask", "target", target, pn, nat.epsilon_n(deltaK, pixelSize, wavelength)[0])
        imager, adjoint = _device_model(socs, pn, pixelSize, deltaK, wavelength, normalize, dev)
    else:
        dev = target.device
    target = target.detach().to(device=dev, dtype=torch.float32)
    if initial is not None:
        if not isinstance(initial, torch.Tensor) or tuple(initial.shape) != (pn, pn) or initial.is_complex():
            raise ValueError(f"optimizeMask: initial must be a real [{pn},{pn}] tensor; got {tuple(getattr(initial, 'shape', ()))}")
        theta = initial.detach().to(device=dev, dtype=torch.float32).clone()
    else:
        theta = torch.full((pn, pn), -1.0, dtype=torch.float32, device=dev)
        k = min(pn, target.shape[0])                                              # the two grids share their first sample
        theta[:k, :k] = torch.where(target[:k, :k] > 0.5, 1.0, -1.0)
    bg, span = complex(background), complex(feature) - complex(background)
    a_m, a_r, dose, threshold = float(maskSteepness), float(resistSteepness), float(dose), float(threshold)

    def transmission_of(th):
        return (bg + span * torch.sigmoid(a_m * th)).to(torch.complex64)

    losses, best, best_theta = [], 0, theta.clone()
    for it in range(iterations + 1):
        s = torch.sigmoid(a_m * theta)
        image = imager((bg + span * s).to(torch.complex64))
        loss, grad_image = _descent.resist_loss(image, target, a_r, dose, threshold, gradient=it < iterations)
        losses.append(float(loss))                                                 # the one host read of this iterate
        if losses[-1] < losses[best]:
            best, best_theta = it, theta.clone()
        if it == iterations or not math.isfinite(losses[-1]):
            break
        grad_t = adjoint(grad_image)                                               # dl/dRe t + i dl/dIm t
        grad_theta = a_m * s * (1.0 - s) * (grad_t * span.conjugate()).real       # dl = Re(conj(grad_t) dt), dt = span s' dtheta
        theta = theta - float(step) * grad_theta / _descent.peak(grad_theta, torch.float32)   # the floor of theta's precision
    return ILTResult(best_theta, transmission_of(best_theta), losses, best)
