"""Hopkins imaging: SOCS (sum of coherent systems) kernels from the transmission cross coefficient; no reference counterpart.

abbeImage sums one field per source point.  For MANY masks through ONE optical setting (pupil + source) -- the correction loop,
EPE on every edge, process-variation bands, Bossung tables -- source and pupil go into the transmission cross coefficient once,

    T = sum_s w_s a_s a_s^H,   a_s = roll(P, d_s),   d = (row - pn/2, col - pn/2) on the source grid,

T is factored into K coherent kernels phi_k (already scaled by sqrt(lambda_k)), and every later image is K fields at shift (0,0):

    I = sum_s w_s |E_s|^2  ~=  sum_k |field(phi_k)|^2,        exact when sum_k phi_k phi_k^H = T  (K = rank).

A hard-edged pupil's eigenvalues decay algebraically, so a truncated K is an approximation with a knob: `captured` reports the
fraction sum_k lambda_k / trace T that the kept kernels carry, and nothing promises Abbe parity at small K.

`socsKernels` factors T by subspace iteration (the operator on the device: litho_tcc_apply, four pn^2 transforms per vector
whatever the number of source points; the J x J eigenproblems in float64 on the host); `hopkinsIntensity` runs the kernels as a
pupil STACK through the unchanged Abbe engine and folds the K planes (litho_socs_fold)."""
from functools import partial

import numpy as np
import torch

from . import _native as nat

MIN_PN, MAX_PN = 16, 4096
STACK_BYTES = 1 << 30            # default bound of hopkinsIntensity's intermediate stack (kernelChunk)


def _device_fft2(x, inverse=False):
    """litho_fft2_c2c in place on a contiguous complex64 [batch,n,n] (or [n,n]) device tensor."""
    n = x.shape[-1]
    with torch.cuda.device(x.device):
        nat.check(nat.lib().litho_fft2_c2c(nat.ptr(x), x.numel() // (n * n), n, 1 if inverse else 0, nat.stream_ptr(x.device)),
                  "litho_fft2_c2c")
    return x


class _DeviceOperator:
    """X -> T X on the device (litho_tcc_apply) for one pupil plane."""

    def __init__(self, pupil, weight_shifted):
        self.ph = _device_fft2(pupil.clone())
        self.w = weight_shifted

    def __call__(self, X):
        Y = torch.empty_like(X)
        n = X.shape[-1]
        with torch.cuda.device(X.device):
            nat.check(nat.lib().litho_tcc_apply(nat.ptr(self.ph), nat.ptr(self.w), nat.ptr(X), nat.ptr(Y), X.shape[0], n,
                                                nat.stream_ptr(X.device)), "litho_tcc_apply")
        return Y


def _support_box(pupil, lit, pn):
    """Rows lo/hi and columns lo/hi of [pupil box (+) shift extents], or None when it exceeds the grid (the source wraps the pupil
    around it).  Integer arithmetic on the host.  The range of T lies inside the box."""
    nz = (pupil != 0).cpu()
    rows, cols = torch.nonzero(nz.any(dim=1)).flatten(), torch.nonzero(nz.any(dim=0)).flatten()
    if rows.numel() == 0:
        raise ValueError("socsKernels: the pupil function is zero everywhere")
    lrows, lcols = torch.nonzero(lit.any(dim=1)).flatten(), torch.nonzero(lit.any(dim=0)).flatten()
    c = pn // 2
    r_lo, r_hi = int(rows[0]) + int(lrows[0]) - c, int(rows[-1]) + int(lrows[-1]) - c
    c_lo, c_hi = int(cols[0]) + int(lcols[0]) - c, int(cols[-1]) + int(lcols[-1]) - c
    if r_lo < 0 or c_lo < 0 or r_hi > pn - 1 or c_hi > pn - 1:
        return None
    return r_lo, r_hi, c_lo, c_hi


def _mask_to_box(X, box):
    """Exact zeros outside the box: without this the transforms' rounding noise hands the engine's planner a full-grid support."""
    if box is not None:
        r_lo, r_hi, c_lo, c_hi = box
        X[:, :r_lo].zero_()
        X[:, r_hi + 1:].zero_()
        X[:, :, :c_lo].zero_()
        X[:, :, c_hi + 1:].zero_()
    return X


GRAM_BLOCK = 1 << 18           # columns per float64 block of the J x J inner products


def _inner_products(A, B):
    """A B^H for complex64 A, B [J,F], accumulated in complex128 block by block of the long dimension.  These dot products run
    over all pn^2 samples, and their error becomes the kernels' norm error one for one: an fp32 matrix product on the device was
    measured 3e-5 off at F = 5e4, growing with F^2 -- six times the image tolerance.  The conversions are per block, so the
    float64 copies stay small."""
    G = torch.zeros((A.shape[0], B.shape[0]), dtype=torch.complex128, device=A.device)
    for c0 in range(0, A.shape[1], GRAM_BLOCK):
        G += A[:, c0:c0 + GRAM_BLOCK].to(torch.complex128) @ B[:, c0:c0 + GRAM_BLOCK].to(torch.complex128).conj().T
    return G


def _hermitian_eigh(G):
    """float64 eigh of a small Hermitian matrix on the host: (values, vectors), descending."""
    g = G.detach().cpu().numpy().astype(np.complex128)
    d, V = np.linalg.eigh((g + g.conj().T) / 2.0)
    return d[::-1].copy(), V[:, ::-1].copy()


def _orthonormalise(X):
    """The rows of X [J,F] recombined to an orthonormal set through their J x J Gram matrix (one pass; the callers make two,
    since the Gram matrix squares the condition number of a block that T has just stretched)."""
    d, V = _hermitian_eigh(_inner_products(X, X))
    d = np.maximum(d, d[0] * 1e-14)
    C = (V / np.sqrt(d)[None, :]).conj().T                              # Q = diag(d^-1/2) V^H X
    return torch.from_numpy(C).to(device=X.device, dtype=torch.complex64) @ X


def _factor_plane(pupil, W, lit, J, K, iterations, seed, apply, dev):
    """One plane: (kernels complex64 [K,pn,pn], eigenvalues float64 [K], box)."""
    pn = pupil.shape[-1]
    box = _support_box(pupil, lit, pn)
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    X = torch.view_as_complex(torch.randn((J, pn, pn, 2), generator=gen, dtype=torch.float32, device=dev))
    X = _mask_to_box(X, box)
    for _ in range(iterations):
        Q = _orthonormalise(_orthonormalise(X.reshape(J, pn * pn)))
        X = _mask_to_box(apply(Q.reshape(J, pn, pn).contiguous()), box)
    Q = _orthonormalise(_orthonormalise(X.reshape(J, pn * pn)))
    del X
    Y = _mask_to_box(apply(Q.reshape(J, pn, pn).contiguous()), box).reshape(J, pn * pn)
    lam, U = _hermitian_eigh(_inner_products(Y, Q).T)                    # Rayleigh-Ritz: H[j,k] = <Q_j, T Q_k>
    del Y
    lam = np.maximum(lam[:K], 0.0)
    C = (U[:, :K] * np.sqrt(lam)[None, :]).T                            # phi_k = sqrt(l_k) sum_j U[j,k] Q_j
    phi = (torch.from_numpy(np.ascontiguousarray(C)).to(device=dev, dtype=torch.complex64) @ Q).reshape(K, pn, pn)
    return _mask_to_box(phi.contiguous(), box), torch.from_numpy(lam.copy()), box


class SOCSKernels:
    """What socsKernels returns.  `kernels` complex64 [K,pn,pn] (or [planes,K,pn,pn] for a through-focus stack), already scaled
    by sqrt(lambda_k); `eigenvalues` float64, descending, [K] or [planes,K]; `trace` = sum W * sum |P|^2 = trace T (per plane);
    `captured` = sum_k lambda_k / trace, the fraction of the image's energy the kept kernels carry (1 at full rank);
    `weight_sum` = sum W (what normalize divides by); `boxes` the masking box per plane (None: the source wraps).  Holds its own
    PlanCaches, one per kernel chunk, so that from the second hopkinsIntensity on nothing is planned afresh."""

    def __init__(self, kernels, eigenvalues, trace, captured, weight_sum, lit_points, boxes):
        self.kernels, self.eigenvalues, self.trace, self.captured = kernels, eigenvalues, trace, captured
        self.weight_sum, self.lit_points, self.boxes = weight_sum, lit_points, boxes
        self.stacked = kernels.dim() == 4
        self.planes = int(kernels.shape[0]) if self.stacked else 1
        self.K, self.pn = int(kernels.shape[-3]), int(kernels.shape[-1])
        self._chunks = {}
        self._shifts = None

    def chunks(self, size):
        """[(kernel stack complex64 [planes * k, pn, pn] with item g * k + j = kernel c0 + j of plane g, its PlanCache, k)] for
        chunks of `size` kernels; made once per size, so the engine's plan records keep their tensors."""
        from .imageformation import PlanCache
        if size not in self._chunks:
            k4 = self.kernels if self.stacked else self.kernels[None]
            self._chunks[size] = [(k4[:, c0:c0 + size].reshape(-1, self.pn, self.pn).contiguous(), PlanCache(),
                                   min(size, self.K - c0)) for c0 in range(0, self.K, size)]
        return self._chunks[size]

    def shifts(self):
        if self._shifts is None:
            self._shifts = torch.zeros((1, 2), dtype=torch.int32, device=self.kernels.device)
        return self._shifts


def _weight_map(lightsource, pn):
    """float64 host copy of the source's intensity weights: an integer or bool bitmap lights its non-zero pixels with weight 1
    (abbeImage's `argwhere`), a floating map carries the weights themselves."""
    if not isinstance(lightsource, torch.Tensor) or tuple(lightsource.shape) != (pn, pn) or lightsource.is_complex():
        raise ValueError(f"socsKernels: the source must be a real bitmap or weight map [{pn},{pn}] (the pupil's grid); got "
                         f"{tuple(getattr(lightsource, 'shape', ()))}")
    src = lightsource.detach().cpu()
    if not src.is_floating_point():
        return (src != 0).to(torch.float64)
    W = src.to(torch.float64)
    if not bool(torch.isfinite(W).all()) or bool((W < 0).any()):
        raise ValueError("socsKernels: a source weight is negative or not finite")
    return W


def socsKernels(pupilF, lightsource, kernels=64, oversample=16, iterations=2, seed=0, applier=None):
    """SOCS kernels of one optical setting.  `pupilF` complex [pn,pn] or a through-focus stack [planes,pn,pn], factored plane by
    plane; `lightsource` the pn x pn bitmap or grey map abbeImage / sourceWeights take (non-zero = lit, a floating map's values
    are the intensity weights, a bitmap means weight 1).  pn must be a power of two, 16 ... 4096 (ValueError otherwise; embedded
    odd sizes are not built), and a negative or non-finite weight raises ValueError.

    Subspace iteration on J = min(kernels + oversample, lit points) vectors -- more than the lit points would only add normalised
    rounding noise: a random start, `iterations` rounds of [orthonormalise twice through the J x J Gram matrix, apply T], then a
    Rayleigh-Ritz step on Q^H T Q.  The large products are torch matmuls on the pupil's device (the pn^2-long inner products
    accumulated in float64), every J x J eigenproblem is float64 on the host.  After every application and in the result the
    vectors are exact zeros outside the box [pupil box (+) shift extents] (skipped when the source wraps the pupil around the
    grid).

    `applier`: a callable X -> T X on complex64 [J,pn,pn] (one per plane for a stack) instead of litho_tcc_apply; the host
    algebra then runs wherever the pupil lives, CPU included."""
    if not isinstance(pupilF, torch.Tensor) or pupilF.dim() not in (2, 3) or pupilF.shape[-1] != pupilF.shape[-2]:
        raise ValueError(f"socsKernels: pupilF must be [pn,pn] or [planes,pn,pn]; got {tuple(getattr(pupilF, 'shape', ()))}")
    pn, stacked = int(pupilF.shape[-1]), pupilF.dim() == 3
    planes = int(pupilF.shape[0]) if stacked else 1

    def planes_of(W, dev):
        P = pupilF.detach().to(dtype=torch.complex64).reshape(planes, pn, pn).contiguous()
        wsh = torch.fft.ifftshift(W).to(torch.float32).to(dev).contiguous()
        wsum = float(W.sum())
        for Pp in P:
            yield Pp, wsum * float((Pp.real.double() ** 2 + Pp.imag.double() ** 2).sum()), partial(_DeviceOperator, Pp, wsh)

    return _factorise("socsKernels", pupilF.device, pn, planes, stacked, lightsource, 1, planes_of, kernels=kernels,
                      oversample=oversample, iterations=iterations, seed=seed, applier=applier)


def _factorise(who, device, pn, planes, stacked, lightsource, rank, planes_of, *, kernels, oversample, iterations, seed, applier):
    """The driver of socsKernels and vectorSocsKernels (`who` in the messages): the checks, the weight map and its lit points,
    J = min(kernels + oversample, rank * lit points) with `rank` the caller's bound on rank T per lit point, the appliers, the
    planes through _factor_plane with seed + p, the SOCSKernels.  The caller's part is `planes_of(W, dev)`, which yields per
    plane (the support handed to _factor_plane, trace T, a callable that makes the device operator)."""
    if pn < MIN_PN or pn > MAX_PN or pn & (pn - 1):
        raise ValueError(f"{who}: pn must be a power of two, {MIN_PN} ... {MAX_PN}; got {pn}")
    kernels, oversample, iterations = int(kernels), int(oversample), int(iterations)
    if kernels < 1 or oversample < 0 or iterations < 1:
        raise ValueError(f"{who}: kernels >= 1, oversample >= 0, iterations >= 1; got {kernels}, {oversample}, {iterations}")
    W = _weight_map(lightsource, pn)
    lit = W > 0
    S = int(lit.sum())
    if S == 0:
        raise ValueError(f"{who}: the source has no lit point")
    J = min(kernels + oversample, rank * S)
    K = min(kernels, J)
    if applier is None:
        dev = nat.require_gpu(device)
        appliers = None
    else:
        dev = device
        appliers = list(applier) if isinstance(applier, (list, tuple)) else [applier]
        if len(appliers) != planes:
            raise ValueError(f"{who}: {len(appliers)} appliers for {planes} pupil planes")
    phis, lams, traces, boxes = [], [], [], []
    for p, (support, trace, operator) in enumerate(planes_of(W, dev)):
        apply = appliers[p] if appliers is not None else operator()
        phi, lam, box = _factor_plane(support, W, lit, J, K, iterations, seed + p, apply, dev)
        phis.append(phi)
        lams.append(lam)
        boxes.append(box)
        traces.append(trace)
    trace = torch.tensor(traces, dtype=torch.float64)
    lam = torch.stack(lams)
    captured = lam.sum(dim=1) / trace
    wsum = float(W.sum())
    if stacked:
        return SOCSKernels(torch.stack(phis), lam, trace, captured, wsum, S, boxes)
    return SOCSKernels(phis[0], lam[0], float(trace[0]), float(captured[0]), wsum, S, boxes)


def _check_socs(who, maskFT, socs):
    """What every consumer of a kernel set checks of `socs` and `maskFT`; returns the device both live on."""
    from .imageformation import ShapeError
    if not isinstance(socs, SOCSKernels):
        raise TypeError(f"{who}: socs must be the SOCSKernels socsKernels returned")
    pn = socs.pn
    if not isinstance(maskFT, torch.Tensor) or maskFT.dim() != 2 or tuple(maskFT.shape) != (pn, pn):
        raise ShapeError(f"maskFT must be [{pn},{pn}] to match the kernels; got {tuple(getattr(maskFT, 'shape', ()))}")
    dev = nat.require_gpu(maskFT.device)
    if socs.kernels.device != dev:
        raise ShapeError(f"the kernels live on {socs.kernels.device}, the mask spectrum on {dev}")
    return dev


def _kernel_chunk(who, kernelChunk, socs, itemsize):
    """Kernels per chunk: `kernelChunk`, or by default what keeps a stack of `itemsize` bytes per sample under STACK_BYTES."""
    if kernelChunk is None:
        kernelChunk = max(1, STACK_BYTES // (socs.planes * socs.pn * socs.pn * itemsize))
    kernelChunk = int(kernelChunk)
    if kernelChunk < 1:
        raise ValueError(f"{who}: kernelChunk must be >= 1; got {kernelChunk}")
    return min(kernelChunk, socs.K)


def _accumulate_into(out, want, dtype, dev):
    """(out, given): the tensor a result is written to, allocated when `out` is None and accumulated into when it is given."""
    from .imageformation import ShapeError
    if out is None:
        return torch.empty(want, dtype=dtype, device=dev), False
    name = str(dtype).split(".")[-1]
    if not isinstance(out, torch.Tensor):
        raise ShapeError(f"out must be a contiguous {name} tensor of shape {want} on {dev}; got {type(out).__name__}")
    if out.dtype != dtype or not out.is_contiguous() or out.device != dev or tuple(out.shape) != want:
        raise ShapeError(f"out must be a contiguous {name} tensor of shape {want} on {dev}; got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}, contiguous={out.is_contiguous()}")
    return out, True


def _stack_and_fold(maskFT, stack, shifts, N, planes, k, out, accumulate, **engine):
    """out[g] (+)= sum_j |field of stack[g k + j]|^2: the pupil stack [planes * k, pn, pn] through abbeIntensity into a zeroed
    fp32 stack (`engine`: its plan, options, weights), then litho_socs_fold."""
    from .imageformation import abbeIntensity
    pn, dev = int(stack.shape[-1]), out.device
    fields = torch.zeros((planes * k, pn, pn), dtype=torch.float32, device=dev)
    abbeIntensity(maskFT, stack, shifts, N, out=fields, **engine)
    with torch.cuda.device(dev):
        nat.check(nat.lib().litho_socs_fold(nat.ptr(fields), planes, k, pn * pn, nat.ptr(out), 1 if accumulate else 0,
                                            nat.stream_ptr(dev)), "litho_socs_fold")


def hopkinsIntensity(maskFT, socs, N, out=None, options=None, kernelChunk=None):
    """sum_k |field of kernel k|^2: the raw fp32 intensity [pn,pn] (or [planes,pn,pn] for kernels of a pupil stack) BEFORE
    post-processing, as abbeIntensity returns it -- K fields per image instead of one per source point.  Each chunk of kernels
    runs as a pupil stack through abbeIntensity (shift (0,0), the chunk's own PlanCache: from the second image on nothing is
    planned afresh and nothing waits for the stream) and litho_socs_fold sums its planes into the image.  `kernelChunk` bounds
    the intermediate stack, chunk * planes * pn^2 * 4 bytes (default: the whole set, or what keeps it under 1 GiB); the result
    depends on it only through the order of the fp32 fold.  `out`: accumulated into when given, as abbeIntensity does.
    `options`: launch-planner options for the engine calls."""
    dev = _check_socs("hopkinsIntensity", maskFT, socs)
    pn, planes = socs.pn, socs.planes
    size = _kernel_chunk("hopkinsIntensity", kernelChunk, socs, 4)
    out, given = _accumulate_into(out, (planes, pn, pn) if socs.stacked else (pn, pn), torch.float32, dev)
    for i, (stack, cache, k) in enumerate(socs.chunks(size)):
        _stack_and_fold(maskFT, stack, socs.shifts(), N, planes, k, out, given or i > 0, plan=cache, options=options)
    return out


def hopkinsIntensityBatch(maskFTs, socs, N, out=None, tileChunk=None):
    """hopkinsIntensity's image for MANY mask spectra in one call per chunk: fp32 [B,pn,pn] (or [B,planes,pn,pn] for the kernels
    of a pupil stack) from `maskFTs` complex [B,pn,pn] -- the windows of a tiled layout (tiling.py), the masks of a correction
    loop.  litho_socs_image_batch (csrc/socs_grad.hip): B x K fields in two row passes, the sum over the kernels kept in LDS in
    the second, so no K-plane stack is written; one running fp32 sum per pixel in kernel order, no atomics.  This is NOT
    hopkinsIntensity's route (the Abbe engine and litho_socs_fold), so the two agree to rounding and not bit for bit.

    `tileChunk` spectra go into one native call; it bounds the workspace, chunk * planes * (K * 8 + 4) * pn^2 bytes (default:
    what keeps it under STACK_BYTES, at least 1; where a single spectrum's workspace is larger than that, the kernels are walked
    in chunks as well, each continuing the running sums of the one before).  A spectrum's bits depend on that spectrum and the
    kernels alone: not on B, on its place in the batch or on `tileChunk`.  `out`: accumulated into when given."""
    from .imageformation import ShapeError
    if not isinstance(socs, SOCSKernels):
        raise TypeError("hopkinsIntensityBatch: socs must be the SOCSKernels socsKernels returned")
    pn, planes, K = socs.pn, socs.planes, socs.K
    if (not isinstance(maskFTs, torch.Tensor) or not maskFTs.is_complex() or maskFTs.dim() != 3 or maskFTs.shape[0] < 1
            or tuple(maskFTs.shape[-2:]) != (pn, pn)):
        raise ShapeError(f"maskFTs must be a complex tensor [B,{pn},{pn}] to match the kernels; got "
                         f"{getattr(maskFTs, 'dtype', type(maskFTs).__name__)} {tuple(getattr(maskFTs, 'shape', ()))}")
    dev = nat.require_gpu(maskFTs.device)
    if socs.kernels.device != dev:
        raise ShapeError(f"the kernels live on {socs.kernels.device}, the mask spectra on {dev}")
    B = int(maskFTs.shape[0])
    cells = pn * pn
    if tileChunk is None:
        tileChunk = max(1, STACK_BYTES // (planes * (K * 8 + 4) * cells))
    tileChunk = int(tileChunk)
    if tileChunk < 1:
        raise ValueError(f"hopkinsIntensityBatch: tileChunk must be >= 1; got {tileChunk}")
    tileChunk = min(tileChunk, B)
    size = K if planes * (K * 8 + 4) * cells <= STACK_BYTES else max(1, (STACK_BYTES // (planes * cells) - 4) // 8)
    m = maskFTs.detach().to(torch.complex64).contiguous()
    out, given = _accumulate_into(out, (B, planes, pn, pn) if socs.stacked else (B, pn, pn), torch.float32, dev)
    lib = nat.lib()
    work = None
    for b0 in range(0, B, tileChunk):
        nb = min(tileChunk, B - b0)
        for i, (stack, _, k) in enumerate(socs.chunks(min(size, K))):
            nbytes = int(lib.litho_socs_image_batch_work_bytes(nb, planes, k, pn))
            if nbytes == 0:
                raise ValueError(f"hopkinsIntensityBatch: {nb} spectra x {planes} planes x {k} kernels at pn {pn} are more lines than "
                                 "one call takes; pass a smaller tileChunk")
            if work is None or work.numel() < nbytes:
                work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                nat.check(lib.litho_socs_image_batch(nat.ptr(stack), nat.ptr(m[b0]), nb, planes, k, pn, int(N), nat.ptr(out[b0]),
                                                     1 if (given or i > 0) else 0, nat.ptr(work), work.numel(), nat.stream_ptr(dev)),
                          "litho_socs_image_batch")
    return out


def hopkinsImage(mask, maskFT, socs, pixelSize, deltaK, wavelength, normalize=False, options=None, kernelChunk=None):
    """abbeImage's post-processing (|.|, bilinear resample by 1 / epsilon, zero pad) on top of hopkinsIntensity: the same return
    shape as abbeImage with the pupil (stack) and source the kernels were made from.  `normalize` divides by the sum of the
    source weights (the number of lit points of a bitmap), as abbeImage does."""
    from .imageformation import postProcess
    from .mask import Mask
    epsilon, N = Mask.calculateEpsilonN(self=mask, deltaK=deltaK, pixelSize=pixelSize, wavelength=wavelength)
    raw = hopkinsIntensity(maskFT, socs, N, options=options, kernelChunk=kernelChunk)
    if normalize and socs.weight_sum > 0:
        raw /= float(socs.weight_sum)
    return postProcess(raw, epsilon)
