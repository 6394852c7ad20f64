"""Forward-mode Hopkins imaging: the mask-error factor, EPE Jacobians and what a MEEF-matrix correction step needs; no reference
counterpart.

The image is quadratic in the mask spectrum, so its tangent along a direction dM is exact and cheap: with E_k = L(phi_k . M) and
the L of hopkinsFields,

    dI = 2 sum_k Re( conj(E_k) . L(phi_k . dM) ),

K more forward fields per direction, folded against the primal fields (`hopkinsTangent`: litho_socs_jvp, csrc/socs_grad.hip; no
adjoint transform, no tape).  The chain around it, link by link:

  * fragment biases -> coverage: `edgeCoverageTangent`, the first-order change of the exact-area coverage when the fragments of a
    Manhattan layout move along their normals.  Built on the host in float64 and uploaded -- a fragment touches spacing / pixel
    cells, so this is no hot path and has no device kernel;
  * coverage -> spectrum: the mask-spectrum chain (resize, pad, centred DFT, crop) is LINEAR, so its tangent is the chain itself on
    the direction, `Mask(transmission=dt)._ffFraunhofer(epsilon, N)`; there is no code for it here.  For a phase-shift mask the
    caller multiplies the coverage tangent by (feature - background) first;
  * spectrum -> raw image: `hopkinsTangent`;
  * raw image -> image: `postProcessTangent`, the linear part of postProcess (the exact transpose of ilt.postProcessAdjoint);
  * image -> EPE / CD: `measureEPETangent` and `measureCDTangent`, the exact derivatives of the two piecewise formulas
    (litho_measure_epe_jvp, litho_measure_cd_jvp: the primal's own search, then the derivative of the interval it chose).

`epeJacobian` strings them together, one forward pass per fragment giving every site at once (the adjoint code prices the same
matrix at one backward pass per site); `maskErrorFactor` is the one-direction case dCD_printed / dCD_mask.  metrology.correctLayout
(step="meef") uses the Jacobian as its model.  Mask tangents only: the pupil and the source are constants here, there is no
threshold or dose direction (the primal's ils already gives -1 / ILS), and the Jacobian is dense."""
import ctypes
import math

import numpy as np
import torch

from . import _native as nat
from . import socs as _socs
from .metrology import LayoutSites, _counter_clockwise, _window_origin, biasLayout, layoutSites, measureEPE

MAX_DIRECTIONS = 16               # LITHO_SOCS_JVP_MAX_DIRECTIONS: directions per native call; the wrappers chunk any P


def hopkinsTangent(maskFT, socs, N, dMaskFT, out=None, kernelChunk=None):
    """dI = 2 sum_k Re(conj(E_k) . L(phi_k . dM_p)) for every direction p: fp32 [P,pn,pn] (or [P,planes,pn,pn] for the kernels of a
    pupil stack) from `dMaskFT` complex [P,pn,pn] (a single [pn,pn] counts as P = 1) -- the directional derivative of
    hopkinsIntensity's image along dM_p, exact since the image is quadratic.  Any P, in chunks of 16 per litho_socs_jvp call; a
    direction's bits depend neither on P nor on its neighbours.  Each chunk of kernels is one call per direction chunk, one running
    fp32 sum per element in kernel order (no atomics: two calls give the same bits).  `kernelChunk` bounds the two field stacks,
    2 * chunk * planes * pn^2 * 8 bytes (default: the whole set, or what keeps them under socs.STACK_BYTES); the result depends on
    it only through the order of the fp32 sum.  `out`: accumulated into when given, as hopkinsGradient does."""
    from .imageformation import ShapeError
    dev = _socs._check_socs("hopkinsTangent", maskFT, socs)
    pn, planes = socs.pn, socs.planes
    if (not isinstance(dMaskFT, torch.Tensor) or not dMaskFT.is_complex() or dMaskFT.dim() not in (2, 3)
            or tuple(dMaskFT.shape[-2:]) != (pn, pn) or dMaskFT.shape[0] < 1 or dMaskFT.device != dev):
        raise ShapeError(f"dMaskFT must be a complex tensor [P,{pn},{pn}] on {dev} (directions of the mask spectrum); got "
                         f"{getattr(dMaskFT, 'dtype', type(dMaskFT).__name__)} {tuple(getattr(dMaskFT, 'shape', ()))} on "
                         f"{getattr(dMaskFT, 'device', None)}")
    m = maskFT.detach().to(torch.complex64).contiguous()
    dM = dMaskFT.detach().to(torch.complex64).reshape(-1, pn, pn).contiguous()
    P = int(dM.shape[0])
    size = _socs._kernel_chunk("hopkinsTangent", kernelChunk, socs, 16)
    out, given = _socs._accumulate_into(out, (P, planes, pn, pn) if socs.stacked else (P, pn, pn), torch.float32, dev)
    lib = nat.lib()
    work = None
    for i, (stack, _, k) in enumerate(socs.chunks(size)):
        for p0 in range(0, P, MAX_DIRECTIONS):
            nb = min(MAX_DIRECTIONS, P - p0)
            nbytes = int(lib.litho_socs_jvp_work_bytes(planes, k, nb, pn))
            if work is None or work.numel() < nbytes:
                work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                nat.check(lib.litho_socs_jvp(nat.ptr(stack), nat.ptr(m), nat.ptr(dM[p0]), nb, planes, k, pn, int(N), nat.ptr(out[p0]),
                                             1 if (given or i > 0) else 0, nat.ptr(work), work.numel(), nat.stream_ptr(dev)),
                          "litho_socs_jvp")
    return out


def _pad(z, lead, n_out):
    """`lead` zero samples in front of the last two axes of z [.., n, n] and zeros up to n_out (negative lead: a crop) -- the pad of
    postProcess, out[s + lead] = z[s] where that exists; the transpose of ilt._unpad."""
    n = z.shape[-1]
    lo, hi = max(0, -lead), min(n, n_out - lead)
    out = torch.zeros(z.shape[:-2] + (n_out, n_out), dtype=z.dtype, device=z.device)
    out[..., lo + lead:hi + lead, lo + lead:hi + lead] = z[..., lo:hi, lo:hi]
    return out


def postProcessTangent(dRaw, pn, epsilon):
    """The linear map of postProcess on a SIGNED tangent: fp32 [.., n_out, n_out] from dRaw [.., pn, pn] -- the bilinear resample by
    1 / epsilon as R z R^T (ilt.resizeMatrix) and the pad that ilt.postProcessAdjoint undoes, its exact transpose.  postProcess
    itself takes |raw| first; on a sum of squares that is the identity, and a tangent must keep its sign."""
    from .ilt import resizeMatrix
    pn = int(pn)
    if (not isinstance(dRaw, torch.Tensor) or dRaw.dim() < 2 or dRaw.is_complex() or tuple(dRaw.shape[-2:]) != (pn, pn)):
        from .imageformation import ShapeError
        raise ShapeError(f"dRaw must be a real tensor [..,{pn},{pn}]; got {tuple(getattr(dRaw, 'shape', ()))}")
    R, ns = resizeMatrix(pn, 1.0 / float(epsilon))
    lead = (pn - round(pn / float(epsilon))) // 2
    n_out = ns + 2 * lead + ns % 2
    z = dRaw.detach().to(torch.float32)
    if R is not None:
        R = R.to(z.device)
        z = R @ z @ R.T
    return _pad(z, lead, n_out).contiguous()


def _fragment_cells(sites, bias, pn, ps, origin):
    """(rows, cols, fragment, weight) of the coverage tangent: fragment i, displaced by bias[i] along its normal, lies with
    weight * pixelSize^2 nanometres of its length in pixel (row, col).  A fragment that lies exactly on a pixel boundary counts half
    for either side (the symmetric derivative)."""
    nrm = sites.normal
    if np.any((nrm[:, 0] != 0.0) & (nrm[:, 1] != 0.0)):
        raise ValueError("edgeCoverageTangent: Manhattan layouts only (an edge is neither horizontal nor vertical)")
    rows, cols, frag, wts = [], [], [], []
    x0, y0 = float(origin[0]), float(origin[1])
    for i in range(len(sites)):
        ends = sites.fragment_ends_nm[i] + nrm[i] * bias[i]
        horizontal = nrm[i, 0] == 0.0                               # the fragment runs along x, its normal along y
        along = 0 if horizontal else 1
        a, b = sorted(((ends[0, along] - (x0, y0)[along]) / ps, (ends[1, along] - (x0, y0)[along]) / ps))
        v = (ends[0, 1 - along] - (x0, y0)[1 - along]) / ps         # the line's position across, in pixels
        across = [(int(math.floor(v)), 1.0)] if v != math.floor(v) else [(int(v) - 1, 0.5), (int(v), 0.5)]
        for c in range(max(0, int(math.floor(a))), min(pn, int(math.ceil(b)))):
            overlap = min(b, c + 1.0) - max(a, float(c))
            if overlap <= 0.0:
                continue
            for r, half in across:
                if 0 <= r < pn:
                    rows.append(r if horizontal else c)
                    cols.append(c if horizontal else r)
                    frag.append(i)
                    wts.append(half * overlap / ps)
    return (np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(frag, dtype=np.int64),
            np.array(wts, dtype=np.float64))


def edgeCoverageTangentHost(sites, directions, pixelNumber, pixelSize, origin, bias_nm=None):
    """edgeCoverageTangent before the upload: float64 numpy [P,pn,pn], no GPU needed."""
    if not isinstance(sites, LayoutSites):
        raise TypeError("edgeCoverageTangent: sites must be a LayoutSites (layoutSites)")
    pn, ps, S = int(pixelNumber), float(pixelSize), len(sites)
    d = np.asarray(directions, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != S or d.shape[0] < 1:
        raise ValueError(f"edgeCoverageTangent: directions must be [P,{S}] (nanometres of bias per fragment); got {d.shape}")
    bias = np.zeros(S) if bias_nm is None else np.asarray(bias_nm, dtype=np.float64).reshape(-1)
    if bias.shape[0] != S or not np.isfinite(bias).all() or not np.isfinite(d).all():
        raise ValueError(f"edgeCoverageTangent: {S} finite biases and finite directions are needed")
    if origin is None:
        origin = _window_origin(sites.polygons, pn, ps)
    rows, cols, frag, wts = _fragment_cells(sites, bias, pn, ps, origin)
    out = np.zeros((d.shape[0], pn, pn), dtype=np.float64)
    for p in range(d.shape[0]):
        np.add.at(out[p], (rows, cols), d[p, frag] * wts)
    return out


def edgeCoverageTangent(sites, directions, pixelNumber, pixelSize, origin, bias_nm=None, device=None):
    """The first-order change of the EXACT-AREA coverage of a Manhattan layout when fragment i of `sites` (a LayoutSites) moves by
    directions[p, i] nanometres along its outward normal: fp32 [P,pn,pn] on the device, per pixel
    sum_i directions[p, i] * (length of fragment i, displaced by bias_nm[i], inside the pixel) / pixelSize^2.  The corner pieces
    that neighbouring fragments open between them are second order and left out.  Built on the host in float64
    (edgeCoverageTangentHost) and uploaded: a fragment touches spacing / pixelSize cells, so this is not a hot path.  `origin` as
    rasterizeLayout takes it (None: the window centred on the layout's bounding box); non-Manhattan sites raise ValueError, as in
    biasLayout.  For a phase-shift mask the caller multiplies by (feature - background)."""
    out = edgeCoverageTangentHost(sites, directions, pixelNumber, pixelSize, origin, bias_nm)
    dev = nat.require_gpu(nat.pick_device(device, "layout"))
    return torch.from_numpy(out.astype(np.float32)).to(dev)


def _tangent_images(who, image, dImage):
    """(image [planes,n,n], dImage [P,planes,n,n], planes, n, P) as the tangent kernels take them, contiguous fp32."""
    from .imageformation import ShapeError
    if not isinstance(image, torch.Tensor) or image.dim() not in (2, 3) or image.shape[-1] != image.shape[-2] \
            or image.dtype != torch.float32 or image.numel() == 0:
        raise ShapeError(f"{who}: image must be a float32 tensor [n,n] or [planes,n,n]; got "
                         f"{getattr(image, 'dtype', type(image))} {tuple(getattr(image, 'shape', ()))}")
    want = tuple(image.shape)
    if (not isinstance(dImage, torch.Tensor) or dImage.dtype != torch.float32 or dImage.dim() != image.dim() + 1
            or tuple(dImage.shape[1:]) != want or dImage.shape[0] < 1 or dImage.device != image.device):
        raise ShapeError(f"{who}: dImage must be a float32 tensor [P,{','.join(map(str, want))}] on {image.device}; got "
                         f"{getattr(dImage, 'dtype', type(dImage))} {tuple(getattr(dImage, 'shape', ()))}")
    planes = image.shape[0] if image.dim() == 3 else 1
    return image.contiguous(), dImage.contiguous(), planes, int(image.shape[-1]), int(dImage.shape[0])


def measureEPETangent(image, dImage, threshold, sites, pixelSize, doses=(1.0,), exposed=True, searchRange=8.0):
    """d(epe_nm) of measureEPE along image directions: fp32 [P, len(doses), planes, S] from `dImage` fp32 [P,n,n] (or
    [P,planes,n,n], matching `image`).  The kernel runs measureEPE's own search on `image`, so it picks the same interval k, and
    returns the exact derivative of t* = t_k + h (T - u_k) / (u_{k+1} - u_k) with du the gained bilinear samples of dImage at the same
    two points; NaN wherever measureEPE is NaN.  Arguments and checks as measureEPE; any P, in chunks of 16."""
    from .imageformation import ShapeError
    img, dimg, planes, n, P = _tangent_images("measureEPETangent", image, dImage)
    given = sites.sites_px if isinstance(sites, LayoutSites) else sites
    s = given if isinstance(given, torch.Tensor) else torch.as_tensor(np.asarray(given))
    if s.dim() != 2 or s.shape[1] != 4 or s.shape[0] < 1 or not s.is_floating_point():
        raise ShapeError(f"measureEPETangent: sites must be floating (x, y, nx, ny) rows [S,4], S >= 1; got {s.dtype} {tuple(s.shape)}")
    gains = [float(d) for d in doses]
    if not 1 <= len(gains) <= 64:
        raise ShapeError(f"measureEPETangent: between 1 and 64 doses per call; got {len(gains)}")
    if not (float(pixelSize) > 0.0 and math.isfinite(float(pixelSize))):
        raise ValueError(f"measureEPETangent: pixelSize must be finite and > 0; got {pixelSize}")
    if not 0.0 < float(searchRange) <= 32.0:
        raise ValueError(f"measureEPETangent: searchRange must lie in (0, 32] pixels; got {searchRange}")
    dev = nat.require_gpu(image.device)
    if isinstance(given, torch.Tensor) and given.device != image.device:
        raise ShapeError(f"measureEPETangent: sites live on {given.device}, the image on {image.device}")
    s = s.to(device=dev, dtype=torch.float32).contiguous()
    S = s.shape[0]
    out = torch.empty((P, len(gains), planes, S), dtype=torch.float32, device=dev)
    arr = (ctypes.c_float * len(gains))(*gains)
    with torch.cuda.device(dev):
        for p0 in range(0, P, MAX_DIRECTIONS):
            nb = min(MAX_DIRECTIONS, P - p0)
            nat.check(nat.lib().litho_measure_epe_jvp(nat.ptr(img), nat.ptr(dimg[p0]), nb, planes, n, nat.ptr(s), S, arr, len(gains),
                                                      float(threshold), 1 if exposed else 0, float(searchRange), float(pixelSize),
                                                      nat.ptr(out[p0]), nat.stream_ptr(dev)), "litho_measure_epe_jvp")
    return out


def measureCDTangent(image, dImage, gauges, threshold, pixelSize, doses=(1.0,), exposed=True):
    """(dcd_nm, dx_lo, dx_hi) of measureCD along image directions: fp32 [P, len(doses), planes, G, 3] from `dImage` fp32 [P,n,n] (or
    [P,planes,n,n]).  The run through the gauge is the primal's; each crossing moves by the exact derivative of its linear
    interpolant, a border edge (-0.5, n - 0.5) does not move.  Where the gauge's pixel is not inside: dcd_nm = 0 and NaN for the
    rest; three NaN for a gauge outside the grid -- measureCD's pattern.  Arguments and checks as measureCD (note exposed=True here:
    the polygons of this module are openings that print bright); any P, in chunks of 16."""
    from .imageformation import ShapeError
    img, dimg, planes, n, P = _tangent_images("measureCDTangent", image, dImage)
    g = gauges if isinstance(gauges, torch.Tensor) else torch.tensor(gauges, dtype=torch.int32)
    if g.dim() != 2 or g.shape[1] != 3 or g.shape[0] < 1 or g.is_floating_point() or g.is_complex() or g.dtype == torch.bool:
        raise ShapeError(f"measureCDTangent: gauges must be integer (row, col, axis) triples [G,3], G >= 1; got {g.dtype} "
                         f"{tuple(g.shape)}")
    gains = [float(d) for d in doses]
    if not 1 <= len(gains) <= 64:
        raise ShapeError(f"measureCDTangent: between 1 and 64 doses per call; got {len(gains)}")
    if not float(pixelSize) > 0.0:
        raise ValueError(f"measureCDTangent: pixelSize must be > 0; got {pixelSize}")
    dev = nat.require_gpu(image.device)
    if isinstance(gauges, torch.Tensor) and gauges.device != image.device:
        raise ShapeError(f"measureCDTangent: gauges live on {gauges.device}, the image on {image.device}")
    g = g.to(device=dev, dtype=torch.int32).contiguous()
    G = g.shape[0]
    out = torch.empty((P, len(gains), planes, G, 3), dtype=torch.float32, device=dev)
    arr = (ctypes.c_float * len(gains))(*gains)
    with torch.cuda.device(dev):
        for p0 in range(0, P, MAX_DIRECTIONS):
            nb = min(MAX_DIRECTIONS, P - p0)
            nat.check(nat.lib().litho_measure_cd_jvp(nat.ptr(img), nat.ptr(dimg[p0]), nb, planes, n, nat.ptr(g), G, arr, len(gains),
                                                     float(threshold), 1 if exposed else 0, float(pixelSize), nat.ptr(out[p0]),
                                                     nat.stream_ptr(dev)), "litho_measure_cd_jvp")
    return out


def _primal_and_tangents(polygons, sites, bias, directions, socs, pn, ps, origin, wavelength, antialias):
    """(image, a generator of (p0, dImage chunk)) of the chain raster -> spectrum -> Hopkins -> post-process at the biased layout."""
    from .imageformation import postProcess
    from .layout import rasterizeLayout
    from .mask import Mask
    dev = socs.kernels.device
    eps, N = nat.epsilon_n(4.0 / pn, ps, float(wavelength))
    raster = rasterizeLayout(biasLayout(polygons, sites, bias), pn, ps, origin, dev, antialias=antialias)
    mft = Mask(pixelSize=ps, device=dev, transmission=raster)._ffFraunhofer(eps, N)
    image = postProcess(_socs.hopkinsIntensity(mft, socs, N), eps)

    def chunks():
        for p0 in range(0, directions.shape[0], MAX_DIRECTIONS):
            dt = edgeCoverageTangent(sites, directions[p0:p0 + MAX_DIRECTIONS], pn, ps, origin, bias_nm=bias, device=dev)
            dM = torch.stack([Mask(pixelSize=ps, device=dev, transmission=t)._ffFraunhofer(eps, N) for t in dt])
            yield p0, postProcessTangent(hopkinsTangent(mft, socs, N, dM), pn, eps)

    return image, chunks()


def _check_window(who, socs, pixelNumber):
    if not isinstance(socs, _socs.SOCSKernels):
        raise TypeError(f"{who}: socs must be a SOCSKernels (socsKernels / vectorSocsKernels)")
    if socs.pn != int(pixelNumber) or socs.stacked:
        raise ValueError(f"{who}: the kernels are {'a stack of ' if socs.stacked else ''}{socs.pn} x {socs.pn}, the window "
                         f"{int(pixelNumber)} x {int(pixelNumber)}: one plane on the window's grid is needed")


def epeJacobian(polygons, sites, bias_nm, socs, pixelNumber, pixelSize, origin, wavelength, threshold, *, antialias=16,
                searchRange=8.0, directions=None):
    """(epe_nm [S], J [S,P]) at the layout biasLayout(polygons, sites, bias_nm): the EPE at the target's sites (plane 0, dose 1, NaN
    where nothing crosses in range) and its derivative along `directions` [P,S] of the fragment biases, in nm per nm; float64 on the
    host.  directions=None is the identity: J[i, j] = d EPE_i / d bias_j, the MEEF matrix.  The primal is the chain of
    correctLayout(model="socs"): raster of the biased layout -> spectrum -> hopkinsIntensity -> postProcess -> measureEPE; then
    the columns, 16 per pass: edgeCoverageTangent -> spectrum -> hopkinsTangent -> postProcessTangent -> measureEPETangent -- one
    forward pass per fragment, every site at once.  A row of J is NaN where the site's EPE is."""
    _check_window("epeJacobian", socs, pixelNumber)
    pn, ps = int(pixelNumber), float(pixelSize)
    target = _counter_clockwise(polygons)
    if origin is None:
        origin = _window_origin(target, pn, ps)
    S = len(sites)
    bias = np.asarray(bias_nm, dtype=np.float64).reshape(-1)
    d = np.eye(S) if directions is None else np.asarray(directions, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != S or d.shape[0] < 1:
        raise ValueError(f"epeJacobian: directions must be [P,{S}]; got {d.shape}")
    image, chunks = _primal_and_tangents(target, sites, bias, d, socs, pn, ps, origin, wavelength, antialias)
    rows = torch.from_numpy(sites.sites_px).to(image.device)
    epe = measureEPE(image, threshold, rows, ps, searchRange=searchRange)[0, 0, :, 0].double().cpu().numpy()
    J = np.empty((S, d.shape[0]))
    for p0, dimage in chunks:
        dE = measureEPETangent(image, dimage, threshold, rows, ps, searchRange=searchRange)[:, 0, 0, :]
        J[:, p0:p0 + dE.shape[0]] = dE.double().cpu().numpy().T
    return epe, J


def maskErrorFactor(polygons, gauges, socs, pixelNumber, pixelSize, origin, wavelength, threshold, *, antialias=16, doses=(1.0,),
                    exposed=True):
    """(cd_nm, meef), each fp32 [len(doses), G] on the device: the printed CD at the (row, col, axis) gauges and the mask-error
    factor dCD_printed / dCD_mask there.  One direction, every edge of the layout biased outward by 1 nm: the mask CD grows by
    2 nm, so meef = dcd_nm / 2 (dimensions on the wafer scale, as everywhere in this package).  The chain of epeJacobian with
    measureCD / measureCDTangent at its end; meef is 0 where the gauge's pixel does not print and NaN outside the grid, as
    measureCD's cd_nm is."""
    from .imageformation import measureCD
    _check_window("maskErrorFactor", socs, pixelNumber)
    pn, ps = int(pixelNumber), float(pixelSize)
    target = _counter_clockwise(polygons)
    if origin is None:
        origin = _window_origin(target, pn, ps)
    sites = layoutSites(target, pn * ps, ps, origin, pn, wavelength)          # one fragment per edge (no edge outgrows the window)
    if len(sites) == 0:
        raise ValueError("maskErrorFactor: the layout has no edges")
    image, chunks = _primal_and_tangents(target, sites, np.zeros(len(sites)), np.ones((1, len(sites))), socs, pn, ps, origin,
                                         wavelength, antialias)
    g = gauges if isinstance(gauges, torch.Tensor) else torch.tensor(gauges, dtype=torch.int32)
    g = g.to(image.device)
    cd = measureCD(image, threshold, g, ps, doses=doses, exposed=exposed)[:, 0, :, 0]
    (_, dimage), = chunks
    dcd = measureCDTangent(image, dimage, g, threshold, ps, doses=doses, exposed=exposed)[0, :, 0, :, 0]
    return cd, dcd / 2.0
