"""Edge placement error (EPE) on layout edges and a model-based correction loop (OPC); no reference counterpart.

The chain GDSII -> area-coverage mask -> Abbe image -> (diffused) resist image ends in a contour; layout verification and
correction ask how far that contour lies from the edge the layout drew, measured along the edge's normal.  Host side (this
file, numpy): where the image grid lies against the mask raster (`imageRegistration`), measurement sites on polygon edges
(`layoutSites`), moving edge fragments (`biasLayout`) and the feedback loop (`correctLayout`).  Device side
(csrc/metrology.hip through the C ABI): `measureEPE`, one wave per site and plane.

Coordinates: layouts in nanometres as in layout.py (x = columns, y = rows, no flip); sites on the IMAGE grid in pixels, sample
(row r, column c) at (x = c, y = r) -- the convention of measureCD's x_lo.
"""
import ctypes
import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat


def _registration(pixelNumber, pixelSize, wavelength):
    """(n_out, scale, offset): mask-raster pixel i is shown at image pixel J = scale * i + offset.  The mask raster is resampled
    by epsilon and padded by pW_mask into the N grid (mask.py:76-81), the field is cropped at pW_crop
    (imageformation.py:36-43), and the image is resampled by 1 / epsilon and padded (or, negative, cropped) by pW_out
    (imageformation.py:71-75).  A resampling by s shows source centre q at (q + 0.5) s - 0.5 -- except that torch copies when
    the output size floor(n s) equals the input size, whatever s says."""
    pn, ps, wl = int(pixelNumber), float(pixelSize), float(wavelength)
    if pn < 2 or not (ps > 0.0 and math.isfinite(ps)) or not (wl > 0.0 and math.isfinite(wl)):
        raise ValueError(f"pixelNumber >= 2, pixelSize and wavelength finite and > 0; got {pixelNumber}, {pixelSize}, {wavelength}")
    eps, N = _epsilon_n(4.0 / pn, ps, wl)
    ns = int(math.floor(pn * eps))
    pW_mask = ((N - pn) - (ns - pn)) // 2
    pW_crop = (N - pn) // 2
    pW_out = (pn - round(pn / eps)) // 2
    n_back = int(math.floor(pn * (1.0 / eps)))                  # size after the image's resampling; n_out as litho_postprocess_size
    n_out = n_back + 2 * pW_out + n_back % 2
    if N < pn or n_out < 1:
        raise ValueError(f"pixelSize {pixelSize} is too large for wavelength {wavelength}: the FFT grid {N} is smaller than the mask")
    scale, offset = (1.0, 0.0) if ns == pn else (eps, 0.5 * eps - 0.5)
    offset += pW_mask - pW_crop
    if n_back != pn:
        scale, offset = scale / eps, (offset + 0.5) / eps - 0.5
    return n_out, scale, offset + pW_out


_TWO_POWERS = tuple(2 ** k for k in range(1, 15))


def _epsilon_n(deltaK, pixelSize, wavelength):
    """mask.py:63-72 on the host (what litho_epsilon_n computes): beta = wavelength / (deltaK pixelSize), N = the power of two
    nearest beta (the first minimum wins; the distance in fp32, as the reference's int16-tensor arithmetic has it),
    epsilon = N / beta.  Host NumPy, so that sites can be laid out without the compiled library."""
    beta = ((deltaK * pixelSize) / wavelength) ** -1
    sq = np.asarray(_TWO_POWERS, dtype=np.float32)
    N = int(_TWO_POWERS[int(np.argmin(np.abs(sq - np.float32(beta))))])
    return N / beta, N


def imageRegistration(pixelNumber: int, pixelSize: float, wavelength: float) -> Tuple[int, float]:
    """(n_out, offset_px): the post-processed image is n_out x n_out, and its pixel J shows mask-raster pixel
    i = J - offset_px, the same on both axes.  The reference's resample-and-pad chain (mask.py:76-81, imageformation.py:36-43
    and 71-75) maps centres by src = (dst + 0.5) / scale - 0.5 twice, with epsilon and with 1 / epsilon, so the half pixels
    cancel and  offset = pW_out - (pW_crop - pW_mask) / epsilon  -- a fraction of a pixel that depends on size and wavelength
    (0.07 px = 1.75 nm at 128^2, 25 nm, 193 nm).  Where one of the two resamplings degenerates to a copy (equal sizes: 128^2
    at 48 nm) the other's scale is left over, J = scale * i + offset with scale within a percent of 1; offset_px is then
    the shift at the window's centre, and layoutSites applies the whole map."""
    n_out, scale, offset = _registration(pixelNumber, pixelSize, wavelength)
    centre = (int(pixelNumber) - 1) / 2.0
    return n_out, (scale - 1.0) * centre + offset


@dataclass
class LayoutSites:
    """EPE sites of a layout: one per edge fragment, at its midpoint, with the unit normal pointing out of the polygon."""
    xy_nm: np.ndarray               # float64 [S,2]
    normal: np.ndarray              # float64 [S,2], unit, outward
    polygon: np.ndarray             # int64 [S]: index into the polygon list
    edge: np.ndarray                # int64 [S]: edge of that polygon (vertex j -> j + 1 of the counter-clockwise polygon)
    fragment_ends_nm: np.ndarray    # float64 [S,2,2]: (start, end) of the fragment, in the polygon's direction
    sites_px: np.ndarray            # float32 [S,4] = (x, y, nx, ny) on the image grid: what measureEPE takes
    polygons: List[np.ndarray] = field(default_factory=list)      # the polygons as used: float64, counter-clockwise

    def __len__(self):
        return int(self.xy_nm.shape[0])


def _counter_clockwise(polygons) -> List[np.ndarray]:
    """Each polygon as float64 [k,2], counter-clockwise (the orientation polygonEdges gives them), in the caller's order."""
    out = []
    for q in polygons:
        q = np.asarray(q, dtype=np.float64).reshape(-1, 2)
        if len(q) >= 3:
            area2 = float(np.sum(q[:, 0] * np.roll(q[:, 1], -1) - np.roll(q[:, 0], -1) * q[:, 1]))
            if area2 < 0:
                q = q[::-1]
        out.append(np.ascontiguousarray(q))
    return out


def _window_origin(polygons, pn, pixelSize):
    """rasterizeLayout's origin=None: the window centred on the polygons' bounding box."""
    pts = [q for q in polygons if len(q) >= 3]
    if pts:
        lo = np.min([q.min(axis=0) for q in pts], axis=0)
        hi = np.max([q.max(axis=0) for q in pts], axis=0)
        ctr = (lo + hi) / 2.0
    else:
        ctr = np.zeros(2)
    return (float(ctr[0]) - pn * pixelSize / 2.0, float(ctr[1]) - pn * pixelSize / 2.0)


def layoutSites(polygons: Sequence[np.ndarray], spacing: float, pixelSize: float, origin, pixelNumber: int,
                wavelength: float, registration=None) -> LayoutSites:
    """Measurement sites on every edge of every polygon (nanometres, any angle; made counter-clockwise as polygonEdges does):
    an edge of length L is cut into ceil(L / spacing) equal fragments, each with one site at its midpoint and the unit
    outward normal (dy, -dx) / L.  `sites_px` places them on the image grid: `origin` exactly as rasterizeLayout takes it
    (None: the window centred on the bounding box), then the registration of imageRegistration.
    `registration` = (n_out, scale, offset) replaces the single window's own map J = scale * i + offset from raster pixel i to
    image pixel J: what a stitched image of several windows carries (tiling.py); None is the window's, as before."""
    spacing, ps, pn = float(spacing), float(pixelSize), int(pixelNumber)
    if not (spacing > 0.0 and math.isfinite(spacing)) or not (ps > 0.0 and math.isfinite(ps)):
        raise ValueError(f"layoutSites: spacing and pixelSize must be finite and > 0; got {spacing} and {ps}")
    polys = _counter_clockwise(polygons)
    if origin is None:
        origin = _window_origin(polys, pn, ps)
    if registration is None:
        _, scale, offset = _registration(pn, ps, wavelength)
    else:
        _, scale, offset = registration
        scale, offset = float(scale), float(offset)
    xy, nrm, pidx, eidx, ends = [], [], [], [], []
    for pi, q in enumerate(polys):
        if len(q) < 3:
            continue
        for ei in range(len(q)):
            a, b = q[ei], q[(ei + 1) % len(q)]
            d = b - a
            length = float(math.hypot(d[0], d[1]))
            if not length > 0.0:
                continue
            m = max(1, int(math.ceil(length / spacing)))
            normal = np.array([d[1], -d[0]]) / length
            for f in range(m):
                p0, p1 = a + d * (f / m), a + d * ((f + 1) / m)
                if f == m - 1:
                    p1 = b.copy()
                xy.append((p0 + p1) / 2.0)
                nrm.append(normal)
                pidx.append(pi)
                eidx.append(ei)
                ends.append((p0, p1))
    S = len(xy)
    xy = np.array(xy, dtype=np.float64).reshape(S, 2)
    nrm = np.array(nrm, dtype=np.float64).reshape(S, 2)
    px = np.empty((S, 4), dtype=np.float32)
    px[:, 0] = ((xy[:, 0] - float(origin[0])) / ps - 0.5) * scale + offset
    px[:, 1] = ((xy[:, 1] - float(origin[1])) / ps - 0.5) * scale + offset
    px[:, 2:] = nrm
    return LayoutSites(xy, nrm, np.array(pidx, dtype=np.int64), np.array(eidx, dtype=np.int64),
                       np.array(ends, dtype=np.float64).reshape(S, 2, 2), px, polys)


def measureEPE(image, threshold, sites, pixelSize, doses=(1.0,), exposed=True, searchRange=8.0):
    """Edge placement error at sites on the image grid -- the aerial image (postProcess) or the diffused one
    (resistContour(..., return_image=True, diffusionLength=...)).  `image` fp32 [n,n] or [planes,n,n] on the GPU; `sites` a
    LayoutSites, or a float tensor / array [S,4] = (x, y, nx, ny) in image pixels with (nx, ny) pointing out of the feature;
    `doses` at most 64 gains; `searchRange` in pixels along the normal, (0, 32].  Returns fp32 [len(doses), planes, S, 3] =
    (epe_nm, ils_per_nm, t_k): the bilinear image is sampled every half pixel along the normal, the crossing nearest the
    site where the samples LEAVE the feature going outward ((dose * image >= threshold) == exposed inside) is interpolated
    linearly; epe_nm > 0 when the printed feature reaches beyond the target edge, ils the image log-slope per nm there,
    t_k the inner end of the crossing's interval.  Three NaN where nothing crosses in range (include/litho_abbe.h)."""
    import torch

    from .imageformation import ShapeError
    if not isinstance(image, torch.Tensor) or image.dim() not in (2, 3) or image.shape[-1] != image.shape[-2] \
            or image.dtype != torch.float32 or image.numel() == 0:
        raise ShapeError(f"measureEPE: image must be a float32 tensor [n,n] or [planes,n,n]; got "
                         f"{getattr(image, 'dtype', type(image))} {tuple(getattr(image, 'shape', ()))}")
    given = sites.sites_px if isinstance(sites, LayoutSites) else sites
    s = given if isinstance(given, torch.Tensor) else torch.as_tensor(np.asarray(given))
    if s.dim() != 2 or s.shape[1] != 4 or s.shape[0] < 1 or not s.is_floating_point():
        raise ShapeError(f"measureEPE: sites must be floating (x, y, nx, ny) rows [S,4], S >= 1; got {s.dtype} {tuple(s.shape)}")
    gains = [float(d) for d in doses]
    if not 1 <= len(gains) <= 64:
        raise ShapeError(f"measureEPE: between 1 and 64 doses per call; got {len(gains)}")
    if not (float(pixelSize) > 0.0 and math.isfinite(float(pixelSize))):
        raise ValueError(f"measureEPE: pixelSize must be finite and > 0; got {pixelSize}")
    if not 0.0 < float(searchRange) <= 32.0:
        raise ValueError(f"measureEPE: searchRange must lie in (0, 32] pixels; got {searchRange}")
    dev = nat.require_gpu(image.device)
    if isinstance(given, torch.Tensor) and given.device != image.device:
        raise ShapeError(f"measureEPE: sites live on {given.device}, the image on {image.device}")
    img = image.contiguous()
    planes = img.shape[0] if img.dim() == 3 else 1
    n = img.shape[-1]
    s = s.to(device=dev, dtype=torch.float32).contiguous()
    S = s.shape[0]
    out = torch.empty((len(gains), planes, S, 3), dtype=torch.float32, device=dev)
    arr = (ctypes.c_float * len(gains))(*gains)
    with torch.cuda.device(dev):
        nat.check(nat.lib().litho_measure_epe(nat.ptr(img), planes, n, nat.ptr(s), S, arr, len(gains), float(threshold),
                                              1 if exposed else 0, float(searchRange), float(pixelSize), nat.ptr(out),
                                              nat.stream_ptr(dev)), "litho_measure_epe")
    return out


def biasLayout(polygons: Sequence[np.ndarray], sites: LayoutSites, bias_nm) -> List[np.ndarray]:
    """The layout with every edge fragment of `sites` (layoutSites of the same polygons) displaced by its bias along its
    outward normal -- the host side of the correction loop.  Manhattan polygons only: an edge that is neither horizontal
    nor vertical raises ValueError.  Neighbouring fragments of one edge (or of two collinear edges) are joined by a jog at
    their common end point (two vertices), fragments meeting at a corner at the intersection of their displaced lines.
    Equal biases on one line add no vertex, so zero bias returns the target's own outline and its raster bit for bit."""
    polys = _counter_clockwise(polygons)
    bias = np.asarray(bias_nm, dtype=np.float64).reshape(-1)
    if bias.shape[0] != len(sites):
        raise ValueError(f"biasLayout: {bias.shape[0]} biases for {len(sites)} sites")
    if not np.isfinite(bias).all():
        raise ValueError("biasLayout: a bias is not finite")
    if len(sites) and int(sites.polygon.max()) >= len(polys):
        raise ValueError("biasLayout: the sites belong to another layout (polygon index out of range)")
    nrm = sites.normal
    if np.any((nrm[:, 0] != 0.0) & (nrm[:, 1] != 0.0)):
        raise ValueError("biasLayout: Manhattan layouts only (an edge is neither horizontal nor vertical)")
    out = []
    for pi, q in enumerate(polys):
        idx = np.nonzero(sites.polygon == pi)[0]                # in order around the polygon: edge by edge, fragment by fragment
        if idx.size == 0:
            out.append(q.copy())
            continue
        pts = []
        for a, i in enumerate(idx):
            j = idx[(a + 1) % idx.size]
            corner = sites.fragment_ends_nm[i, 1]
            if not np.array_equal(corner, sites.fragment_ends_nm[j, 0]):
                raise ValueError("biasLayout: the sites do not trace the polygon (fragment ends do not meet)")
            di, dj = nrm[i] * bias[i], nrm[j] * bias[j]
            if nrm[i, 0] * nrm[j, 1] - nrm[i, 1] * nrm[j, 0] == 0.0:     # the same line: a jog, or nothing between equal biases
                if not np.array_equal(di, dj):
                    pts += [corner + di, corner + dj]
            else:                                                        # perpendicular lines: their intersection
                pts.append(corner + di + dj)
        keep = [p for k, p in enumerate(pts) if not np.array_equal(p, pts[k - 1])]
        out.append(np.array(keep if len(keep) >= 3 else pts, dtype=np.float64))
    return out


@dataclass
class OPCResult:
    """What correctLayout returns.  `history`: per iteration (rms_nm, max_abs_nm, nan_sites) of the EPE measured on that
    iteration's layout; `polygons` / `bias_nm`: the iterate `best_iteration` names -- the fewest NaN sites, then the lowest
    RMS EPE; `sites`: the target's sites, fixed through the loop; `epe_nm`: the EPE per site of that iterate, `epe_history`
    that of every iteration."""
    polygons: List[np.ndarray]
    bias_nm: np.ndarray
    history: List[Tuple[float, float, int]]
    sites: LayoutSites
    best_iteration: int = 0
    epe_nm: Optional[np.ndarray] = None
    epe_history: List[np.ndarray] = field(default_factory=list)
    jacobian: Optional[np.ndarray] = None   # step="meef": the frozen MEEF matrix J[i, j] = dEPE_i / dbias_j of the first iterate


def correctLayout(polygons, pixelNumber, pixelSize, origin, wavelength, pupil, source, threshold, *, spacing, iterations=6,
                  gain=0.6, maxBias, antialias=16, exposed=True, diffusionLength=0.0, searchRange=8.0,
                  imager: Optional[Callable] = None, epe: Optional[Callable] = None, device=None, model="abbe",
                  kernels=64, socs=None, step="damped", sensitivity: Optional[Callable] = None) -> OPCResult:
    """Model-based optical proximity correction of a Manhattan layout (nanometres; the polygons are the mask's openings):
    edge fragments of at most `spacing` are moved along their normals until the printed contour lies on the target's edges.
    Every iteration: biasLayout -> rasterizeLayout(antialias=) -> Mask(transmission=) -> fraunhofer -> abbeIntensity through
    one PlanCache (from the second iteration on no source compaction and no host wait inside the image) -> postProcess, or
    the diffused image of resistContour when diffusionLength > 0 -> measureEPE at the target's sites, which stay fixed
    (plane 0, dose 1) -> bias <- clip(bias - gain * EPE, +-maxBias).  A site with NaN EPE (nothing printed in range) gets
    bias += maxBias / 6 (the opening grows), then the clip.  Exposed features only: exposed=False raises ValueError (neither the
    mask tone nor that step is defined for it yet).  `threshold` is absolute, on the returned image's scale (raw
    sums over the source points); `pupil` the pupil function [pn,pn], `source` the source bitmap [pn,pn] or a (dy,dx) list.

    `model="socs"`: the optical setting is factored once into `kernels` SOCS kernels (socsKernels: Hopkins imaging, an
    approximation unless `kernels` reaches the number of lit source points) and every iteration's image is those K fields
    (hopkinsIntensity) instead of one field per source point.  The default "abbe" is the path described above, call for call.
    `socs`: a SOCSKernels (socsKernels, or vectorSocsKernels for polarised high-NA imaging) used instead of factoring `pupil`
    and `source`; with model="socs" only, one plane, and its pn must be the window's (ValueError otherwise).

    `imager(polygons) -> image` replaces the raster-to-image steps and `epe(image) -> EPE in nm per site` (NaN where nothing
    is found) the measurement, so the loop itself runs without a GPU on any model; give both or neither.

    `step="damped"` (the default) is the update above, whose model of the process is the identity: every fragment moves its own
    edge one for one and nobody else's.  `step="meef"` replaces that model by the MEEF matrix J[i, j] = dEPE_i / dbias_j, computed
    once at the first iterate and kept (a frozen Jacobian: one Jacobian, then one image per iteration).  It needs model="socs"
    (ValueError otherwise): mask tangents go through the SOCS kernels (sensitivity.epeJacobian, forward mode, one pass per
    fragment).  On the sites that found an edge the step solves (J^T J + mu diag J^T J) delta = -J^T e in float64 on the host,
    with the accept / reject rule of calibrate._levenberg_marquardt -- an iterate that is not better (fewer lost sites, then lower
    RMS) than the best so far is not accepted, the next step starts from the best again and mu grows tenfold, an accepted one
    divides mu by ten -- then the +-maxBias clip.  mu starts at that rule's floor, 1e-12 (on a frozen Jacobian of a nearly linear
    map the undamped step is the right first try), and a rejection raises it to at least 1e-3, the rule's own start.  Sites that
    found no edge keep the +maxBias / 6 rule.  `sensitivity(polygons, bias) -> J [S,S]` replaces epeJacobian when imager= and epe=
    are given; the loop then runs on the CPU on any model.  `gain` is not used by this step; OPCResult.jacobian holds J."""
    if step not in ("damped", "meef"):
        raise ValueError(f"correctLayout: step must be 'damped' or 'meef'; got {step!r}")
    if step == "meef" and imager is None and model != "socs":
        raise ValueError("correctLayout: step='meef' needs model='socs' (mask tangents go through the SOCS kernels), or imager=, "
                         "epe= and sensitivity= of the caller's own model")
    if step == "meef" and imager is not None and sensitivity is None:
        raise ValueError("correctLayout: step='meef' with imager= and epe= needs sensitivity(polygons, bias) -> J as well")
    if sensitivity is not None and (step != "meef" or imager is None):
        raise ValueError("correctLayout: sensitivity= goes with step='meef' and the imager= / epe= pair")
    if (imager is None) != (epe is None):
        raise ValueError("correctLayout: imager and epe replace the image and its measurement together; give both or neither")
    if model not in ("abbe", "socs"):
        raise ValueError(f"correctLayout: model must be 'abbe' or 'socs'; got {model!r}")
    if socs is not None:
        from .socs import SOCSKernels
        if not isinstance(socs, SOCSKernels):
            raise TypeError("correctLayout: socs must be a SOCSKernels (socsKernels / vectorSocsKernels)")
        if model != "socs":
            raise ValueError("correctLayout: socs= goes with model='socs'")
        if socs.pn != int(pixelNumber) or socs.stacked:
            raise ValueError(f"correctLayout: the kernels are {'a stack of ' if socs.stacked else ''}{socs.pn} x {socs.pn}, the "
                             f"window {int(pixelNumber)} x {int(pixelNumber)}: one plane on the window's grid is needed")
    if not exposed:
        raise ValueError("correctLayout: the loop is defined for exposed features (the polygons are the mask's openings and print "
                         "bright); for exposed=False neither the mask tone nor the step of a site that finds no edge is defined yet")
    iterations, gain, maxBias = int(iterations), float(gain), float(maxBias)
    if iterations < 1 or not maxBias >= 0.0 or not math.isfinite(maxBias) or not math.isfinite(gain):
        raise ValueError(f"correctLayout: iterations >= 1, finite gain and maxBias >= 0; got {iterations}, {gain}, {maxBias}")
    pn, ps = int(pixelNumber), float(pixelSize)
    target = _counter_clockwise(polygons)
    if origin is None:
        origin = _window_origin(target, pn, ps)
    sites = layoutSites(target, spacing, ps, origin, pn, wavelength)
    if len(sites) == 0:
        raise ValueError("correctLayout: the layout has no edges")
    biasLayout(target, sites, np.zeros(len(sites)))            # raises for a non-Manhattan layout before any image is made
    if imager is None:
        state = {}
        imager, epe = _gpu_model(pn, ps, origin, wavelength, pupil, source, threshold, antialias, exposed, diffusionLength,
                                 searchRange, sites, device, model, kernels, socs, state)
        if step == "meef":
            if float(diffusionLength) > 0.0:
                raise ValueError("correctLayout: step='meef' differentiates the aerial image; diffusionLength > 0 is not built")

            def sensitivity(polys, b):
                from .sensitivity import epeJacobian
                return epeJacobian(target, sites, b, state["socs"], pn, ps, origin, wavelength, threshold, antialias=antialias,
                                   searchRange=searchRange)[1]
    if step == "meef":
        return _meef_loop(target, sites, imager, epe, sensitivity, iterations, maxBias)
    return _damped_loop(target, sites, imager, epe, iterations, gain, maxBias)


def _damped_loop(target, sites, imager, epe, iterations, gain, maxBias):
    """correctLayout(step="damped"): bias <- clip(bias - gain * EPE, +-maxBias), +maxBias / 6 where a site found no edge."""
    bias = np.zeros(len(sites))
    history, measured, best = [], [], None
    for it in range(iterations):
        polys = biasLayout(target, sites, bias)
        e = np.asarray(epe(imager(polys)), dtype=np.float64).reshape(-1)
        if e.shape[0] != len(sites):
            raise ValueError(f"correctLayout: epe returned {e.shape[0]} values for {len(sites)} sites")
        measured.append(e.copy())
        lost = np.isnan(e)
        found = e[~lost]
        rms = float(np.sqrt(np.mean(found * found))) if found.size else float("inf")
        worst = float(np.abs(found).max()) if found.size else float("inf")
        history.append((rms, worst, int(lost.sum())))
        if best is None or (int(lost.sum()), rms) < (history[best[0]][2], history[best[0]][0]):
            best = (it, polys, bias.copy(), e.copy())
        bias = np.clip(np.where(lost, bias + maxBias / 6.0, bias - gain * np.where(lost, 0.0, e)), -maxBias, maxBias)
    return OPCResult(best[1], best[2], history, sites, best[0], best[3], measured)


def _meef_loop(target, sites, imager, epe, sensitivity, iterations, maxBias):
    """correctLayout(step="meef"): Levenberg-Marquardt steps on a Jacobian frozen at the first iterate."""
    S = len(sites)
    bias = np.zeros(S)
    history, measured, best, J, mu = [], [], None, None, 1e-12
    for it in range(iterations):
        polys = biasLayout(target, sites, bias)
        e = np.asarray(epe(imager(polys)), dtype=np.float64).reshape(-1)
        if e.shape[0] != S:
            raise ValueError(f"correctLayout: epe returned {e.shape[0]} values for {S} sites")
        measured.append(e.copy())
        lost = np.isnan(e)
        found = e[~lost]
        rms = float(np.sqrt(np.mean(found * found))) if found.size else float("inf")
        worst = float(np.abs(found).max()) if found.size else float("inf")
        history.append((rms, worst, int(lost.sum())))
        if J is None:
            J = np.asarray(sensitivity(polys, bias.copy()), dtype=np.float64)
            if J.shape != (S, S):
                raise ValueError(f"correctLayout: sensitivity returned {J.shape} for {S} sites")
        accepted = best is None or (int(lost.sum()), rms) < (history[best[0]][2], history[best[0]][0])
        if accepted:
            best = (it, polys, bias.copy(), e.copy())
            if it:
                mu = max(mu / 10.0, 1e-12)
        else:
            mu = max(mu * 10.0, 1e-3)
        b0, e0 = best[2], best[3]                                   # every step starts from the best iterate
        gone = np.isnan(e0)
        Jf = np.where(np.isfinite(J[~gone]), J[~gone], 0.0)         # a row of a site that lost its edge in the Jacobian's image
        A, g = Jf.T @ Jf, Jf.T @ e0[~gone]
        diag = np.diag(A)
        move = (diag > 0.0) & ~gone                                 # a fragment without a column, or without an edge, does not move
        delta = np.zeros(S)
        if move.any():
            delta[move] = np.linalg.solve((A + mu * np.diag(diag))[np.ix_(move, move)], -g[move])
        bias = np.clip(np.where(gone, b0 + maxBias / 6.0, b0 + delta), -maxBias, maxBias)
    return OPCResult(best[1], best[2], history, sites, best[0], best[3], measured, J)


def _gpu_model(pn, ps, origin, wavelength, pupil, source, threshold, antialias, exposed, diffusionLength, searchRange, sites,
               device, model="abbe", kernels=64, socs=None, state=None):
    """(imager, epe) of correctLayout on the HIP path; `state` (a dict) receives the SOCS kernels under "socs"."""
    import torch

    from .imageformation import PlanCache, ShapeError, abbeIntensity, postProcess, resistContour
    from .layout import rasterizeLayout
    from .lightsource import sourceShiftsAsync
    from .mask import Mask
    if not isinstance(pupil, torch.Tensor) or tuple(pupil.shape) != (pn, pn):
        raise ShapeError(f"correctLayout: pupil must be the pupil function [{pn},{pn}]; got {tuple(getattr(pupil, 'shape', ()))}")
    if not isinstance(source, torch.Tensor) or source.dim() != 2 or (tuple(source.shape) != (pn, pn) and source.shape[1] != 2):
        raise ShapeError(f"correctLayout: source must be a bitmap [{pn},{pn}] or a (dy,dx) list [S,2]; got "
                         f"{tuple(getattr(source, 'shape', ()))}")
    dev = nat.require_gpu(device if device is not None else pupil.device)
    eps, N = nat.epsilon_n(4.0 / pn, ps, float(wavelength))
    pupil = pupil.to(device=dev, dtype=torch.complex64).contiguous()
    cache = PlanCache()
    state = {} if state is None else state
    site_rows = torch.from_numpy(sites.sites_px).to(dev)
    if model == "socs" and socs is not None:
        from .socs import hopkinsIntensity
        state["socs"] = socs
    elif model == "socs":
        from .socs import hopkinsIntensity, socsKernels
        if tuple(source.shape) == (pn, pn):
            bitmap = source.to(dev)
        else:                                                   # a (dy,dx) list: its bitmap, a repeated point counted as often
            rc = source.to(device=dev, dtype=torch.int64) + pn // 2
            if rc.numel() and (int(rc.min()) < 0 or int(rc.max()) > pn - 1):
                raise ShapeError(f"correctLayout: a source shift lies outside the {pn} x {pn} source grid")
            bitmap = torch.zeros((pn, pn), dtype=torch.float32, device=dev)
            bitmap.index_put_((rc[:, 0], rc[:, 1]), torch.ones(rc.shape[0], dtype=torch.float32, device=dev), accumulate=True)
        state["socs"] = socsKernels(pupil, bitmap, kernels=kernels)

    def imager(polys):
        raster = rasterizeLayout(polys, pn, ps, origin, dev, antialias=antialias)
        mask = Mask(pixelSize=ps, device=dev, transmission=raster) if raster.is_floating_point() else Mask(raster, ps, dev)
        mft = mask.fraunhofer(wavelength, True)
        if model == "socs":
            raw = hopkinsIntensity(mft, state["socs"], N)
        elif "shifts" not in state:
            if tuple(source.shape) == (pn, pn):
                shifts, count = sourceShiftsAsync(source.to(dev), pn)
            else:
                shifts, count = source.to(device=dev, dtype=torch.int32).contiguous(), None
            raw, total = abbeIntensity(mft, pupil, shifts, N, count=count, plan=cache)
            state["shifts"], state["S"] = shifts, total
        else:
            raw, _ = abbeIntensity(mft, pupil, state["shifts"][:state["S"]], N, plan=cache)
        if float(diffusionLength) > 0.0:
            return resistContour(raw, eps, threshold, return_image=True, diffusionLength=diffusionLength, pixelSize=ps)[0]
        return postProcess(raw, eps)

    def epe(image):
        return measureEPE(image, threshold, site_rows, ps, exposed=exposed, searchRange=searchRange)[0, 0, :, 0].cpu().numpy()

    return imager, epe
