"""Printed contours as polygons: what a resist or aerial image prints, as closed loops with sub-pixel vertices; no reference
counterpart.

The chain GDSII -> area-coverage mask -> Abbe image -> (diffused) resist image ended in a thresholded bitmap and in distances
at pre-placed sites.  Here it ends in geometry: GDSII in, GDSII out.  Device side (csrc/contour.hip through the C ABI, the
definition in include/litho_abbe.h): a marching-squares tracer that emits only the contour vertices, numbered and linked
(`contourVertices`), and the dose-focus envelope of an image stack.  Host side (this file, numpy): the cycles of the link
permutation as polygons (`traceContours`), image pixels -> layout nanometres (`contoursToLayout`), Douglas-Peucker
simplification (`simplifyContour`), the GDSII writer (`contoursToGDSII`) and process-variation bands
(`processVariationBand`).

Coordinates: image pixels, sample (row r, column c) at (x = c, y = r), as measureEPE and measureCD.  Walking a polygon the
feature lies on the left: outer boundaries have positive shoelace area, holes negative.
"""
import ctypes
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _native as nat

GDS_MAX_VERTICES = 8190          # distinct vertices of one BOUNDARY (the stream repeats the first: 8191 XY pairs)


@dataclass
class Contours:
    """The printed outline of one image.  `polygons`: float64 [k,2] arrays (x, y) in image pixels, in the order of their
    lowest-numbered vertex; `area_px`: their signed shoelace areas (px^2); `holes`: area_px < 0."""
    polygons: List[np.ndarray] = field(default_factory=list)
    area_px: np.ndarray = field(default_factory=lambda: np.zeros(0))
    holes: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=bool))

    def __len__(self):
        return len(self.polygons)

    @property
    def total_area_px(self) -> float:
        """Printed area: outer boundaries minus holes."""
        return float(np.sum(self.area_px))


def signedArea(polygon) -> float:
    """Shoelace area of a closed polygon [k,2] (positive: counter-clockwise in (x, y) axes)."""
    q = np.asarray(polygon, dtype=np.float64).reshape(-1, 2)
    if len(q) < 3:
        return 0.0
    return 0.5 * float(np.sum(q[:, 0] * np.roll(q[:, 1], -1) - np.roll(q[:, 0], -1) * q[:, 1]))


def _check_image(image, what):
    import torch

    from .imageformation import ShapeError
    if not isinstance(image, torch.Tensor) or image.dim() not in (2, 3) or image.shape[-1] != image.shape[-2] \
            or image.dtype != torch.float32 or image.numel() == 0:
        raise ShapeError(f"{what}: image must be a float32 tensor [n,n] or [planes,n,n]; got "
                         f"{getattr(image, 'dtype', type(image))} {tuple(getattr(image, 'shape', ()))}")
    if image.shape[-1] > 16384 or (image.dim() == 3 and image.shape[0] > 65535):
        raise ShapeError(f"{what}: at most 16384 x 16384 samples and 65535 planes; got {tuple(image.shape)}")


def _gains(doses, what):
    from .imageformation import ShapeError
    gains = [float(d) for d in doses]
    if not 1 <= len(gains) <= 64:
        raise ShapeError(f"{what}: between 1 and 64 doses per call; got {len(gains)}")
    if any(math.isnan(g) for g in gains):
        raise ValueError(f"{what}: a dose is NaN")
    return gains, (ctypes.c_float * len(gains))(*gains)


def contourVertices(image, threshold, doses=(1.0,), exposed=True):
    """The contour vertices of every (dose, plane) image, numbered and linked on the device.  `image` fp32 [n,n] or
    [planes,n,n] on the GPU; `doses` at most 64 gains; a sample is inside where (dose * image >= threshold) == exposed.
    Returns (xy, next, offsets): xy fp32 [V,2] = (x, y) in image pixels and next int32 [V] on the GPU, offsets int64
    [images + 1] on the host; image dose_index * planes + plane owns rows offsets[i] .. offsets[i + 1], and its `next` holds
    image-local indices: walking v -> next[v] goes round a closed contour with the feature on the left
    (include/litho_abbe.h has the whole definition).  Two launches count, ONE read-back of the per-image counts sizes the
    outputs -- the only host wait -- and one launch emits."""
    import torch
    _check_image(image, "contourVertices")
    gains, arr = _gains(doses, "contourVertices")
    dev = nat.require_gpu(image.device)
    img = image.contiguous()
    planes = img.shape[0] if img.dim() == 3 else 1
    n = img.shape[-1]
    images = planes * len(gains)
    lib = nat.lib()
    nbytes = int(lib.litho_contour_work_bytes(n, planes, len(gains)))
    work = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    counts = torch.empty((images,), dtype=torch.int64, device=dev)
    args = (nat.ptr(img), planes, n, arr, len(gains), float(threshold), 1 if exposed else 0, nat.ptr(work), nbytes)
    with torch.cuda.device(dev):
        nat.check(lib.litho_contour_count(*args, nat.ptr(counts), nat.stream_ptr(dev)), "litho_contour_count")
        offsets = np.zeros(images + 1, dtype=np.int64)
        np.cumsum(counts.cpu().numpy(), out=offsets[1:])                       # the one host wait
        total = int(offsets[-1])
        xy = torch.empty((total, 2), dtype=torch.float32, device=dev)
        nxt = torch.empty((total,), dtype=torch.int32, device=dev)
        # emit reads `offsets` with an asynchronous copy on the stream: the array has to outlive that copy, and it does,
        # because it is returned -- treat the returned offsets as read-only until the stream has been synchronised
        nat.check(lib.litho_contour_emit(*args, offsets.ctypes.data_as(ctypes.c_void_p), nat.ptr(xy) if total else None,
                                         nat.ptr(nxt) if total else None, nat.stream_ptr(dev)), "litho_contour_emit")
    return xy, nxt, offsets


def linkContours(next_indices):
    """(order, starts): the cycles of a contour's `next` permutation (host int32 [V]) through litho_contour_link -- `order`
    int64 [V] lists the vertices cycle by cycle, every cycle from its lowest-numbered vertex and the cycles by that number;
    `starts` int64 [cycles + 1] bounds them.  ValueError when `next_indices` is not a permutation."""
    nx = np.ascontiguousarray(np.asarray(next_indices, dtype=np.int32).reshape(-1))
    V = int(nx.shape[0])
    order = np.empty(max(V, 1), dtype=np.int64)
    starts = np.empty(V + 1, dtype=np.int64)
    cycles = ctypes.c_int64(0)
    rc = nat.lib().litho_contour_link(nx.ctypes.data_as(ctypes.c_void_p), V, order.ctypes.data_as(ctypes.c_void_p),
                                      starts.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cycles))
    if rc != nat.LITHO_OK:
        raise ValueError("linkContours: next is not a permutation of 0 .. V - 1")
    return order[:V], starts[:cycles.value + 1]


def polygonsFromVertices(xy, next_indices) -> Contours:
    """One image's vertices and links (host arrays) as polygons: the cycles of `next`; consecutive duplicate vertices
    (zero-length segments at border corners, and where a sample equals the threshold) collapse, a cycle with fewer than
    three distinct consecutive vertices is dropped."""
    pts = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    order, starts = linkContours(next_indices)
    polys, areas = [], []
    for a, b in zip(starts[:-1], starts[1:]):
        q = pts[order[a:b]]
        q = q[np.any(q != np.roll(q, 1, axis=0), axis=1)]
        if len(q) < 3:
            continue
        polys.append(np.ascontiguousarray(q))
        areas.append(signedArea(q))
    areas = np.array(areas, dtype=np.float64)
    return Contours(polys, areas, areas < 0)


def traceContours(image, threshold, doses=(1.0,), exposed=True) -> List[List[Contours]]:
    """The printed outlines as polygons: result[dose_index][plane] is a `Contours` (image pixels; outer boundaries
    counter-clockwise with positive area, holes clockwise with negative area).  Vertices come from contourVertices (one host
    wait), then the vertex and link arrays -- not the images -- are copied back and the cycles are walked on the host."""
    xy, nxt, offsets = contourVertices(image, threshold, doses, exposed)
    xy, nxt = xy.cpu().numpy(), nxt.cpu().numpy()
    planes = image.shape[0] if image.dim() == 3 else 1
    out = []
    for g in range((len(offsets) - 1) // planes):
        out.append([polygonsFromVertices(xy[offsets[i]:offsets[i + 1]], nxt[offsets[i]:offsets[i + 1]])
                    for i in range(g * planes, (g + 1) * planes)])
    return out


def contoursToLayout(polygons, pixelSize, origin, pixelNumber, wavelength) -> List[np.ndarray]:
    """Image pixels -> layout nanometres: the exact inverse of the map layoutSites applies to its sites,
    nm = ((px - offset) / scale + 0.5) * pixelSize + origin with (scale, offset) the registration of the post-processed image
    against the mask raster (imageRegistration).  `origin` = (x0, y0) as rasterizeLayout took it; `polygons` a Contours or a
    sequence of [k,2] arrays.  Orientation is kept (the map has a positive scale on both axes)."""
    from .metrology import _registration
    if isinstance(polygons, Contours):
        polygons = polygons.polygons
    ps = float(pixelSize)
    _, scale, offset = _registration(int(pixelNumber), ps, float(wavelength))
    o = np.array([float(origin[0]), float(origin[1])])
    return [((np.asarray(q, dtype=np.float64).reshape(-1, 2) - offset) / scale + 0.5) * ps + o for q in polygons]


def _distance_to_segment(p, a, b):
    d = b - a
    dd = float(d[0] * d[0] + d[1] * d[1])
    if dd == 0.0:
        return np.hypot(p[:, 0] - a[0], p[:, 1] - a[1])
    t = np.clip(((p[:, 0] - a[0]) * d[0] + (p[:, 1] - a[1]) * d[1]) / dd, 0.0, 1.0)
    return np.hypot(p[:, 0] - (a[0] + t * d[0]), p[:, 1] - (a[1] + t * d[1]))


def simplifyContour(polygon, tolerance) -> np.ndarray:
    """Douglas-Peucker on a CLOSED polygon [k,2]: vertex 0 and the vertex farthest from it are kept, the two chains between
    them are simplified; every removed vertex lies within `tolerance` of the segment of the result that replaces its chain.
    Orientation is kept: if fewer than three vertices would remain, or the sign of the area would change (a sliver thinner
    than the tolerance), the polygon is returned as it came.  tolerance <= 0 returns a copy."""
    q = np.asarray(polygon, dtype=np.float64).reshape(-1, 2)
    tol = float(tolerance)
    if not tol > 0.0 or len(q) < 4:
        return q.copy()
    k = len(q)
    far = int(np.argmax(np.hypot(q[:, 0] - q[0, 0], q[:, 1] - q[0, 1])))
    if far == 0:
        return q.copy()
    ring = np.concatenate([q, q[:1]])                                           # chain 0 .. far, chain far .. k (= vertex 0)
    keep = np.zeros(k + 1, dtype=bool)
    keep[[0, far, k]] = True
    stack = [(0, far), (far, k)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        d = _distance_to_segment(ring[a + 1:b], ring[a], ring[b])
        i = int(np.argmax(d))
        if d[i] > tol:
            m = a + 1 + i
            keep[m] = True
            stack += [(a, m), (m, b)]
    out = ring[:k][keep[:k]]
    if len(out) < 3 or (signedArea(out) > 0) != (signedArea(q) > 0):
        return q.copy()
    return out


def contoursToGDSII(polygons_nm, path: Optional[str] = None, layer: int = 0, datatype: int = 0, holeDatatype: int = 1,
                    dbu_nm: float = 0.1, tolerance_nm: float = 0.0, name: str = "CONTOURS"):
    """A GdsLibrary with one structure `name` holding the polygons (nanometres, as contoursToLayout returns them) as
    BOUNDARY elements, written with writeGDSII to `path` if given; returns the library.  A GDSII boundary has no holes, so
    clockwise polygons (negative area: holes) go on `holeDatatype`, the others on `datatype`.  Coordinates are rounded to the
    database unit `dbu_nm`; with tolerance_nm > 0 every polygon is first simplified (simplifyContour).  A polygon that rounds
    to fewer than three distinct vertices is left out; one that still has more than 8190 raises ValueError."""
    from .layout import GdsElement, GdsLibrary, GdsStructure, writeGDSII
    dbu = float(dbu_nm)
    if not (dbu > 0.0 and math.isfinite(dbu)):
        raise ValueError(f"contoursToGDSII: dbu_nm must be finite and > 0; got {dbu_nm}")
    if isinstance(polygons_nm, Contours):
        polygons_nm = polygons_nm.polygons
    lib = GdsLibrary(name="LITHO", user_unit=dbu * 1e-3, user_unit_m=dbu * 1e-9)
    cell = GdsStructure(name)
    lib.structures[name] = cell
    for q in polygons_nm:
        q = np.asarray(q, dtype=np.float64).reshape(-1, 2)
        if float(tolerance_nm) > 0.0:
            q = simplifyContour(q, float(tolerance_nm))
        hole = signedArea(q) < 0
        xy = np.rint(q / dbu).astype(np.int64)
        xy = xy[np.any(xy != np.roll(xy, 1, axis=0), axis=1)]
        if len(xy) < 3:
            continue
        if len(xy) > GDS_MAX_VERTICES:
            raise ValueError(f"contoursToGDSII: a boundary has {len(xy)} vertices, a GDSII boundary holds at most "
                             f"{GDS_MAX_VERTICES}; raise tolerance_nm")
        if np.abs(xy).max() >= 2 ** 31:
            raise ValueError("contoursToGDSII: a coordinate does not fit the 32-bit database unit; raise dbu_nm")
        cell.elements.append(GdsElement("boundary", layer=int(layer), datatype=int(holeDatatype if hole else datatype),
                                        xy=np.concatenate([xy, xy[:1]])))
    if path:
        writeGDSII(lib, path)
    return lib


def doseFocusEnvelope(image, doses=(1.0,)):
    """(lo, hi): per pixel the smallest and the largest dose * image over all doses and planes, fp32 [n,n] on the GPU."""
    import torch
    _check_image(image, "doseFocusEnvelope")
    gains, arr = _gains(doses, "doseFocusEnvelope")
    dev = nat.require_gpu(image.device)
    img = image.contiguous()
    planes = img.shape[0] if img.dim() == 3 else 1
    n = img.shape[-1]
    lo = torch.empty((n, n), dtype=torch.float32, device=dev)
    hi = torch.empty((n, n), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().litho_dose_focus_envelope(nat.ptr(img), planes, n, arr, len(gains), nat.ptr(lo), nat.ptr(hi),
                                                      nat.stream_ptr(dev)), "litho_dose_focus_envelope")
    return lo, hi


def processVariationBand(image, threshold, doses, exposed=True):
    """(outer, inner, band_area_px): the process-variation band of an image stack over its planes (focus) and `doses`.  The
    contours are traced on the envelope images: for exposed features `outer` is the contour of the per-pixel maximum (what
    prints under ANY condition), `inner` that of the minimum (what prints under EVERY condition); for dark features
    (exposed=False) the other way round.  band_area_px = area(outer) - area(inner) >= 0, holes counted negative."""
    lo, hi = doseFocusEnvelope(image, doses)
    big, small = (hi, lo) if exposed else (lo, hi)
    outer = traceContours(big, threshold, (1.0,), exposed)[0][0]
    inner = traceContours(small, threshold, (1.0,), exposed)[0][0]
    return outer, inner, outer.total_area_px - inner.total_area_px
