"""Tiled imaging of layouts larger than one window; no reference counterpart.

Every imaging entry takes one mask of one power-of-two grid and images it as ONE window.  A layout block a few times larger is
cut into windows of pn x pn raster pixels on one pixel lattice; each window is imaged on its own (rasterizeLayout, Mask.fraunhofer,
hopkinsIntensityBatch, postProcess: all windows of a chunk in one batch), and only its CORE -- the window without a halo of
`halo` pixels on every side -- is trusted and copied into the stitched image (litho_tiles_stitch).  The halo is the knob: what lies
farther than the halo from a core pixel is imaged wrongly for it (the window's periodic continuation instead of the layout), and
`seamError` reads the knob out -- the largest disagreement of two neighbouring windows on the two pixel lines either side of the
boundary between their cores (litho_tiles_seam), relative to the image's maximum.

Geometry.  Raster pixel g of the lattice covers [origin + g * pixelSize, origin + (g + 1) * pixelSize) on both
axes.  core = pn - 2 * halo; tile (ix, iy) owns the raster pixels [ix * core, (ix + 1) * core) x [iy * core, (iy + 1) * core) and its
window starts `halo` pixels before them.  A single window shows its raster pixel i at image pixel i + offset
(metrology._registration, scale 1); with offset = o_int + o_frac, the core of a window's image starts at j0 = halo + o_int, and the
stitched image shows raster pixel g at G = g + o_frac: `offset_px` = o_frac, the same fraction as a single window's.

Caveat.  With epsilon != 1 the reference's resample chain (bilinear by epsilon, transform, bilinear by 1 / epsilon) is not
translation invariant: two windows image the same feature slightly differently WHATEVER the halo.  In the float64 restatement of
this driver (pn 64, 25 nm, 193 nm) two tilings of one layout differ by 4-6 % of the maximum at halo 8, 14 and 20 alike.  At a pixel
size with epsilon = 1, pixelSize = wavelength * pn / (4 N) (193 / 8 nm at 193 nm), the same measure falls with the halo
(tests/test_tiling_cpu.py)."""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from .metrology import LayoutSites, _epsilon_n, _registration, layoutSites


def tileValidRegion(pixelNumber: int, pixelSize: float, wavelength: float) -> Tuple[int, int]:
    """(lo, hi): the pixels [lo, hi) of one window's post-processed image, on either axis, that show mask raster -- image pixel J
    shows raster pixel J - offset (metrology._registration), which must lie in [0, pn - 1], and J must not lie in the zero padding
    postProcess adds (epsilon > 1: the field crop drops (ns - pn) / 2 resampled raster pixels per side and the image is padded
    by pW in front and pW + size % 2 behind) nor be cropped by it (epsilon < 1).  Raises ValueError where the registration's
    scale is not 1: the degenerate case in which one of the two resamplings is a plain copy and the other's scale is left over."""
    pn = int(pixelNumber)
    n_out, scale, offset = _registration(pn, pixelSize, wavelength)
    if scale != 1.0:
        raise ValueError(f"tileValidRegion: at pixelNumber {pn}, pixelSize {pixelSize}, wavelength {wavelength} the image is "
                         f"scaled by {scale!r} against the mask raster (one resampling degenerates to a copy); windows cannot "
                         "be stitched on one pixel lattice")
    eps, _ = _epsilon_n(4.0 / pn, float(pixelSize), float(wavelength))
    n_back = int(math.floor(pn * (1.0 / eps)))
    pW = (pn - round(pn / eps)) // 2
    pad_lo, pad_hi = max(pW, 0), max(pW + n_back % 2, 0)
    lo = max(pad_lo, int(math.ceil(offset)))
    hi = min(n_out - pad_hi, int(math.floor(pn - 1 + offset)) + 1)
    return lo, hi


@dataclass
class TilePlan:
    """What planTiles returns.  Tile t = iy * nx + ix; `windows_nm` float64 [T,2] = (x0, y0) of each window's lower-left corner,
    what rasterizeLayout takes as origin; `place` int32 [T,2] = (row, col) of the core's first pixel in the stitched image;
    `neighbours` int32 [T,2] = (right, lower) tile (ix + 1, iy) and (ix, iy + 1), -1 where there is none; `j0` the first core
    pixel of a window's image; `n` the side of the (square) stitched image, core * max(nx, ny); `origin` (x0, y0) of the
    stitched raster's pixel 0 in nm; `offset_px`: stitched image pixel G shows raster pixel G - offset_px; `n_tile` the side of
    one window's post-processed image."""
    pixelNumber: int
    pixelSize: float
    wavelength: float
    halo: int
    core: int
    j0: int
    nx: int
    ny: int
    n: int
    n_tile: int
    origin: Tuple[float, float]
    bounds: Tuple[float, float, float, float]
    offset_px: float
    windows_nm: np.ndarray
    place: np.ndarray
    neighbours: np.ndarray

    @property
    def count(self) -> int:
        return int(self.place.shape[0])

    @property
    def registration(self):
        """(n, scale, offset) of the stitched image, what layoutSites(registration=...) takes."""
        return self.n, 1.0, self.offset_px


def planTiles(bounds_nm, pixelNumber: int, pixelSize: float, wavelength: float, halo: int, origin=None) -> TilePlan:
    """The windows that image the rectangle `bounds_nm` = (x0, y0, x1, y1) (nanometres) with cores of pn - 2 * halo pixels; host
    only.  `origin` = (x, y) of the pixel lattice (None: the bounds' lower-left corner); the windows step by `core` pixels of that
    lattice, tile (0, 0) being the one whose core holds the bounds' first pixel.  The cores tile the bounds' pixels without gap or
    overlap and every core lies inside tileValidRegion of its window's image, the integer part of the registration offset
    included.  ValueError: core < 1, bounds that are not finite or empty, a core that leaves the valid region (the halo is
    smaller than the padding of this pixel size), or a registration scale other than 1."""
    pn, ps, halo = int(pixelNumber), float(pixelSize), int(halo)
    b = [float(v) for v in bounds_nm]
    if len(b) != 4 or not all(math.isfinite(v) for v in b) or not (b[2] > b[0] and b[3] > b[1]):
        raise ValueError(f"planTiles: bounds must be finite (x0, y0, x1, y1) with x1 > x0 and y1 > y0; got {tuple(bounds_nm)}")
    core = pn - 2 * halo
    if halo < 0 or core < 1:
        raise ValueError(f"planTiles: halo {halo} leaves a core of {core} pixels at pixelNumber {pn}")
    lo, hi = tileValidRegion(pn, ps, wavelength)
    n_tile, _, offset = _registration(pn, ps, wavelength)
    o_int = int(math.floor(offset))
    j0 = halo + o_int
    if j0 < lo or j0 + core > hi:
        raise ValueError(f"planTiles: the core [{j0}, {j0 + core}) of a window's image leaves its valid region [{lo}, {hi}) at "
                         f"pixelNumber {pn}, pixelSize {ps}: halo {halo} is too small")
    if origin is None:
        origin = (b[0], b[1])
    ox, oy = float(origin[0]), float(origin[1])
    if not (math.isfinite(ox) and math.isfinite(oy)):
        raise ValueError(f"planTiles: origin must be finite; got {origin}")
    # the bounds' pixels on the lattice, then the tiles that hold them
    gx0, gy0 = int(math.floor((b[0] - ox) / ps)), int(math.floor((b[1] - oy) / ps))
    gx1, gy1 = max(gx0 + 1, int(math.ceil((b[2] - ox) / ps))), max(gy0 + 1, int(math.ceil((b[3] - oy) / ps)))
    ix0, iy0 = gx0 // core, gy0 // core
    nx, ny = -(-gx1 // core) - ix0, -(-gy1 // core) - iy0
    n = core * max(nx, ny)
    base = (ox + ix0 * core * ps, oy + iy0 * core * ps)
    T = nx * ny
    windows = np.empty((T, 2), dtype=np.float64)
    place = np.empty((T, 2), dtype=np.int32)
    neighbours = np.full((T, 2), -1, dtype=np.int32)
    for iy in range(ny):
        for ix in range(nx):
            t = iy * nx + ix
            windows[t] = (base[0] + (ix * core - halo) * ps, base[1] + (iy * core - halo) * ps)
            place[t] = (iy * core, ix * core)
            if ix + 1 < nx:
                neighbours[t, 0] = t + 1
            if iy + 1 < ny:
                neighbours[t, 1] = t + nx
    return TilePlan(pn, ps, float(wavelength), halo, core, j0, nx, ny, n, int(n_tile), base, tuple(b), offset - o_int, windows, place,
                    neighbours)


class TiledImage:
    """What hopkinsImageTiled returns.  `image` fp32 [n,n] (or [planes,n,n] for the kernels of a pupil stack) on the GPU: the
    stitched cores, zero where no tile lies (the image is square, the bounds need not be); `plan` the TilePlan; `seam` fp32
    [T,planes,2], litho_tiles_seam's output (NaN where a tile has no right / lower neighbour); `seamError` = max seam / max image,
    a float (NaN for a single tile or a halo of 0, where no seam can be measured): the halo's read-out, reported as `captured`
    is for the kernels."""

    def __init__(self, image, plan, seam, seamError):
        self.image, self.plan, self.seam, self.seamError = image, plan, seam, seamError

    def sites(self, polygons: Sequence[np.ndarray], spacing: float) -> LayoutSites:
        """layoutSites of `polygons` (nanometres) on the stitched grid: what measureEPE takes together with `image`."""
        p = self.plan
        return layoutSites(polygons, spacing, p.pixelSize, p.origin, p.pixelNumber, p.wavelength, registration=p.registration)

    def toLayout(self, contours) -> List[np.ndarray]:
        """Stitched-image pixels -> layout nanometres, the inverse of `sites`' map: for traceContours(image, ...) on the way to
        contoursToGDSII.  `contours` a Contours or a sequence of [k,2] arrays; orientation is kept."""
        from .contours import Contours
        if isinstance(contours, Contours):
            contours = contours.polygons
        p = self.plan
        o = np.array([p.origin[0], p.origin[1]])
        return [(np.asarray(q, dtype=np.float64).reshape(-1, 2) - p.offset_px + 0.5) * p.pixelSize + o for q in contours]


def _bounding_boxes(polygons):
    """(polygons as float64 [k,2] arrays with k >= 3, their boxes float64 [P,4] = x0, y0, x1, y1)."""
    polys = [q for q in (np.asarray(q, dtype=np.float64).reshape(-1, 2) for q in polygons) if len(q) >= 3]
    boxes = np.array([[q[:, 0].min(), q[:, 1].min(), q[:, 0].max(), q[:, 1].max()] for q in polys], dtype=np.float64).reshape(-1, 4)
    return polys, boxes


def stitchTiles(tiles, place, j0, core, image):
    """litho_tiles_stitch: the cores of `tiles` fp32 [count,planes,nt,nt] into `image` fp32 [planes,n,n] at `place` int32
    [count,2] (device); returns image."""
    import torch
    from .imageformation import ShapeError
    tiles, place = tiles.contiguous(), place.contiguous()
    count, planes, nt = int(tiles.shape[0]), int(tiles.shape[1]), int(tiles.shape[-1])
    dev = nat.require_gpu(tiles.device)
    if (tiles.dtype != torch.float32 or image.dtype != torch.float32 or not image.is_contiguous() or place.dtype != torch.int32
            or tuple(place.shape) != (count, 2) or image.dim() != 3 or image.shape[0] != planes or image.shape[1] != image.shape[2]
            or image.device != dev or place.device != dev):
        raise ShapeError(f"stitchTiles: fp32 tiles [count,planes,nt,nt], int32 place [count,2] and a contiguous fp32 image [planes,n,n] "
                         f"on one GPU; got {tuple(tiles.shape)}, {tuple(place.shape)}, {tuple(image.shape)}")
    with torch.cuda.device(dev):
        nat.check(nat.lib().litho_tiles_stitch(nat.ptr(tiles), count, planes, nt, nat.ptr(place), int(j0), int(core), nat.ptr(image),
                                               int(image.shape[-1]), nat.stream_ptr(dev)), "litho_tiles_stitch")
    return image


def seamTiles(tiles, neighbours, j0, core):
    """litho_tiles_seam: fp32 [count,planes,2] from `tiles` fp32 [count,planes,nt,nt] and `neighbours` int32 [count,2] (device)."""
    import torch
    from .imageformation import ShapeError
    tiles, neighbours = tiles.contiguous(), neighbours.contiguous()
    count, planes, nt = int(tiles.shape[0]), int(tiles.shape[1]), int(tiles.shape[-1])
    dev = nat.require_gpu(tiles.device)
    if tiles.dtype != torch.float32 or neighbours.dtype != torch.int32 or tuple(neighbours.shape) != (count, 2) or neighbours.device != dev:
        raise ShapeError(f"seamTiles: fp32 tiles [count,planes,nt,nt] and int32 neighbours [count,2] on one GPU; got "
                         f"{tuple(tiles.shape)}, {tuple(neighbours.shape)}")
    out = torch.empty((count, planes, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().litho_tiles_seam(nat.ptr(tiles), count, planes, nt, nat.ptr(neighbours), int(j0), int(core), nat.ptr(out),
                                             nat.stream_ptr(dev)), "litho_tiles_seam")
    return out


def hopkinsImageTiled(polygons, socs, pixelNumber: int, pixelSize: float, wavelength: float, bounds=None, halo: Optional[int] = None,
                      antialias: int = 1, normalize: bool = False, tileChunk: Optional[int] = None, origin=None) -> TiledImage:
    """The Hopkins aerial image of a layout larger than one window.  `polygons` in nanometres (as rasterizeLayout takes them),
    `socs` the SOCSKernels of the optical setting at `pixelNumber` (on the GPU), `bounds` = (x0, y0, x1, y1) the rectangle to
    image (None: the polygons' bounding box), `halo` in pixels (None: pixelNumber / 4), `antialias` and `normalize` as
    rasterizeLayout and hopkinsImage take them, `origin` the pixel lattice's (planTiles).

    Per chunk of `tileChunk` tiles (None: what keeps hopkinsIntensityBatch's workspace under socs.STACK_BYTES): the polygons
    are culled against each window by bounding box on the host, every window is rasterised and transformed by the existing
    entries (rasterizeLayout(origin=window), Mask.fraunhofer), then ONE hopkinsIntensityBatch, ONE postProcess with the chunk's
    tiles as planes, ONE litho_tiles_stitch.  litho_tiles_seam runs per chunk on the chunk and the one row of tiles before it
    (the only earlier tiles a later one can border), so no more than nx + tileChunk window images are alive at a time.  A window
    without a polygon is imaged like any other: a dark or clear field is not zero intensity for a phase mask or a bright
    background.  The image does not depend on tileChunk, bit for bit.

    See the module's caveat: with epsilon != 1 neighbouring windows differ by a few percent whatever the halo."""
    import torch

    from . import socs as _socs
    from .imageformation import ShapeError, postProcess
    from .layout import rasterizeLayout
    from .mask import Mask
    if not isinstance(socs, _socs.SOCSKernels):
        raise TypeError("hopkinsImageTiled: socs must be the SOCSKernels socsKernels returned")
    pn, ps = int(pixelNumber), float(pixelSize)
    if socs.pn != pn:
        raise ShapeError(f"hopkinsImageTiled: the kernels are {socs.pn} x {socs.pn}, pixelNumber is {pn}")
    dev = nat.require_gpu(socs.kernels.device)
    polys, boxes = _bounding_boxes(polygons)
    if bounds is None:
        if not polys:
            raise ValueError("hopkinsImageTiled: no polygon and no bounds")
        bounds = (boxes[:, 0].min(), boxes[:, 1].min(), boxes[:, 2].max(), boxes[:, 3].max())
    plan = planTiles(bounds, pn, ps, wavelength, pn // 4 if halo is None else halo, origin)
    planes, K, T, nt = socs.planes, socs.K, plan.count, plan.n_tile
    if tileChunk is None:
        tileChunk = max(1, _socs.STACK_BYTES // (planes * (K * 8 + 4) * pn * pn))
    tileChunk = int(tileChunk)
    if tileChunk < 1:
        raise ValueError(f"hopkinsImageTiled: tileChunk must be >= 1; got {tileChunk}")
    eps, N = nat.epsilon_n(4.0 / pn, ps, float(wavelength))
    image = torch.zeros((planes, plan.n, plan.n), dtype=torch.float32, device=dev)
    place = torch.from_numpy(plan.place).to(dev)
    can_seam = plan.j0 >= 1 and plan.j0 + plan.core < nt
    seam = torch.full((T, planes, 2), float("nan"), dtype=torch.float32, device=dev)
    kept, kept_ids = None, np.zeros(0, dtype=np.int64)                # the last row of window images and their tile numbers
    span = pn * ps
    for t0 in range(0, T, tileChunk):
        t1 = min(T, t0 + tileChunk)
        specs = torch.empty((t1 - t0, pn, pn), dtype=torch.complex64, device=dev)
        for t in range(t0, t1):
            wx, wy = plan.windows_nm[t]
            hit = (boxes[:, 2] > wx) & (boxes[:, 0] < wx + span) & (boxes[:, 3] > wy) & (boxes[:, 1] < wy + span)
            raster = rasterizeLayout([polys[i] for i in np.nonzero(hit)[0]], pn, ps, origin=(wx, wy), device=dev, antialias=antialias)
            mask = Mask(transmission=raster, pixelSize=ps, device=dev) if int(antialias) > 1 else Mask(raster, ps, dev)
            specs[t - t0] = mask.fraunhofer(wavelength, True)
        raw = _socs.hopkinsIntensityBatch(specs, socs, N, tileChunk=t1 - t0)
        if normalize and socs.weight_sum > 0:
            raw /= float(socs.weight_sum)
        tiles = postProcess(raw.reshape(-1, pn, pn), eps).reshape(t1 - t0, planes, nt, nt)
        stitchTiles(tiles, place[t0:t1], plan.j0, plan.core, image)
        if can_seam and T > 1:
            # the chunk behind the kept tiles; a pair is measured when its later tile arrives, so every pair is measured once
            ids = np.concatenate([kept_ids, np.arange(t0, t1)])
            both = tiles if kept is None else torch.cat([kept, tiles])
            local = {int(g): i for i, g in enumerate(ids)}
            nb = np.full((len(ids), 2), -1, dtype=np.int32)
            for i, g in enumerate(ids):
                for side in (0, 1):
                    other = int(plan.neighbours[g, side])
                    if t0 <= other < t1:
                        nb[i, side] = local[other]
            part = seamTiles(both, torch.from_numpy(nb).to(dev), plan.j0, plan.core)
            at = torch.from_numpy(ids).to(dev)
            seam[at] = torch.fmax(seam[at], part)
            keep = ids >= t1 - plan.nx
            kept_ids = ids[keep]
            kept = both[torch.from_numpy(np.nonzero(keep)[0]).to(dev)]
    seam_error = float("nan")
    if can_seam and T > 1:
        finite = seam[~torch.isnan(seam)]
        top = float(image.max())
        if finite.numel() and top > 0:
            seam_error = float(finite.max()) / top
    return TiledImage(image if socs.stacked else image[0], plan, seam, seam_error)
