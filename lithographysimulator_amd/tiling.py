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


def tileEdgeIndex(polygons, plan: TilePlan, orient: bool = True):
    """(edges float64 [E,4], offsets int64 [T + 1], index int32 [M]) on the host: `edges` = polygonEdges(polygons, orient), and
    tile t of `plan` rasterises the edges index[offsets[t]:offsets[t + 1]], ascending.  Culling is per POLYGON, never per edge: a
    polygon belongs to a tile when its bounding box overlaps the window (strictly: touching a border is no overlap), and then
    ALL its edges do -- an edge to the right of a window adds winding to every column of its rows, which only the polygon's other
    edges cancel.  No Python loop over polygons times tiles."""
    from .layout import polygonEdgeOwners, polygonEdges
    if not isinstance(plan, TilePlan):
        raise TypeError("tileEdgeIndex: plan must be the TilePlan planTiles returned")
    polygons = list(polygons)
    edges = polygonEdges(polygons, orient=orient)
    owner = polygonEdgeOwners(polygons)
    E, T, P = int(edges.shape[0]), plan.count, len(polygons)
    if E >= 2 ** 31:
        raise ValueError(f"tileEdgeIndex: {E} edges do not fit the int32 index")
    if E == 0:
        return edges, np.zeros(T + 1, dtype=np.int64), np.zeros(0, dtype=np.int32)
    xs, ys = edges[:, 0], edges[:, 1]                       # every vertex starts one edge
    boxes = np.empty((P, 4))
    boxes[:, :2], boxes[:, 2:] = np.inf, -np.inf
    np.minimum.at(boxes[:, 0], owner, xs)
    np.minimum.at(boxes[:, 1], owner, ys)
    np.maximum.at(boxes[:, 2], owner, xs)
    np.maximum.at(boxes[:, 3], owner, ys)
    span = plan.pixelNumber * plan.pixelSize
    wx, wy = plan.windows_nm[:, 0:1], plan.windows_nm[:, 1:2]
    hit = (boxes[None, :, 2] > wx) & (boxes[None, :, 0] < wx + span) & (boxes[None, :, 3] > wy) & (boxes[None, :, 1] < wy + span)
    tt, pp = np.nonzero(hit)                                # by tile, then polygon
    by_owner = np.argsort(owner, kind="stable")             # a polygon's edges, ascending
    count = np.bincount(owner, minlength=P)
    start = np.cumsum(count) - count
    n = count[pp]
    total = int(n.sum())
    first = np.cumsum(n) - n
    within = np.arange(total, dtype=np.int64) - np.repeat(first, n)
    tile = np.repeat(tt, n)
    picked = by_owner[np.repeat(start[pp], n) + within]
    order = np.argsort(tile.astype(np.int64) * E + picked, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(tile, minlength=T))]).astype(np.int64)
    return edges, offsets, picked[order].astype(np.int32)


def _check_tile_index(who, edges, offsets, index, tiles):
    """The host-side check the C entry cannot make: shapes, ascending offsets inside the index, edge numbers inside the edges."""
    if (edges.ndim != 2 or edges.shape[1] != 4 or offsets.shape != (tiles + 1,) or index.ndim != 1 or offsets[0] < 0
            or np.any(np.diff(offsets) < 0) or offsets[-1] > index.shape[0]
            or (index.size and (int(index.min()) < 0 or int(index.max()) >= edges.shape[0]))):
        raise ValueError(f"{who}: the tile index does not fit its edges ({edges.shape}, {offsets.shape}, {index.shape} for {tiles} tiles)")


def _upload_tile_index(who, polygons, plan, orient, dev):
    """tileEdgeIndex on the device: (edges, offsets, index, windows), ONE upload of each."""
    import torch
    edges, offsets, index = tileEdgeIndex(polygons, plan, orient)
    _check_tile_index(who, edges, offsets, index, plan.count)
    return (torch.from_numpy(edges).to(dev), torch.from_numpy(offsets).to(dev), torch.from_numpy(index).to(dev),
            torch.from_numpy(np.ascontiguousarray(plan.windows_nm, dtype=np.float64)).to(dev))


def _raster_tiles(arrays, plan, antialias, t0, t1):
    from .layout import rasterizeCoverageTiles
    edges, offsets, index, windows = arrays
    return rasterizeCoverageTiles(edges, offsets[t0:t1 + 1], index, windows[t0:t1], plan.pixelNumber, plan.pixelSize, antialias)


def rasterizeLayoutTiles(polygons, plan: TilePlan, antialias: int = 16, device=None, orient: bool = True, tiles=None):
    """The area coverage of every window of `plan`: float32 [count,pn,pn], window t bit for bit
    rasterizeLayout(the polygons whose boxes overlap it, pn, pixelSize, origin=plan.windows_nm[t], antialias=antialias) -- all of
    them in ONE launch (litho_rasterize_coverage_tiles) after ONE upload of the edges and of the per-tile index (tileEdgeIndex).
    antialias = 1 gives 0.0 / 1.0, the binary raster as a transmission.  `tiles` = (t0, t1) rasterises the windows t0 .. t1 - 1
    only; a window's bits do not depend on the others.  `orient` as rasterizeLayout takes it."""
    from .layout import ANTIALIAS_LEVELS
    if not isinstance(plan, TilePlan):
        raise TypeError("rasterizeLayoutTiles: plan must be the TilePlan planTiles returned")
    s = int(antialias)
    if s != antialias or s not in ANTIALIAS_LEVELS:
        raise ValueError(f"rasterizeLayoutTiles: antialias must be one of {ANTIALIAS_LEVELS}; got {antialias!r}")
    if plan.pixelNumber * s > 32768:
        raise ValueError(f"rasterizeLayoutTiles: pixelNumber * antialias must lie in 1..32768; got {plan.pixelNumber} * {s}")
    t0, t1 = (0, plan.count) if tiles is None else (int(tiles[0]), int(tiles[1]))
    if not 0 <= t0 < t1 <= plan.count:
        raise ValueError(f"rasterizeLayoutTiles: tiles must be (t0, t1) with 0 <= t0 < t1 <= {plan.count}; got {tiles!r}")
    if not np.isfinite(plan.windows_nm).all():
        raise ValueError("rasterizeLayoutTiles: a window origin of the plan is not finite")
    dev = nat.require_gpu(nat.pick_device(device, "layout"))
    return _raster_tiles(_upload_tile_index("rasterizeLayoutTiles", polygons, plan, orient, dev), plan, s, t0, t1)


def _sweep_layout(polygons, socs, plan, antialias, divide, chunks, dev, orient=True, each=None, spectra=None):
    """The stitched image fp32 [planes,n,n] of a layout, the sweep hopkinsImageTiled, correctLayoutTiled and epeJacobianTiled
    share: ONE upload of the culled edges; per chunk (t0, t1) ONE raster launch, the window spectra, ONE hopkinsIntensityBatch,
    the division by `divide` (None: none), ONE postProcess with the windows as planes, ONE stitch.  `each(t0, t1, tiles)` sees
    every chunk's window images; `spectra` (a dict) receives the spectrum of every window under its tile number."""
    import torch

    from . import socs as _socs
    from .imageformation import postProcess
    pn, planes, nt = plan.pixelNumber, socs.planes, plan.n_tile
    eps, N = nat.epsilon_n(4.0 / pn, plan.pixelSize, float(plan.wavelength))
    arrays = _upload_tile_index("tiled imaging", polygons, plan, orient, dev)
    image = torch.zeros((planes, plan.n, plan.n), dtype=torch.float32, device=dev)
    place = torch.from_numpy(plan.place).to(dev)
    for t0, t1 in chunks:
        specs = _window_spectra(_raster_tiles(arrays, plan, antialias, t0, t1), plan, eps, N)
        if spectra is not None:
            for t in range(t0, t1):
                spectra[t] = specs[t - t0]
        raw = _socs.hopkinsIntensityBatch(specs, socs, N, tileChunk=t1 - t0)
        if divide is not None:
            raw /= divide
        tiles = postProcess(raw.reshape(-1, pn, pn), eps).reshape(t1 - t0, planes, nt, nt)
        stitchTiles(tiles, place[t0:t1], plan.j0, plan.core, image)
        if each is not None:
            each(t0, t1, tiles)
    return image


def hopkinsImageTiled(polygons, socs, pixelNumber: int, pixelSize: float, wavelength: float, bounds=None, halo: Optional[int] = None,
                      antialias: int = 1, normalize: bool = False, tileChunk: Optional[int] = None, origin=None) -> TiledImage:
    """The Hopkins aerial image of a layout larger than one window.  `polygons` in nanometres (as rasterizeLayout takes them),
    `socs` the SOCSKernels of the optical setting at `pixelNumber` (on the GPU), `bounds` = (x0, y0, x1, y1) the rectangle to
    image (None: the polygons' bounding box), `halo` in pixels (None: pixelNumber / 4), `antialias` and `normalize` as
    rasterizeLayout and hopkinsImage take them, `origin` the pixel lattice's (planTiles).

    The polygons are culled against every window by bounding box on the host (tileEdgeIndex) and uploaded once.  Per chunk of
    `tileChunk` tiles (None: what keeps hopkinsIntensityBatch's workspace under socs.STACK_BYTES): the chunk's windows are
    rasterised in ONE launch (rasterizeCoverageTiles: the bits of rasterizeLayout(origin=window) per window) and transformed by
    the mask-spectrum entry, then ONE hopkinsIntensityBatch, ONE postProcess with the chunk's tiles as planes, ONE
    litho_tiles_stitch.  litho_tiles_seam runs per chunk on the chunk and the one row of tiles before it
    (the only earlier tiles a later one can border), so no more than nx + tileChunk window images are alive at a time.  A window
    without a polygon is imaged like any other: a dark or clear field is not zero intensity for a phase mask or a bright
    background.  The image does not depend on tileChunk, bit for bit.

    See the module's caveat: with epsilon != 1 neighbouring windows differ by a few percent whatever the halo."""
    import torch

    from . import socs as _socs
    from .imageformation import ShapeError
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
    can_seam = plan.j0 >= 1 and plan.j0 + plan.core < nt
    seam = torch.full((T, planes, 2), float("nan"), dtype=torch.float32, device=dev)
    state = {"kept": None, "ids": np.zeros(0, dtype=np.int64)}        # the last row of window images and their tile numbers

    def measure_seams(t0, t1, tiles):
        # the chunk behind the kept tiles; a pair is measured when its later tile arrives, so every pair is measured once
        kept, kept_ids = state["kept"], state["ids"]
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
        state["ids"] = ids[keep]
        state["kept"] = both[torch.from_numpy(np.nonzero(keep)[0]).to(dev)]

    chunks = [(t0, min(T, t0 + tileChunk)) for t0 in range(0, T, tileChunk)]
    image = _sweep_layout(polys, socs, plan, antialias, float(socs.weight_sum) if normalize and socs.weight_sum > 0 else None, chunks,
                          dev, each=measure_seams if can_seam and T > 1 else None)
    seam_error = float("nan")
    if can_seam and T > 1:
        finite = seam[~torch.isnan(seam)]
        top = float(image.max())
        if finite.numel() and top > 0:
            seam_error = float(finite.max()) / top
    return TiledImage(image if socs.stacked else image[0], plan, seam, seam_error)


# ---- tiled inverse lithography -----------------------------------------------------------------------------------------------------
def _tile_args(who, place, dev):
    import torch
    from .imageformation import ShapeError
    if not isinstance(place, torch.Tensor) or place.dtype != torch.int32 or place.dim() != 2 or place.shape[1] != 2 or place.shape[0] < 1:
        raise ShapeError(f"{who}: place must be an int32 tensor [count,2]; got {getattr(place, 'dtype', type(place).__name__)} "
                         f"{tuple(getattr(place, 'shape', ()))}")
    if place.device != dev:
        raise ShapeError(f"{who}: place lives on {place.device}, the data on {dev}")
    return place.contiguous()


def cutTiles(plane, place, pixelNumber, halo, fill=0.0):
    """litho_tiles_cut: complex64 [count,pn,pn], window t = plane[place[t] - halo ... + pn) on both axes, `fill` (complex) where
    that leaves `plane` complex64 [rows,cols]; `place` int32 [count,2] = (row, col) of each core's first pixel (device)."""
    import torch
    from .imageformation import ShapeError
    if not isinstance(plane, torch.Tensor) or plane.dtype != torch.complex64 or plane.dim() != 2:
        raise ShapeError(f"cutTiles: plane must be a complex64 tensor [rows,cols]; got {getattr(plane, 'dtype', type(plane).__name__)} "
                         f"{tuple(getattr(plane, 'shape', ()))}")
    dev = nat.require_gpu(plane.device)
    place = _tile_args("cutTiles", place, dev)
    pn, halo, fill = int(pixelNumber), int(halo), complex(fill)
    rows, cols, count = int(plane.shape[0]), int(plane.shape[1]), int(place.shape[0])
    if pn < 1 or halo < 0 or 2 * halo >= pn or pn - 2 * halo > min(rows, cols):
        raise ShapeError(f"cutTiles: halo {halo} at pixelNumber {pn} leaves no core inside a plane of {rows} x {cols}")
    plane = plane.contiguous()
    windows = torch.empty((count, pn, pn), dtype=torch.complex64, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().litho_tiles_cut(nat.ptr(plane), rows, cols, nat.ptr(place), count, pn, halo, fill.real, fill.imag,
                                            nat.ptr(windows), nat.stream_ptr(dev)), "litho_tiles_cut")
    return windows


def overlapAddTiles(windows, place, halo, rows, cols):
    """litho_tiles_overlap_add, the adjoint of cutTiles: complex64 [rows,cols], every pixel the sum of the `windows` complex64
    [count,pn,pn] samples that show it, in ascending tile order in fp32 from zero (no atomics); what a window holds outside the
    plane is dropped."""
    import torch
    from .imageformation import ShapeError
    if (not isinstance(windows, torch.Tensor) or windows.dtype != torch.complex64 or windows.dim() != 3
            or windows.shape[1] != windows.shape[2]):
        raise ShapeError(f"overlapAddTiles: windows must be a complex64 tensor [count,pn,pn]; got "
                         f"{getattr(windows, 'dtype', type(windows).__name__)} {tuple(getattr(windows, 'shape', ()))}")
    dev = nat.require_gpu(windows.device)
    place = _tile_args("overlapAddTiles", place, dev)
    count, pn, halo, rows, cols = int(windows.shape[0]), int(windows.shape[-1]), int(halo), int(rows), int(cols)
    if int(place.shape[0]) != count:
        raise ShapeError(f"overlapAddTiles: {count} windows and {int(place.shape[0])} places")
    if rows < 1 or cols < 1 or halo < 0 or 2 * halo >= pn or pn - 2 * halo > min(rows, cols):
        raise ShapeError(f"overlapAddTiles: halo {halo} at pixelNumber {pn} leaves no core inside a plane of {rows} x {cols}")
    windows = windows.contiguous()
    plane = torch.empty((rows, cols), dtype=torch.complex64, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().litho_tiles_overlap_add(nat.ptr(windows), count, pn, halo, nat.ptr(place), nat.ptr(plane), rows, cols,
                                                    nat.stream_ptr(dev)), "litho_tiles_overlap_add")
    return plane


def unstitchTiles(image, place, nt, j0, core):
    """litho_tiles_unstitch, the adjoint of stitchTiles: fp32 [count,planes,nt,nt], the cores read back from `image` fp32
    [planes,n,n] at `place` int32 [count,2] (device) and zero around them."""
    import torch
    from .imageformation import ShapeError
    if (not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or image.dim() != 3 or image.shape[1] != image.shape[2]):
        raise ShapeError(f"unstitchTiles: image must be an fp32 tensor [planes,n,n]; got {getattr(image, 'dtype', type(image).__name__)} "
                         f"{tuple(getattr(image, 'shape', ()))}")
    dev = nat.require_gpu(image.device)
    place = _tile_args("unstitchTiles", place, dev)
    planes, n, count, nt, j0, core = int(image.shape[0]), int(image.shape[-1]), int(place.shape[0]), int(nt), int(j0), int(core)
    if nt < 1 or core < 1 or j0 < 0 or j0 + core > nt or core > n:
        raise ShapeError(f"unstitchTiles: the core [{j0}, {j0 + core}) leaves a window image of {nt} or a stitched image of {n}")
    image = image.contiguous()
    tiles = torch.empty((count, planes, nt, nt), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.lib().litho_tiles_unstitch(nat.ptr(image), n, nat.ptr(place), count, planes, nt, j0, core, nat.ptr(tiles),
                                                 nat.stream_ptr(dev)), "litho_tiles_unstitch")
    return tiles


def maskPolygons(plan: TilePlan, mask, level: float = 0.5) -> List[np.ndarray]:
    """The cells of a mask on the plan's raster lattice as polygons in layout nanometres: `mask` an ILTResult of optimizeMaskTiled
    or a bool / real [ny core, nx core] tensor (cell (r, c) covers origin + (c, r) ... (c + 1, r + 1) pixels).  The outlines are
    traceContours' at `level`, a cell's centre sitting at (c + 0.5, r + 0.5) pixels: what contoursToGDSII takes."""
    import torch

    from .contours import traceContours
    m = getattr(mask, "mask", mask)
    m = torch.as_tensor(m).to(torch.float32)
    traced = traceContours(m, float(level))[0][0]
    o = np.array([plan.origin[0], plan.origin[1]])
    return [(np.asarray(q, dtype=np.float64).reshape(-1, 2) + 0.5) * plan.pixelSize + o for q in getattr(traced, "polygons", traced)]


def _window_spectra(windows, plan, eps, N):
    """complex64 [count,pn,pn]: the spectra of `windows` (transmissions, complex or real) by the mask-spectrum entry, window by
    window."""
    import torch
    from .mask import Mask
    specs = torch.empty(windows.shape, dtype=torch.complex64, device=windows.device)
    for b in range(int(windows.shape[0])):
        specs[b] = Mask(transmission=windows[b], pixelSize=plan.pixelSize, device=windows.device)._ffFraunhofer(eps, N)
    return specs


def _image_windows(windows, socs, plan, place, gain, chunks, keep=False):
    """(image fp32 [planes,n,n], {t0: spectra of the chunk that starts at t0} when `keep`): per chunk (t0, t1) of `windows` the
    spectra, ONE hopkinsIntensityBatch, the gain, ONE postProcess with the windows as planes, ONE stitch."""
    import torch

    from . import socs as _socs
    from .imageformation import postProcess
    pn, planes, nt = plan.pixelNumber, socs.planes, plan.n_tile
    eps, N = nat.epsilon_n(4.0 / pn, plan.pixelSize, plan.wavelength)
    image = torch.zeros((planes, plan.n, plan.n), dtype=torch.float32, device=windows.device)
    kept = {}
    for t0, t1 in chunks:
        specs = _window_spectra(windows[t0:t1], plan, eps, N)
        if keep:
            kept[t0] = specs
        raw = _socs.hopkinsIntensityBatch(specs, socs, N, tileChunk=t1 - t0)
        if gain != 1.0:
            raw *= gain
        tiles = postProcess(raw.reshape(-1, pn, pn), eps).reshape(t1 - t0, planes, nt, nt)
        stitchTiles(tiles, place[t0:t1], plan.j0, plan.core, image)
    return image, kept


def _tile_chunks(who, tileChunk, socs, plan):
    from . import socs as _socs
    if tileChunk is None:
        tileChunk = max(1, _socs.STACK_BYTES // (socs.planes * (socs.K * 8 + 4) * plan.pixelNumber ** 2))
    tileChunk = int(tileChunk)
    if tileChunk < 1:
        raise ValueError(f"{who}: tileChunk must be >= 1; got {tileChunk}")
    return [(t0, min(plan.count, t0 + tileChunk)) for t0 in range(0, plan.count, tileChunk)]


def maskImageTiled(transmission, socs, plan: TilePlan, background=0, normalize=False, tileChunk=None):
    """The stitched Hopkins image of a PIXEL mask on the plan's raster lattice: `transmission` complex or real [ny core, nx core],
    cut into the plan's windows (`background` outside the plane) and imaged as optimizeMaskTiled's forward sweep images them.
    fp32 [n,n] (or [planes,n,n] for the kernels of a pupil stack), the grid of hopkinsImageTiled(...).image."""
    import torch

    from . import socs as _socs
    from .imageformation import ShapeError
    if not isinstance(socs, _socs.SOCSKernels):
        raise TypeError("maskImageTiled: socs must be the SOCSKernels socsKernels returned")
    if not isinstance(plan, TilePlan):
        raise TypeError("maskImageTiled: plan must be the TilePlan planTiles returned")
    rows, cols = plan.ny * plan.core, plan.nx * plan.core
    if not isinstance(transmission, torch.Tensor) or tuple(transmission.shape) != (rows, cols) or plan.pixelNumber != socs.pn:
        raise ShapeError(f"maskImageTiled: transmission must be [{rows},{cols}] and the kernels {plan.pixelNumber} x {plan.pixelNumber}; "
                         f"got {tuple(getattr(transmission, 'shape', ()))} and {socs.pn}")
    dev = nat.require_gpu(socs.kernels.device)
    place = torch.from_numpy(plan.place).to(dev)
    windows = cutTiles(transmission.detach().to(device=dev, dtype=torch.complex64), place, plan.pixelNumber, plan.halo, background)
    gain = 1.0 / float(socs.weight_sum) if normalize and socs.weight_sum > 0 else 1.0
    image, _ = _image_windows(windows, socs, plan, place, gain, _tile_chunks("maskImageTiled", tileChunk, socs, plan))
    return image if socs.stacked else image[0]


def optimizeMaskTiled(target, socs, plan: TilePlan, threshold, dose=1.0, iterations=20, step=0.25, maskSteepness=4.0,
                      resistSteepness=None, background=0, feature=1, initial=None, normalize=True, tileChunk=None):
    """ilt.optimizeMask for a layout block larger than one window: ONE theta, fp32 [ny core, nx core] on the plan's raster lattice
    (exactly the cores), one loss on the stitched image, and the exact gradient of the tiled forward model.

    Per iterate: t = background + (feature - background) sigmoid(maskSteepness theta); the windows are cut from t with their halos
    (cutTiles, `background` outside the plane); per chunk of `tileChunk` windows (None: what keeps the batched workspaces under
    socs.STACK_BYTES) their spectra, ONE hopkinsIntensityBatch, the normalisation, ONE postProcess with the windows as planes, ONE
    stitch.  The loss is _descent.resist_loss on image[:, :ny core, :nx core] -- the covered region: the empty part of the square
    image of a non-square plan carries no loss.  `target`: real [n,n] or [planes,n,n] on the stitched grid, the grid of
    hopkinsImageTiled(...).image.  Backwards: unstitchTiles, postProcessAdjoint, the normalisation, ONE hopkinsGradientBatch per
    chunk, maskSpectrumAdjoint per window, overlapAddTiles -- a window's halo pixels carry gradient into the neighbouring cores --
    then the theta chain and the peak-normalised step of optimizeMask.  The loss is read on the host once per iterate.  The
    spectra are kept from the forward sweep when all of them fit under socs.STACK_BYTES and recomputed chunk by chunk otherwise;
    neither that nor `tileChunk` changes a bit.  theta starts at +-1 from the target where the two grids share samples, or from
    `initial` (real [ny core, nx core]).  Returns an ILTResult (theta, transmission, mask on the global lattice) with `.plan`.
    See the module's caveat on pixel sizes with epsilon != 1."""
    import torch

    from . import _descent
    from . import socs as _socs
    from .ilt import ILTResult, hopkinsGradientBatch, maskSpectrumAdjoint, postProcessAdjoint
    from .imageformation import ShapeError
    who = "optimizeMaskTiled"
    if not isinstance(socs, _socs.SOCSKernels):
        raise TypeError(f"{who}: socs must be the SOCSKernels socsKernels returned")
    if not isinstance(plan, TilePlan):
        raise TypeError(f"{who}: plan must be the TilePlan planTiles returned")
    iterations = int(iterations)
    if resistSteepness is None:
        resistSteepness = _descent.default_resist_steepness(threshold)
    if iterations < 1 or not float(step) > 0 or not float(maskSteepness) > 0 or not float(resistSteepness) > 0:
        raise ValueError(f"{who}: iterations >= 1 and step, maskSteepness, resistSteepness > 0; got {iterations}, {step}, "
                         f"{maskSteepness}, {resistSteepness}")
    if complex(feature) == complex(background):
        raise ValueError(f"{who}: feature and background transmissions are equal; nothing to optimise")
    pn, planes = int(socs.pn), socs.planes
    if plan.pixelNumber != pn:
        raise ShapeError(f"{who}: the kernels are {pn} x {pn}, the plan's windows {plan.pixelNumber}")
    dev = nat.require_gpu(socs.kernels.device)
    n, nt, core, halo, T = plan.n, plan.n_tile, plan.core, plan.halo, plan.count
    rows, cols = plan.ny * core, plan.nx * core
    want = ((planes, n, n), (n, n)) if socs.stacked else ((n, n),)
    if not isinstance(target, torch.Tensor) or target.is_complex() or tuple(target.shape) not in want:
        raise ShapeError(f"{who}: target must be a real tensor of shape {' or '.join(map(str, want))}, the stitched image's grid; got "
                         f"{tuple(getattr(target, 'shape', ()))}")
    target = target.detach().to(device=dev, dtype=torch.float32)
    covered = target[..., :rows, :cols]
    if initial is not None:
        if not isinstance(initial, torch.Tensor) or tuple(initial.shape) != (rows, cols) or initial.is_complex():
            raise ShapeError(f"{who}: initial must be a real [{rows},{cols}] tensor; got {tuple(getattr(initial, 'shape', ()))}")
        theta = initial.detach().to(device=dev, dtype=torch.float32).clone()
    else:
        first = covered if covered.dim() == 2 else covered[0]                      # the two grids share their first sample
        theta = torch.where(first > 0.5, 1.0, -1.0).to(torch.float32)
    chunks = _tile_chunks(who, tileChunk, socs, plan)
    eps, N = nat.epsilon_n(4.0 / pn, plan.pixelSize, plan.wavelength)
    gain = 1.0 / float(socs.weight_sum) if normalize and socs.weight_sum > 0 else 1.0
    keep = T * pn * pn * 8 <= _socs.STACK_BYTES
    place = torch.from_numpy(plan.place).to(dev)
    bg, span = complex(background), complex(feature) - complex(background)
    a_m, a_r, dose, threshold = float(maskSteepness), float(resistSteepness), float(dose), float(threshold)

    def transmission_of(th):
        return (bg + span * torch.sigmoid(a_m * th)).to(torch.complex64)

    losses, best, best_theta = [], 0, theta.clone()
    for it in range(iterations + 1):
        s = torch.sigmoid(a_m * theta)
        windows = cutTiles((bg + span * s).to(torch.complex64), place, pn, halo, bg)
        image, kept = _image_windows(windows, socs, plan, place, gain, chunks, keep)
        loss, grad_cov = _descent.resist_loss(image[:, :rows, :cols], covered, a_r, dose, threshold, gradient=it < iterations)
        losses.append(float(loss))                                                 # the one host read of this iterate
        if losses[-1] < losses[best]:
            best, best_theta = it, theta.clone()
        if it == iterations or not math.isfinite(losses[-1]):
            break
        grad_image = torch.zeros((planes, n, n), dtype=torch.float32, device=dev)
        grad_image[:, :rows, :cols] = grad_cov
        grad_windows = torch.empty((T, pn, pn), dtype=torch.complex64, device=dev)
        for t0, t1 in chunks:
            specs = kept[t0] if keep else _window_spectra(windows[t0:t1], plan, eps, N)
            gtiles = unstitchTiles(grad_image, place[t0:t1], nt, plan.j0, core)
            # window by window: the same launches whatever the chunk, so the chunking changes no bit
            graw = torch.stack([postProcessAdjoint(gtiles[b], pn, eps) for b in range(t1 - t0)])
            if gain != 1.0:
                graw *= gain
            g = hopkinsGradientBatch(specs, socs, N, graw if socs.stacked else graw[:, 0], tileChunk=t1 - t0)
            for b in range(t1 - t0):
                grad_windows[t0 + b] = maskSpectrumAdjoint(g[b], pn, eps, N)
        grad_t = overlapAddTiles(grad_windows, place, halo, rows, cols)           # dl/dRe t + i dl/dIm t on the global lattice
        grad_theta = a_m * s * (1.0 - s) * (grad_t * span.conjugate()).real
        theta = theta - float(step) * grad_theta / _descent.peak(grad_theta, torch.float32)
    result = ILTResult(best_theta, transmission_of(best_theta), losses, best)
    result.plan = plan
    return result


# ---- tiled optical proximity correction ------------------------------------------------------------------------------------------
MEEF_MATRIX_BYTES = 2 << 30               # ceiling of the dense S x S float64 MEEF matrix of correctLayoutTiled(step="meef")


def _check_tiled_socs(who, socs, plan):
    from . import socs as _socs
    if not isinstance(socs, _socs.SOCSKernels):
        raise TypeError(f"{who}: socs must be a SOCSKernels (socsKernels / vectorSocsKernels)")
    if socs.pn != plan.pixelNumber or socs.stacked:
        raise ValueError(f"{who}: the kernels are {'a stack of ' if socs.stacked else ''}{socs.pn} x {socs.pn}, the windows "
                         f"{plan.pixelNumber} x {plan.pixelNumber}: one plane on the window's grid is needed")


def _opc_bounds(polygons, maxBias, searchRange, pixelSize):
    """The polygons' bounding box grown on every side by maxBias + (searchRange + 2) pixels: every biased polygon and every site's
    search segment (searchRange pixels along the normal, bilinear samples one pixel further) then lies in covered image."""
    polys, boxes = _bounding_boxes(polygons)
    if not polys:
        raise ValueError("correctLayoutTiled: the layout has no polygon")
    m = float(maxBias) + (float(searchRange) + 2.0) * float(pixelSize)
    return (boxes[:, 0].min() - m, boxes[:, 1].min() - m, boxes[:, 2].max() + m, boxes[:, 3].max() + m)


def _tiled_model(who, socs, plan, sites, threshold, antialias, searchRange, normalize, tileChunk):
    """(imager, epe) of correctLayoutTiled: imager(polygons) -> the stitched image fp32 [n,n] by hopkinsImageTiled's sweep,
    epe(image) -> EPE in nm per site (plane 0, dose 1; NaN where nothing crosses) by ONE measureEPE."""
    import torch

    from .metrology import measureEPE
    chunks = _tile_chunks(who, tileChunk, socs, plan)
    dev = nat.require_gpu(socs.kernels.device)
    divide = float(socs.weight_sum) if normalize and socs.weight_sum > 0 else None
    site_rows = torch.from_numpy(sites.sites_px).to(dev)

    def imager(polys):
        return _sweep_layout(polys, socs, plan, antialias, divide, chunks, dev)[0]

    def epe(image):
        return measureEPE(image, threshold, site_rows, plan.pixelSize, searchRange=searchRange)[0, 0, :, 0].cpu().numpy()

    return imager, epe


def correctLayoutTiled(polygons, socs, pixelNumber, pixelSize, wavelength, threshold, *, spacing, maxBias, halo=None, bounds=None,
                       origin=None, iterations=6, gain=0.6, antialias=16, searchRange=8.0, step="damped", normalize=False,
                       tileChunk=None, exposed=True):
    """metrology.correctLayout for a Manhattan layout block larger than one window: the fragments of ALL polygons move on one
    stitched image.  `socs` the SOCSKernels at `pixelNumber` (one plane), `halo` in pixels (None: pixelNumber / 4), `bounds` =
    (x0, y0, x1, y1) the rectangle to image -- None: the polygons' bounding box grown on every side by maxBias + (searchRange + 2)
    * pixelSize, so that every biased polygon and every site's search segment lies in covered image --, `origin` the pixel
    lattice's (planTiles).  The sites are layoutSites of the target on the stitched grid and stay fixed.

    Per iterate: biasLayout, tileEdgeIndex and ONE upload; per chunk of `tileChunk` windows ONE raster launch
    (rasterizeCoverageTiles), the window spectra, ONE hopkinsIntensityBatch, ONE postProcess with the windows as planes, ONE stitch
    -- hopkinsImageTiled's own sweep, so the image of an iterate IS hopkinsImageTiled's of the biased layout on the same plan, bit
    for bit --; then ONE measureEPE on the stitched image.  The two update rules are correctLayout's (`step` "damped" or "meef",
    `gain`, `maxBias`); step="meef" takes its frozen matrix from epeJacobianTiled, the exact Jacobian of this tiled model, dense
    [S,S] float64 on the host (ValueError where that would exceed 2 GiB: raise `spacing`).  The result depends on neither
    `tileChunk` nor the chunking of the Jacobian's directions, bit for bit.  Returns an OPCResult with `.plan`.  ValueError before
    any image is made: a non-Manhattan layout, a stacked or wrong-size `socs`, exposed=False, an unknown `step`."""
    from .metrology import _counter_clockwise, _damped_loop, _meef_loop, biasLayout
    who = "correctLayoutTiled"
    if step not in ("damped", "meef"):
        raise ValueError(f"{who}: step must be 'damped' or 'meef'; got {step!r}")
    if not exposed:
        raise ValueError(f"{who}: the loop is defined for exposed features (the polygons are the mask's openings and print bright)")
    iterations, gain, maxBias = int(iterations), float(gain), float(maxBias)
    if iterations < 1 or not maxBias >= 0.0 or not math.isfinite(maxBias) or not math.isfinite(gain):
        raise ValueError(f"{who}: iterations >= 1, finite gain and maxBias >= 0; got {iterations}, {gain}, {maxBias}")
    if not 0.0 < float(searchRange) <= 32.0:
        raise ValueError(f"{who}: searchRange must lie in (0, 32] pixels; got {searchRange}")
    pn, ps = int(pixelNumber), float(pixelSize)
    target = _counter_clockwise(polygons)
    if bounds is None:
        bounds = _opc_bounds(target, maxBias, searchRange, ps)
    plan = planTiles(bounds, pn, ps, wavelength, pn // 4 if halo is None else halo, origin)
    _check_tiled_socs(who, socs, plan)
    sites = layoutSites(target, spacing, ps, plan.origin, pn, wavelength, registration=plan.registration)
    if len(sites) == 0:
        raise ValueError(f"{who}: the layout has no edges")
    biasLayout(target, sites, np.zeros(len(sites)))            # raises for a non-Manhattan layout before any image is made
    if step == "meef" and len(sites) ** 2 * 8 > MEEF_MATRIX_BYTES:
        raise ValueError(f"{who}: {len(sites)} sites make a dense MEEF matrix of {len(sites) ** 2 * 8 / 2 ** 30:.1f} GiB, more than "
                         f"{MEEF_MATRIX_BYTES >> 30} GiB; raise spacing (now {spacing}) or use step='damped'")
    imager, epe = _tiled_model(who, socs, plan, sites, threshold, antialias, searchRange, normalize, tileChunk)
    if step == "meef":
        def sensitivity(polys, b):
            return epeJacobianTiled(target, sites, b, socs, plan, threshold, antialias=antialias, searchRange=searchRange,
                                    normalize=normalize, tileChunk=tileChunk)[1]
        result = _meef_loop(target, sites, imager, epe, sensitivity, iterations, maxBias)
    else:
        result = _damped_loop(target, sites, imager, epe, iterations, gain, maxBias)
    result.plan = plan
    return result


def _global_fragment_cells(sites, bias, plan):
    """sensitivity._fragment_cells once on the lattice of ALL windows, halo included: (rows, cols, fragment, weight) with (row, col)
    counted from the first window's corner, so that window (ix, iy) holds the cells [iy core, iy core + pn) x [ix core, ix core + pn)
    at (row - iy core, col - ix core)."""
    from .sensitivity import _fragment_cells
    side = plan.core * max(plan.nx, plan.ny) + 2 * plan.halo
    corner = (plan.origin[0] - plan.halo * plan.pixelSize, plan.origin[1] - plan.halo * plan.pixelSize)
    return _fragment_cells(sites, bias, side, plan.pixelSize, corner)


def epeJacobianTiled(polygons, sites, bias_nm, socs, plan: TilePlan, threshold, *, antialias=16, searchRange=8.0, directions=None,
                     normalize=False, tileChunk=None, directionChunk=None, cull=True):
    """(epe_nm [S], J [S,P]) of the TILED forward model at biasLayout(polygons, sites, bias_nm), float64 on the host: the EPE at
    `sites` (layoutSites on the stitched grid of `plan`; NaN where nothing crosses in range) on the stitched image of
    correctLayoutTiled, and its exact derivative along `directions` [P,S] of the fragment biases (None: the identity, the MEEF
    matrix).  For direction p: the coverage tangent of window w is edgeCoverageTangentHost's at the window's origin (the cells are
    found once on the lattice of all windows, halo included, and sliced per window); the image tangent of w is
    postProcessTangent(hopkinsTangent(M_w, socs, N, spectrum of that tangent)), divided as the image is when `normalize`; the
    stitched tangent holds the cores of those and zero in every core whose window holds no cell of a moving fragment; J[:, p] =
    measureEPETangent(stitched image, stitched tangent).  A fragment in one window's halo moves edges in the neighbouring core:
    the matrix is NOT block diagonal by tile.  Windows a direction cannot reach are skipped -- their tangent is exactly zero --,
    `cull=False` evaluates every window for every direction and gives the same bits.  Directions go in chunks of at most 16
    (`directionChunk`), lowered until the stitched tangents stay under socs.STACK_BYTES, windows in tile order; neither that nor
    `tileChunk` (the primal sweep's) changes a bit.  A row of J is NaN where the site's EPE is."""
    import torch

    from . import socs as _socs
    from .mask import Mask
    from .metrology import _counter_clockwise, biasLayout, measureEPE
    from .sensitivity import MAX_DIRECTIONS, hopkinsTangent, measureEPETangent, postProcessTangent
    who = "epeJacobianTiled"
    if not isinstance(plan, TilePlan):
        raise TypeError(f"{who}: plan must be the TilePlan planTiles returned")
    _check_tiled_socs(who, socs, plan)
    if not isinstance(sites, LayoutSites):
        raise TypeError(f"{who}: sites must be a LayoutSites (layoutSites on the plan's stitched grid)")
    S = len(sites)
    bias = np.asarray(bias_nm, dtype=np.float64).reshape(-1)
    d = np.eye(S) if directions is None else np.asarray(directions, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != S or d.shape[0] < 1 or not np.isfinite(d).all():
        raise ValueError(f"{who}: directions must be finite [P,{S}]; got {d.shape}")
    if bias.shape[0] != S or not np.isfinite(bias).all():
        raise ValueError(f"{who}: {S} finite biases are needed; got {bias.shape[0]}")
    P = int(d.shape[0])
    size = MAX_DIRECTIONS if directionChunk is None else int(directionChunk)
    if not 1 <= size <= MAX_DIRECTIONS:
        raise ValueError(f"{who}: directionChunk must lie in 1..{MAX_DIRECTIONS}; got {directionChunk}")
    pn, ps, core, n, j0 = plan.pixelNumber, plan.pixelSize, plan.core, plan.n, plan.j0
    while size > 1 and size * n * n * 4 > _socs.STACK_BYTES:
        size -= 1
    target = _counter_clockwise(polygons)
    dev = nat.require_gpu(socs.kernels.device)
    eps, N = nat.epsilon_n(4.0 / pn, ps, float(plan.wavelength))
    divide = float(socs.weight_sum) if normalize and socs.weight_sum > 0 else None
    chunks = _tile_chunks(who, tileChunk, socs, plan)
    polys = biasLayout(target, sites, bias)
    rows, cols, frag, wts = _global_fragment_cells(sites, bias, plan)
    keep = plan.count * pn * pn * 8 <= _socs.STACK_BYTES
    spectra = {} if keep else None
    image = _sweep_layout(polys, socs, plan, antialias, divide, chunks, dev, spectra=spectra)[0]
    arrays = None if keep else _upload_tile_index(who, polys, plan, True, dev)

    def spectrum_of(w):
        if keep:
            return spectra[w]
        return _window_spectra(_raster_tiles(arrays, plan, antialias, w, w + 1), plan, eps, N)[0]

    site_rows = torch.from_numpy(sites.sites_px).to(dev)
    epe = measureEPE(image, threshold, site_rows, ps, searchRange=searchRange)[0, 0, :, 0].double().cpu().numpy()
    # the cells of every window: window (ix, iy) holds the global cells [iy core, iy core + pn) x [ix core, ix core + pn)
    inside = []
    for w in range(plan.count):
        r0, c0 = int(plan.place[w, 0]), int(plan.place[w, 1])
        inside.append(np.nonzero((rows >= r0) & (rows < r0 + pn) & (cols >= c0) & (cols < c0 + pn))[0])
    J = np.empty((S, P))
    for p0 in range(0, P, size):
        dd = d[p0:p0 + size]
        k = dd.shape[0]
        stitched = torch.zeros((k, n, n), dtype=torch.float32, device=dev)
        for w in range(plan.count):
            cells = inside[w]
            moving = dd[:, frag[cells]] != 0.0                                     # [k, cells of w]
            reach = np.nonzero(moving.any(axis=1))[0] if cull else np.arange(k)
            if reach.size == 0:
                continue
            r0, c0 = int(plan.place[w, 0]), int(plan.place[w, 1])
            dt = np.zeros((reach.size, pn, pn), dtype=np.float64)
            for a, p in enumerate(reach):
                np.add.at(dt[a], (rows[cells] - r0, cols[cells] - c0), dd[p, frag[cells]] * wts[cells])
            dts = torch.from_numpy(dt.astype(np.float32)).to(dev)
            dM = torch.stack([Mask(pixelSize=ps, device=dev, transmission=t)._ffFraunhofer(eps, N) for t in dts])
            draw = hopkinsTangent(spectrum_of(w), socs, N, dM)
            if divide is not None:
                draw /= divide
            for a, p in enumerate(reach):                                          # one direction a call: the batch cannot show
                tile = postProcessTangent(draw[a], pn, eps)
                stitched[int(p), r0:r0 + core, c0:c0 + core] = tile[j0:j0 + core, j0:j0 + core]
        dE = measureEPETangent(image, stitched, threshold, site_rows, ps, searchRange=searchRange)[:, 0, 0, :]
        J[:, p0:p0 + k] = dE.double().cpu().numpy().T
    return epe, J
