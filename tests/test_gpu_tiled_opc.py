"""Tiled OPC on the GPU (`-m gpu`): litho_rasterize_coverage_tiles bit for bit against the per-window entry and the CPU restatement
(tests/coverage_oracle.py), hopkinsImageTiled through it against its own per-window route, and correctLayoutTiled /
epeJacobianTiled against tests/tiled_opc_oracle.py and central differences of the device's own tiled primal.

Rasteriser shapes (pn, s): (16, 1) a line shorter than a wave, (16, 4) pn s = 64, (20, 2), (33, 4) ragged, (64, 16), (256, 16) one
whole scan step, (2048, 16) with one tile: 32768 sub-columns, the 128 KiB LDS line (dynamic-LDS opt-in) and eight scan steps.  Tiles
1, 3 and 7; from three tiles on the last window lies where no polygon is (an empty tile)."""
import functools

import numpy as np
import pytest
import torch

import coverage_oracle as CO
import test_gpu_resist_memory as RM

pytestmark = pytest.mark.gpu

dev, L, nat, side = RM.dev, RM.L, RM.nat, RM.side                                 # the fixtures
PIXEL = 5.0                                                                        # q = 5 / s is a dyadic number for every s
RASTER_SHAPES = [(16, 1), (16, 4), (20, 2), (33, 4), (64, 16), (256, 16)]
TILE_COUNTS = [1, 3, 7]


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def raster_plan(pn, pixel, windows):
    """A TilePlan by hand, for the rasteriser alone: it reads windows_nm, pixelNumber, pixelSize and the tile count."""
    from lithographysimulator_amd.tiling import TilePlan
    w = np.ascontiguousarray(windows, dtype=np.float64).reshape(-1, 2)
    T = w.shape[0]
    return TilePlan(pn, float(pixel), 193.0, 0, pn, 0, T, 1, pn * T, pn, (0.0, 0.0), (0.0, 0.0, 1.0, 1.0), 0.0, w,
                    np.zeros((T, 2), dtype=np.int32), np.full((T, 2), -1, dtype=np.int32))


def windows_of(pn, T):
    """T windows in a row, stepping by 5/8 of a window (they overlap, as windows with halos do); from three on, the last one far
    above the layout: an empty tile."""
    span = pn * PIXEL
    w = np.array([[0.625 * span * t, 0.0] for t in range(T)])
    if T >= 3:
        w[-1] = (0.0, 10.0 * span)
    return w


@functools.lru_cache(maxsize=None)
def layout_of(pn, s, T):
    """Per window: a rectangle straddling the next window's left border and one the bottom border, a rectangle overlapping the
    first (they must union), a slanted triangle (every other one clockwise), a polygon with its vertices ON sub-centres and one on
    sub-grid lines (the half-open rule; all coordinates on the q / 2 lattice); the restatement's random layout over window 0."""
    span, q = pn * PIXEL, PIXEL / s
    polys = list(CO.random_layout(7 * pn + s, pn, PIXEL, s))
    m = pn * s
    for t in range(T):
        x = 0.625 * span * t
        polys.append(rect(x + 0.55 * span, 0.10 * span, x + 0.80 * span, 0.45 * span))
        polys.append(rect(x + 0.70 * span, 0.30 * span, x + 0.95 * span, 0.60 * span))
        polys.append(rect(x + 0.05 * span, -0.10 * span, x + 0.30 * span, 0.15 * span))
        tri = np.array([[x + 0.10 * span, 0.50 * span], [x + 0.50 * span, 0.62 * span], [x + 0.22 * span, 0.93 * span]])
        polys.append(tri[::-1] if t % 2 else tri)
        a, b = max(1, m // 7), max(3, m // 3)
        polys.append(rect(x + (a + 0.5) * q, 0.7 * span + 0.5 * q, x + (b + 0.5) * q, 0.7 * span + (b - a + 0.5) * q))
        polys.append(np.array([[x + a * q, 0.2 * span], [x + b * q, 0.2 * span], [x + (a + b) // 2 * q, 0.2 * span + a * q]]))
    return tuple(polys)


def culled(polys, pn, window):
    """The polygons whose bounding box overlaps the window, strictly: hopkinsImageTiled's test, by a plain loop."""
    span = pn * PIXEL
    wx, wy = float(window[0]), float(window[1])
    return [p for p in polys
            if p[:, 0].max() > wx and p[:, 0].min() < wx + span and p[:, 1].max() > wy and p[:, 1].min() < wy + span]


def per_window(L, dev, polys, pn, s, window, orient=True):
    """rasterizeLayout of the culled polygons at the window's origin, as float32 (antialias 1 gives int16)."""
    got = L.rasterizeLayout(culled(polys, pn, window), pn, PIXEL, origin=(float(window[0]), float(window[1])), device=dev, antialias=s,
                            orient=orient)
    return got.to(torch.float32)


# ---- 1. the rasteriser, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TILE_COUNTS)
@pytest.mark.parametrize("pn,s", RASTER_SHAPES)
def test_tiles_equal_the_per_window_entry_and_the_restatement(L, dev, pn, s, T):
    from lithographysimulator_amd import layout as LY
    polys, windows = list(layout_of(pn, s, T)), windows_of(pn, T)
    plan = raster_plan(pn, PIXEL, windows)
    got = L.rasterizeLayoutTiles(polys, plan, antialias=s, device=dev)
    assert got.dtype == torch.float32 and tuple(got.shape) == (T, pn, pn) and got.device.type == "cuda"
    oracle_tiles = range(T) if pn * s <= 1024 else (0, T - 1)
    grey = 0
    for t in range(T):
        want = per_window(L, dev, polys, pn, s, windows[t])
        differ = int((got[t] != want).sum())
        line = f"tiles {T}, window {t} at {pn}^2 s={s}: {differ} pixels differ from rasterizeLayout"
        assert differ == 0, line
        if t in oracle_tiles:
            counts = CO.coverage_counts(LY.polygonEdges(culled(polys, pn, windows[t])), pn, windows[t][0], windows[t][1], PIXEL, s)
            mine = got[t].cpu().numpy().astype(np.float64) * (s * s)
            off = int((mine != counts).sum())
            line += f", {off} from the restatement ({int(counts.sum())} of {pn * pn * s * s} sub-centres inside)"
            assert off == 0, line
            grey += int(((counts > 0) & (counts < s * s)).sum())
        print(line)
    assert s == 1 or grey > 0
    if T >= 3:
        assert not bool(got[T - 1].any()) and bool(got[0].any())                  # the empty tile, and a tile that is not
    if s == 1:
        assert bool(((got == 0.0) | (got == 1.0)).all())


def test_the_lds_limit_2048_by_16(L, dev):
    """pn s = 32768: the 128 KiB line, eight scan steps.  Against the per-window entry everywhere; against the restatement on the
    last 64 x 64 pixels (every coordinate is dyadic, so a shifted origin is the same arithmetic)."""
    from lithographysimulator_amd import layout as LY
    pn, s = 2048, 16
    span = pn * PIXEL
    polys = [rect(0.1 * span, 0.2 * span, 0.4 * span, 0.3 * span), rect(-0.5 * span, 0.6 * span, 1.5 * span, 0.7 * span),
             np.array([[0.2 * span, 0.1 * span], [0.9 * span, 0.5 * span], [0.3 * span, 0.95 * span]]),
             rect(span - 40.3125, span - 70.0, span + 100.0, span - 9.6875),
             np.array([[span - 300.0, span - 310.0], [span - 5.0, span - 200.0], [span - 150.0, span + 50.0]])[::-1]]
    plan = raster_plan(pn, PIXEL, [[0.0, 0.0]])
    got = L.rasterizeLayoutTiles(polys, plan, antialias=s, device=dev)
    want = per_window(L, dev, polys, pn, s, (0.0, 0.0))
    differ = int((got[0] != want).sum())
    corner = (pn - 64) * PIXEL
    counts = CO.coverage_counts(LY.polygonEdges(polys), 64, corner, corner, PIXEL, s)
    mine = got[0, pn - 64:, pn - 64:].cpu().numpy().astype(np.float64) * (s * s)
    off = int((mine != counts).sum())
    print(f"2048^2 s=16: {differ} pixels differ from rasterizeLayout, {off} of the last 64 x 64 from the restatement; "
          f"covered {float(got.mean()):.4f}, {int(((counts > 0) & (counts < 256)).sum())} grey pixels in the corner")
    assert differ == 0 and off == 0 and 0.0 < float(got.mean()) < 1.0 and ((counts > 0) & (counts < 256)).any()


@pytest.mark.parametrize("pn,s", [(33, 4), (64, 16)])
def test_a_covering_polygon_and_a_clockwise_hole(L, dev, pn, s):
    """One polygon covers window 1 and more: the winding of its pixels comes only from edges outside the window.  With orient=False
    a clockwise polygon inside it is a hole; with orient=True it is made counter-clockwise and vanishes in the union."""
    span = pn * PIXEL
    windows = windows_of(pn, 3)
    x = windows[1][0]
    cover = rect(x - 0.3 * span, -0.4 * span, x + 1.2 * span, 1.3 * span)
    hole = rect(x + 0.31 * span, 0.22 * span, x + 0.74 * span, 0.58 * span)[::-1]
    polys = [cover, hole]
    plan = raster_plan(pn, PIXEL, windows)
    for orient in (True, False):
        got = L.rasterizeLayoutTiles(polys, plan, antialias=s, device=dev, orient=orient)
        for t in range(3):
            assert torch.equal(got[t], per_window(L, dev, polys, pn, s, windows[t], orient=orient)), (orient, t)
        inside = float(got[1].mean())
        print(f"{pn}^2 s={s} orient={orient}: window 1 covered {inside:.4f}, window 0 {float(got[0].mean()):.4f}, window 2 (empty) "
              f"{float(got[2].mean()):.4f}")
        assert (inside == 1.0) if orient else (0.8 < inside < 0.9)
        assert not bool(got[2].any()) and 0.0 < float(got[0].mean()) < 1.0


def test_a_tiles_bits_are_its_own(L, dev):
    """The tile alone, the tiles permuted, and chunks tiles=(t0, t1) give the bits of the whole call."""
    pn, s, T = 33, 4, 7
    polys, windows = list(layout_of(pn, s, T)), windows_of(pn, T)
    whole = L.rasterizeLayoutTiles(polys, raster_plan(pn, PIXEL, windows), antialias=s, device=dev)
    for t in range(T):
        alone = L.rasterizeLayoutTiles(polys, raster_plan(pn, PIXEL, windows[t:t + 1]), antialias=s, device=dev)
        assert torch.equal(alone[0], whole[t]), t
    perm = np.array([4, 0, 6, 2, 5, 1, 3])
    mixed = L.rasterizeLayoutTiles(polys, raster_plan(pn, PIXEL, windows[perm]), antialias=s, device=dev)
    assert torch.equal(mixed, whole[torch.from_numpy(perm).to(dev)])
    plan = raster_plan(pn, PIXEL, windows)
    for t0, t1 in ((0, 1), (0, 3), (3, 7), (6, 7), (2, 5)):
        part = L.rasterizeLayoutTiles(polys, plan, antialias=s, device=dev, tiles=(t0, t1))
        assert tuple(part.shape) == (t1 - t0, pn, pn) and torch.equal(part, whole[t0:t1]), (t0, t1)
    for bad in ((0, 0), (3, 2), (-1, 2), (0, 8)):
        with pytest.raises(ValueError):
            L.rasterizeLayoutTiles(polys, plan, antialias=s, device=dev, tiles=bad)
    print(f"{pn}^2 s={s}, {T} tiles: alone, permuted and in five chunks -- the same bits")


def test_bad_edge_numbers_non_finite_edges_and_origins_are_skipped(L, dev):
    """The device arrays guard themselves: edge numbers outside [0, E) and non-finite edges change nothing, offsets are clamped to
    the index (a descending pair is an empty list), a window with a non-finite origin is zeros."""
    from lithographysimulator_amd import layout as LY
    from lithographysimulator_amd import tiling as TL
    pn, s, T = 33, 4, 3
    polys, windows = list(layout_of(pn, s, T)), windows_of(pn, T)
    plan = raster_plan(pn, PIXEL, windows)
    whole = L.rasterizeLayoutTiles(polys, plan, antialias=s, device=dev)
    edges, offsets, index = TL.tileEdgeIndex(polys, plan)
    E = edges.shape[0]
    span = pn * PIXEL
    bad_edges = np.array([[np.inf, 0.0, 0.3 * span, 0.5 * span], [0.1 * span, -np.inf, 0.1 * span, 0.4 * span],
                          [np.nan, 0.0, 0.2 * span, 0.9 * span], [0.2 * span, np.nan, 0.5 * span, 0.3 * span]])
    edges2 = np.concatenate([edges, bad_edges])
    # per tile: the list, then the non-finite edges and four numbers that are no edge
    junk = np.array([E, E + 1, E + 2, E + 3, -1, E + 4, 2 ** 31 - 1, -2 ** 31], dtype=np.int32)
    parts, offs = [], [0]
    for t in range(T):
        parts += [index[offsets[t]:offsets[t + 1]], junk]
        offs.append(offs[-1] + int(offsets[t + 1] - offsets[t]) + len(junk))
    index2 = np.concatenate(parts).astype(np.int32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = LY.rasterizeCoverageTiles(to(edges2), to(np.array(offs, dtype=np.int64)), to(index2), to(windows), pn, PIXEL, s)
    assert torch.equal(got, whole)
    # offsets past the index, in front of it and descending; a NaN and an infinite origin
    M = index.shape[0]
    wild = np.array([-5, offsets[1], offsets[1] - 3, M + 1000], dtype=np.int64)      # tile 0: [0, o1); tile 1: empty; tile 2: [o1 - 3, M)
    w2 = windows.copy()
    got = LY.rasterizeCoverageTiles(to(edges), to(wild), to(index), to(w2), pn, PIXEL, s)
    assert torch.equal(got[0], whole[0]) and not bool(got[1].any())
    w2[0, 0], w2[1, 1] = np.nan, np.inf
    got = LY.rasterizeCoverageTiles(to(edges), to(offsets), to(index), to(w2), pn, PIXEL, s)
    assert not bool(got[0].any()) and not bool(got[1].any()) and torch.equal(got[2], whole[2])
    print(f"{pn}^2 s={s}: {len(junk)} bad edge numbers per tile, {len(bad_edges)} non-finite edges, wild offsets and two non-finite "
          "origins: the other tiles keep their bits")


def raster_case(L, nat, dev, pn, s, T):
    from lithographysimulator_amd import tiling as TL
    polys, windows = list(layout_of(pn, s, T)), windows_of(pn, T)
    plan = raster_plan(pn, PIXEL, windows)
    edges, offsets, index = TL.tileEdgeIndex(polys, plan)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    want = RM.memo(("raster tiles", pn, s, T), lambda: L.rasterizeLayoutTiles(polys, plan, antialias=s, device=dev))

    def call(p, st):
        return nat.lib().litho_rasterize_coverage_tiles(p["edges"], edges.shape[0], p["offsets"], p["index"], index.shape[0], p["windows"],
                                                        T, pn, PIXEL, s, p["coverage"], st)
    return RM.Case("litho_rasterize_coverage_tiles", (pn, s), f"{T} tiles, {edges.shape[0]} edges, {index.shape[0]} listed",
                   [("edges", to(edges)), ("offsets", to(offsets)), ("index", to(index)), ("windows", to(windows))], {"coverage": want}, call,
                   RM.guard_bytes(pn), mod=8)


@pytest.mark.parametrize("pn,s,T", [(33, 4, 3), (16, 1, 1), (64, 16, 3)])
def test_where_the_rasteriser_reads_and_writes(L, nat, dev, pn, s, T):
    """In the guarded, poisoned arena: every output element written, no guard or input byte changed, every buffer 8 bytes past a
    16-byte boundary in turn, twice."""
    RM.run(nat, dev, raster_case(L, nat, dev, pn, s, T))


def test_the_rasteriser_on_a_side_stream(L, nat, dev, side):
    RM.run(nat, dev, raster_case(L, nat, dev, 33, 4, 3), side)


def test_more_candidate_edges_than_the_lds_list_holds(L, dev):
    """700 thin slits cross every pixel row: 1400 candidate edges, past the 1024 the compacted list holds -- the direct walk."""
    pn, s = 64, 4
    span = pn * PIXEL
    step = span / 700.0
    polys = [rect(i * step, -10.0, i * step + 0.5 * step, span + 10.0) for i in range(700)] + [rect(0.2 * span, 0.3 * span, 0.5 * span, 0.6 * span)]
    windows = np.array([[0.0, 0.0], [0.5 * span, 0.25 * span]])
    got = L.rasterizeLayoutTiles(polys, raster_plan(pn, PIXEL, windows), antialias=s, device=dev)
    for t in range(2):
        assert torch.equal(got[t], per_window(L, dev, polys, pn, s, windows[t])), t
    print(f"{pn}^2 s={s}: {2 * len(polys)} vertical edges per pixel row, covered {float(got[0].mean()):.4f} and {float(got[1].mean()):.4f}")
    assert 0.5 < float(got[0].mean()) < 0.7


# ---- the 2 x 2 block shared with tests/test_tiled_opc_cpu.py -----------------------------------------------------------------------
import epe_oracle as EO                                                            # noqa: E402
import tiled_opc_oracle as TP                                                      # noqa: E402


class Block:
    pass


@pytest.fixture(scope="module")
def blk(L, dev):
    """The plan, the device's SOCS kernels (all 8 of an 8-point source), the target, its sites, the threshold and the CPU model."""
    from lithographysimulator_amd.metrology import _counter_clockwise
    b = Block()
    b.plan = L.planTiles(TP.BOUNDS, TP.PN, TP.PIXEL, TP.WL, TP.HALO, TP.ORIGIN)
    kernels, W, _ = TP.kernels_of()
    b.pupil = L.Pupil(TP.PN, TP.WL, TP.NA, None, dev).generatePupilFunction()
    b.source = W.to(dev)
    b.socs = L.socsKernels(b.pupil, b.source, kernels=TP.SOURCE_POINTS)
    assert b.socs.K == TP.SOURCE_POINTS and not b.socs.stacked
    b.model = TP.TiledModel(b.plan, kernels)
    b.target = _counter_clockwise(TP.block_layout())
    b.sites = L.layoutSites(b.target, TP.SPACING, TP.PIXEL, b.plan.origin, TP.PN, TP.WL, registration=b.plan.registration)
    b.threshold = 0.3 * float(b.model.image([TP.rect_px(-100, -100, 200, 200)]).max())
    b.kw = dict(spacing=TP.SPACING, maxBias=TP.MAX_BIAS, halo=TP.HALO, bounds=TP.BOUNDS, origin=TP.ORIGIN, searchRange=TP.RANGE)
    b.args = (b.target, b.socs, TP.PN, TP.PIXEL, TP.WL, b.threshold)
    b.first = L.correctLayoutTiled(*b.args, iterations=1, **b.kw)
    return b


def model_of(L, b, tileChunk=None):
    from lithographysimulator_amd import tiling
    return tiling._tiled_model("test", b.socs, b.plan, b.sites, b.threshold, 16, TP.RANGE, False, tileChunk)


# ---- 2. the imager -----------------------------------------------------------------------------------------------------------------
def test_the_imager_is_hopkins_image_tiled(L, dev, blk):
    tiled = L.hopkinsImageTiled(blk.target, blk.socs, TP.PN, TP.PIXEL, TP.WL, bounds=TP.BOUNDS, halo=TP.HALO, antialias=16, origin=TP.ORIGIN)
    imager, _ = model_of(L, blk)
    image = imager(L.biasLayout(blk.target, blk.sites, np.zeros(len(blk.sites))))
    assert tuple(image.shape) == (blk.plan.n, blk.plan.n) and torch.equal(image, tiled.image)
    one, _ = model_of(L, blk, tileChunk=1)
    assert torch.equal(one(blk.target), image)
    want = blk.model.image(blk.target)
    err = float(np.abs(image.cpu().numpy() - want).max() / want.max())
    print(f"imager at zero bias == hopkinsImageTiled, bit for bit (tileChunk 1 too); against the restatement {err:.2e} of the maximum; "
          f"seamError {tiled.seamError:.3e}")
    assert err < 2e-5                                                               # helpers.TOL_IMAGE_MAX: the image bound of the suite


@pytest.mark.parametrize("antialias", [1, 8])
def test_hopkins_image_tiled_equals_its_per_window_route(L, dev, blk, antialias):
    """The route hopkinsImageTiled took before the batched rasteriser, restated: rasterizeLayout(origin=window) and Mask.fraunhofer
    window by window (antialias 1: the binary mask's spectrum), one batch, one post-process, one stitch, one seam measure."""
    from lithographysimulator_amd import tiling
    from lithographysimulator_amd import _native as nat
    plan, socs = blk.plan, blk.socs
    polys = list(blk.target) + [TP.rect_px(30.3, 30.6, 33.1, 33.4), TP.rect_px(-20, 55, 90, 58.7)]        # off the lattice, across all four tiles
    got = L.hopkinsImageTiled(polys, socs, TP.PN, TP.PIXEL, TP.WL, bounds=TP.BOUNDS, halo=TP.HALO, antialias=antialias, origin=TP.ORIGIN,
                              tileChunk=3)
    eps, N = nat.epsilon_n(4.0 / TP.PN, TP.PIXEL, TP.WL)
    specs = []
    for t in range(plan.count):
        raster = L.rasterizeLayout(TP.culled(polys, plan, t), TP.PN, TP.PIXEL, origin=tuple(plan.windows_nm[t]), device=dev, antialias=antialias)
        mask = L.Mask(transmission=raster, pixelSize=TP.PIXEL, device=dev) if antialias > 1 else L.Mask(raster, TP.PIXEL, dev)
        specs.append(mask.fraunhofer(TP.WL, True))
    raw = L.hopkinsIntensityBatch(torch.stack(specs), socs, N)
    tiles = L.postProcess(raw.reshape(-1, TP.PN, TP.PN), eps).reshape(plan.count, 1, plan.n_tile, plan.n_tile)
    image = tiling.stitchTiles(tiles, torch.from_numpy(plan.place).to(dev), plan.j0, plan.core,
                               torch.zeros((1, plan.n, plan.n), dtype=torch.float32, device=dev))[0]
    seam = tiling.seamTiles(tiles, torch.from_numpy(plan.neighbours).to(dev), plan.j0, plan.core)
    finite = seam[~torch.isnan(seam)]
    print(f"antialias {antialias}: image max {float(image.max()):.4e}, seamError {got.seamError:.3e}")
    assert torch.equal(got.image, image)
    assert torch.equal(torch.nan_to_num(got.seam, nan=-1.0), torch.nan_to_num(seam, nan=-1.0))
    assert got.seamError == float(finite.max()) / float(image.max())


# ---- 3. the first iterate's EPE ----------------------------------------------------------------------------------------------------
def test_first_iterate_epe(L, dev, blk):
    """Exactly measureEPE of hopkinsImageTiled's image at TiledImage.sites; and the restatement's EPE of THAT image within
    2^-22 (|t_k| + h cond) pixel, test_gpu_epe.py's bound (the image error does not enter)."""
    tiled = L.hopkinsImageTiled(blk.target, blk.socs, TP.PN, TP.PIXEL, TP.WL, bounds=TP.BOUNDS, halo=TP.HALO, antialias=16, origin=TP.ORIGIN)
    sites = tiled.sites(blk.target, TP.SPACING)
    assert np.array_equal(sites.sites_px, blk.sites.sites_px)
    got = L.measureEPE(tiled.image, blk.threshold, sites, TP.PIXEL, searchRange=TP.RANGE)[0, 0].double().cpu().numpy()
    first = blk.first
    assert first.plan.count == 4 and len(first.history) == 1 and np.array_equal(first.epe_history[0], got[:, 0], equal_nan=True)
    table, cond = EO.measure_epe(tiled.image.cpu().numpy(), sites.sites_px, [1.0], blk.threshold, True, TP.RANGE, TP.PIXEL)
    fin = ~np.isnan(table[0, 0, :, 0])
    assert np.array_equal(np.isnan(got[:, 0]), ~fin) and np.array_equal(got[fin, 2], table[0, 0, fin, 2]) and fin.sum() >= 0.9 * len(sites)
    tol = 2.0 ** -22 * (np.abs(table[0, 0, :, 2]) + 0.5 * cond[0, 0]) * TP.PIXEL
    d = np.abs(got[:, 0] - table[0, 0, :, 0])[fin]
    print(f"{len(sites)} sites, {int(fin.sum())} found; RMS EPE {TP.rms(got[:, 0]):.4f} nm; max |epe - restatement| {d.max():.2e} nm, "
          f"{float((d / tol[fin]).max()):.3f} of its bound")
    assert (d <= tol[fin]).all()


# ---- 4. one window -----------------------------------------------------------------------------------------------------------------
def test_one_window_plan_against_correct_layout(L, dev, blk):
    """A plan of ONE tile images one window: correctLayout(model="socs") at that window's origin sees the same raster and the same
    kernels.  Its sites are the same points in window pixels, x_w = x_s + j0, each rounded to fp32 on its own: the two site rows
    differ by at most one ulp of the largest coordinate, delta = 2^-18 pixel below 64.  A site moved by (ex, ey) moves the crossing by
    -(grad I . e) / (grad I . n): at most 2 G delta h / |u_b - u_a| sample steps with G the largest difference of neighbouring
    pixels (the bilinear image's slope), plus twice measureEPE's own rounding 2^-22 (|t_k| + h cond) -- both in pixels."""
    ps, pn, halo = TP.PIXEL, TP.PN, TP.HALO
    polys = [TP.rect_px(7, 7, 12, 25), TP.rect_px(18, 8, 25, 14), TP.rect_px(17, 19, 25, 24)]          # >= range + 2 = 6 pixels inside the core [0, 32)
    bounds = (0.0, 0.0, 31 * ps, 31 * ps)
    kw = dict(spacing=TP.SPACING, maxBias=TP.MAX_BIAS, searchRange=TP.RANGE, iterations=1)
    tiled = L.correctLayoutTiled(polys, blk.socs, pn, ps, TP.WL, blk.threshold, halo=halo, bounds=bounds, origin=TP.ORIGIN, **kw)
    plan = tiled.plan
    assert plan.count == 1 and plan.core == 32
    single = L.correctLayout(polys, pn, ps, tuple(plan.windows_nm[0]), TP.WL, blk.pupil, blk.source, blk.threshold, model="socs", socs=blk.socs,
                             **kw)
    a, b = tiled.epe_history[0], single.epe_history[0]
    assert len(a) == len(b) and np.array_equal(np.isnan(a), np.isnan(b)) and not np.isnan(a).any()
    moved = np.abs(single.sites.sites_px[:, :2].astype(np.float64) - plan.j0 - tiled.sites.sites_px[:, :2].astype(np.float64)).max()
    delta = float(np.spacing(np.float32(single.sites.sites_px[:, :2].max())))
    image = L.hopkinsImageTiled(polys, blk.socs, pn, ps, TP.WL, bounds=bounds, halo=halo, antialias=16, origin=TP.ORIGIN).image.cpu().numpy()
    table, cond = EO.measure_epe(image, tiled.sites.sites_px, [1.0], blk.threshold, True, TP.RANGE, ps)
    G = max(float(np.abs(np.diff(image, axis=0)).max()), float(np.abs(np.diff(image, axis=1)).max()))
    den = table[0, 0, :, 1] * (0.5 * ps) * float(np.float32(blk.threshold))                  # |u_b - u_a| from the log-slope
    bound = ps * (2 * G * delta * 0.5 / den + 2 * 2.0 ** -22 * (np.abs(table[0, 0, :, 2]) + 0.5 * cond[0, 0]))
    d = np.abs(a - b)
    print(f"{len(a)} sites; site rows differ by {moved:.2e} pixel (ulp of the largest coordinate {delta:.2e}); first-iterate EPE differs by "
          f"at most {d.max():.2e} nm, {float((d / bound).max()):.3f} of its bound (smallest bound {bound.min():.2e} nm); RMS {TP.rms(a):.3f} nm")
    assert moved <= delta and (d <= bound).all() and bound.max() < 1e-2


# ---- 5. the Jacobian ---------------------------------------------------------------------------------------------------------------
def pick_columns(sites):
    mid = sites.xy_nm / TP.PIXEL
    find = lambda x, y: int(np.argmin(np.abs(mid[:, 0] - x) + np.abs(mid[:, 1] - y)))       # noqa: E731
    return [find(12, 12), find(9, 32), find(34, 34)]                                        # deep in a core, across a boundary, at the corner


def fields_image(L, dev, b, polys):
    """The stitched image from the code the tangent runs on: sum_k |hopkinsFields|^2 per window (float64 sum), for the repeatability."""
    from lithographysimulator_amd import _native as nat
    from lithographysimulator_amd import tiling
    plan = b.plan
    eps, N = nat.epsilon_n(4.0 / TP.PN, plan.pixelSize, TP.WL)
    cov = L.rasterizeLayoutTiles(polys, plan, antialias=16, device=dev)
    raws = []
    for t in range(plan.count):
        E = L.hopkinsFields(L.Mask(transmission=cov[t], pixelSize=plan.pixelSize, device=dev).fraunhofer(TP.WL, True), b.socs, N)
        raws.append((E.real.double() ** 2 + E.imag.double() ** 2).sum(dim=0).float())
    tiles = L.postProcess(torch.stack(raws), eps).reshape(plan.count, 1, plan.n_tile, plan.n_tile)
    return tiling.stitchTiles(tiles, torch.from_numpy(plan.place).to(dev), plan.j0, plan.core,
                              torch.zeros((1, plan.n, plan.n), dtype=torch.float32, device=dev))[0]


def jacobian_case(L, dev, b, pixel_tag):
    """|J - FD(d/2)| <= |FD(d) - FD(d/2)| + 2 rho / d at d = pixel / 8 for three columns, on the sites that keep their interval (at
    least 90 %); rho the largest change of an EPE between the sweep's image and the one of the line transforms the tangent runs on."""
    imager, epe_of = model_of(L, b)
    S = len(b.sites)
    zero = np.zeros(S)
    rows = torch.from_numpy(b.sites.sites_px).to(dev)

    def measure(image):
        e = L.measureEPE(image, b.threshold, rows, b.plan.pixelSize, searchRange=TP.RANGE)[0, 0].double().cpu().numpy()
        return e[:, 0], np.nan_to_num(e[:, 2], nan=-99.0)

    e0, tk0 = measure(imager(b.target))
    e1, _ = measure(fields_image(L, dev, b, b.target))
    rho = float(np.nanmax(np.abs(e0 - e1)))
    d = b.plan.pixelSize / 8
    cols = pick_columns(b.sites) if pixel_tag == "193/8" else [0, S // 2, S - 1]
    dirs = np.zeros((3, S))
    dirs[np.arange(3), cols] = 1.0
    epe, J = L.epeJacobianTiled(b.target, b.sites, zero, b.socs, b.plan, b.threshold, searchRange=TP.RANGE, directions=dirs)
    assert np.array_equal(epe, e0, equal_nan=True) and J.shape == (S, 3)
    print(f"{pixel_tag} nm: {S} sites; repeatability between the two images' EPE {rho:.2e} nm")

    def fd(direction, step):
        up, dn = (measure(imager(L.biasLayout(b.target, b.sites, sgn * step * direction))) for sgn in (1.0, -1.0))
        return (up[0] - dn[0]) / (2 * step), (up[1] == tk0) & (dn[1] == tk0)

    for j, col in enumerate(cols):
        (f1, s1), (f2, s2) = fd(dirs[j], d), fd(dirs[j], d / 2)
        keep = s1 & s2 & ~np.isnan(J[:, j])
        err, bound = np.abs(J[:, j] - f2)[keep], np.abs(f1 - f2)[keep] + 2 * rho / d
        print(f"column {col}: J[{col},{col}] = {J[col, j]:.4f}; {int(keep.sum())} of {S} sites keep their interval; max |J - FD(d/2)| "
              f"{err.max():.2e}, its bound {bound[np.argmax(err)]:.2e}")
        assert keep.sum() >= 0.9 * S and (err <= bound).all() and abs(J[col, j]) > 0.3
    return cols, dirs, J, e0, (fd, rho, d)


def test_jacobian_against_differences_of_the_tiled_primal(L, dev, blk):
    cols, dirs, J, e0, (fd, rho, d) = jacobian_case(L, dev, blk, "193/8")
    S = len(blk.sites)
    zero = np.zeros(S)
    assert np.array_equal(e0, blk.first.epe_history[0], equal_nan=True)                     # the loop's first-iterate EPE, exactly
    # a cross-tile entry: the corner fragment (tile 1's core) and the site in another tile's core it moves most
    home = blk.model.home_tile(blk.sites)
    other = home != home[cols[2]]
    i = int(np.nanargmax(np.abs(np.where(other, J[:, 2], 0.0))))
    (f1, s1), (f2, s2) = fd(dirs[2], d), fd(dirs[2], d / 2)
    want = blk.model.jacobian(blk.target, blk.sites, zero, blk.threshold, directions=dirs)[1]
    print(f"cross-tile entry J[{i},{cols[2]}] = {J[i, 2]:.5f} (site in tile {home[i]}, fragment in tile {home[cols[2]]}); FD(d/2) {f2[i]:.5f}, "
          f"the restatement {want[i, 2]:.5f}; largest |J - restatement| {np.nanmax(np.abs(J - want)):.2e}")
    assert J[i, 2] != 0.0 and abs(J[i, 2]) > 1e-3 and s1[i] and s2[i]
    assert abs(J[i, 2] - f2[i]) <= abs(f1[i] - f2[i]) + 2 * rho / d
    # culled == brute force; the direction chunk and tileChunk change no bit
    kw = dict(searchRange=TP.RANGE, directions=dirs)
    args = (blk.target, blk.sites, zero, blk.socs, blk.plan, blk.threshold)
    brute = L.epeJacobianTiled(*args, cull=False, **kw)[1]
    assert np.array_equal(J, brute, equal_nan=True)
    for chunk in (1, 3, 16):
        assert np.array_equal(J, L.epeJacobianTiled(*args, directionChunk=chunk, **kw)[1], equal_nan=True), chunk
    assert np.array_equal(J, L.epeJacobianTiled(*args, tileChunk=1, **kw)[1], equal_nan=True)
    # the fragment deep in tile 0's core reaches window 0 alone: sites whose search segment lies in another core see an exact zero
    far = (home == 3) & ~np.isnan(J[:, 0])
    assert far.any() and (J[far, 0] == 0.0).all()


def test_jacobian_at_25_nm(L, dev):
    """epsilon != 1: both resamplings are bilinear and the post-process tangent is a matrix product."""
    from lithographysimulator_amd.metrology import _counter_clockwise
    b = Block()
    ps = 25.0
    q = ps / 16
    b.plan = L.planTiles((0.0, 0.0, 55 * ps, 55 * ps), TP.PN, ps, TP.WL, 18, (-5 * q, -3 * q))
    assert (b.plan.nx, b.plan.ny, b.plan.core) == (2, 2, 28)
    _, W, _ = TP.kernels_of()
    pupil = L.Pupil(TP.PN, TP.WL, TP.NA, None, dev).generatePupilFunction()
    b.socs = L.socsKernels(pupil, W.to(dev), kernels=TP.SOURCE_POINTS)
    b.target = _counter_clockwise([TP.rect_px(9, 10, 15, 42, ps), TP.rect_px(21, 9, 27, 33, ps), TP.rect_px(20, 39, 44, 45, ps),
                                   TP.rect_px(32, 20, 38, 34, ps)])
    b.sites = L.layoutSites(b.target, 8 * ps, ps, b.plan.origin, TP.PN, TP.WL, registration=b.plan.registration)
    clear = L.hopkinsImageTiled([TP.rect_px(-100, -100, 200, 200, ps)], b.socs, TP.PN, ps, TP.WL, bounds=(0.0, 0.0, 55 * ps, 55 * ps), halo=18,
                                origin=(-5 * q, -3 * q))
    b.threshold = 0.3 * float(clear.image.max())
    jacobian_case(L, dev, b, "25")


# ---- 6. the loop -------------------------------------------------------------------------------------------------------------------
def test_both_steps_lower_the_epe_and_meef_is_no_worse(L, dev, blk):
    damped = L.correctLayoutTiled(*blk.args, iterations=4, **blk.kw)
    meef = L.correctLayoutTiled(*blk.args, iterations=4, step="meef", **blk.kw)
    print("damped history (rms nm, max nm, lost):", [(round(a, 4), round(b, 4), c) for a, b, c in damped.history])
    print("meef   history (rms nm, max nm, lost):", [(round(a, 4), round(b, 4), c) for a, b, c in meef.history])
    best = lambda r: (r.history[r.best_iteration][2], r.history[r.best_iteration][0])       # noqa: E731
    assert damped.history[0] == meef.history[0] == blk.first.history[0]
    assert best(damped) < (damped.history[0][2], damped.history[0][0]) and best(meef) < (meef.history[0][2], meef.history[0][0])
    assert best(meef) <= best(damped)
    for step, whole in (("damped", damped), ("meef", meef)):
        one = L.correctLayoutTiled(*blk.args, iterations=4, step=step, tileChunk=1, **blk.kw)
        assert one.history == whole.history and one.best_iteration == whole.best_iteration and np.array_equal(one.bias_nm, whole.bias_nm)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(one.epe_history, whole.epe_history))
    S = len(blk.sites)
    J = L.epeJacobianTiled(blk.target, blk.sites, np.zeros(S), blk.socs, blk.plan, blk.threshold, searchRange=TP.RANGE)[1]
    assert damped.jacobian is None and meef.jacobian.shape == (S, S) and np.array_equal(meef.jacobian, J, equal_nan=True)
    cols = pick_columns(blk.sites)
    three = np.zeros((3, S))
    three[np.arange(3), cols] = 1.0
    part = L.epeJacobianTiled(blk.target, blk.sites, np.zeros(S), blk.socs, blk.plan, blk.threshold, searchRange=TP.RANGE, directions=three)[1]
    assert np.array_equal(J[:, cols], part, equal_nan=True)                                 # the matrix of test 5
    assert meef.plan.count == 4 and len(meef.polygons) == len(blk.target)
