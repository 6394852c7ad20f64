"""Times the batched window rasteriser and one tiled OPC iterate on one MI355X, warm, in one process:

    timeout -k 10 900 python scripts/tiled_opc_time.py [--rounds 5] [--kernels 24]

Rasteriser: litho_rasterize_coverage_tiles (rasterizeCoverageTiles on edges and an index already on the device) per window at 128^2,
256^2 and 1024^2 windows, s = 8 and 16, B = 1 / 8 / 64 windows of the 96-polygon block of examples/tiled_layout.py, against a loop of
rasterizeLayout over the same windows -- the route every window took before: a host edge list and an upload per window, then
litho_rasterize_coverage's clear, edge and fill kernels per band.  The two are timed alternately, `rounds` times each, every timing
window between two device synchronises and long enough to last about 0.2 s; the median and the spread (min ... max) of the per-window
time are printed, and the two routes are compared bit for bit first.

Iterate: one correctLayoutTiled iterate on four 128^2 windows (halo 32, 193 / 8 nm, antialias 16) broken into host bias and index,
raster, spectra, image, post-process plus stitch, and EPE, each between synchronises; and one epeJacobianTiled per fragment.
First measurements of an untuned path; the figures go into LABNOTES.md."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import lithographysimulator_amd as L                                     # noqa: E402
from lithographysimulator_amd import _native as nat                      # noqa: E402
from lithographysimulator_amd import layout as LY                        # noqa: E402
from lithographysimulator_amd import tiling                              # noqa: E402
from tiled_layout import cell                                            # noqa: E402
from tiling_time import alternate, show, window                          # noqa: E402

WL, NA, PS = 193.0, 0.7, 193.0 / 8.0


def block(pn, blocks):
    size = pn * PS / 2.0
    return [q for j in range(blocks) for i in range(blocks) for q in cell(i * size, j * size, size, i + 2 * j)], blocks * size


def windows_plan(pn, count, extent):
    """`count` windows of pn^2 pixels over the block, stepping by half a window and wrapping row by row."""
    per_row = max(1, int(extent / (pn * PS / 2.0)))
    w = np.array([[(t % per_row) * pn * PS / 2.0 - pn * PS / 4.0, ((t // per_row) % per_row) * pn * PS / 2.0 - pn * PS / 4.0]
                  for t in range(count)])
    return tiling.TilePlan(pn, PS, WL, 0, pn, 0, count, 1, pn * count, pn, (0.0, 0.0), (0.0, 0.0, 1.0, 1.0), 0.0, w,
                           np.zeros((count, 2), dtype=np.int32), np.full((count, 2), -1, dtype=np.int32))


def raster_timing(dev, a):
    for pn in a.sizes:
        polys, extent = block(pn, 4)
        span = pn * PS
        for s in a.levels:
            for B in a.batches:
                plan = windows_plan(pn, B, extent)
                arrays = tiling._upload_tile_index("timing", polys, plan, True, dev)
                culled = [[p for p in polys if p[:, 0].max() > wx and p[:, 0].min() < wx + span and p[:, 1].max() > wy and p[:, 1].min() < wy + span]
                          for wx, wy in plan.windows_nm.tolist()]

                def batched():
                    return tiling._raster_tiles(arrays, plan, s, 0, B)

                def loop():
                    return [LY.rasterizeLayout(culled[t], pn, PS, origin=tuple(plan.windows_nm[t]), device=dev, antialias=s) for t in range(B)]

                same = all(torch.equal(x, y) for x, y in zip(batched(), loop()))
                tb, tl = alternate(batched, loop, a.rounds)
                ratio = statistics.median(tl) / statistics.median(tb)
                listed = int(arrays[2].shape[0])
                print(f"pn {pn:4d} s {s:2d} B {B:2d} ({listed / B:.0f} edges listed per window; bits equal: {same}): per window, batched "
                      f"{show(tb, B)}, loop of rasterizeLayout {show(tl, B)}; loop / batched {ratio:.2f}", flush=True)


def iterate_timing(dev, a):
    pn, halo = 128, 32
    polys, extent = block(pn, 2)                                          # 24 polygons on one window's width: 2 x 2 cores of 64
    source = L.LightSource(0.4, 0.8, pn, NA, device=dev).generateAnnular()
    pupil = L.Pupil(pn, WL, NA, None, dev).generatePupilFunction()
    socs = L.socsKernels(pupil, source, kernels=a.kernels)
    plan = L.planTiles((0.0, 0.0, extent - 1.0, extent - 1.0), pn, PS, WL, halo)
    target = L.metrology._counter_clockwise(polys)
    sites = L.layoutSites(target, 8 * PS, PS, plan.origin, pn, WL, registration=plan.registration)
    S, T = len(sites), plan.count
    bias = np.random.default_rng(0).uniform(-6.0, 6.0, S)
    eps, N = nat.epsilon_n(4.0 / pn, PS, WL)
    open_mask = L.Mask(torch.ones((pn, pn), dtype=torch.int16), PS, dev)
    threshold = 0.3 * float(L.hopkinsIntensity(open_mask.fraunhofer(WL, True), socs, N)[pn // 2, pn // 2])
    place = torch.from_numpy(plan.place).to(dev)
    rows = torch.from_numpy(sites.sites_px).to(dev)
    image = torch.zeros((1, plan.n, plan.n), dtype=torch.float32, device=dev)
    state = {}

    def host():
        state["polys"] = L.biasLayout(target, sites, bias)
        state["arrays"] = tiling._upload_tile_index("timing", state["polys"], plan, True, dev)

    def raster():
        state["cov"] = tiling._raster_tiles(state["arrays"], plan, 16, 0, T)

    def spectra():
        state["specs"] = tiling._window_spectra(state["cov"], plan, eps, N)

    def imaging():
        state["raw"] = L.hopkinsIntensityBatch(state["specs"], socs, N, tileChunk=T)

    def post():
        tiles = L.postProcess(state["raw"].reshape(-1, pn, pn), eps).reshape(T, 1, plan.n_tile, plan.n_tile)
        tiling.stitchTiles(tiles, place, plan.j0, plan.core, image)

    def epe():
        state["epe"] = L.measureEPE(image[0], threshold, rows, PS, searchRange=8.0)[0, 0, :, 0].cpu().numpy()

    steps = [("host bias and index (with the upload)", host), ("raster, one launch", raster), ("spectra, window by window", spectra),
             ("image, one batch", imaging), ("post-process plus stitch", post), ("EPE with its read-back", epe)]
    for _, fn in steps:
        fn()
    print(f"one iterate: {T} windows of {pn}^2, halo {halo}, K {socs.K}, {len(polys)} polygons, {S} sites", flush=True)
    total = 0.0
    for name, fn in steps:
        ts = [window(fn, 20) for _ in range(a.rounds)]
        total += statistics.median(ts)
        print(f"  {name}: {show(ts, 1)}", flush=True)
    print(f"  sum of the medians {total:.3f} ms", flush=True)
    zero = np.zeros(S)
    L.epeJacobianTiled(target, sites, zero, socs, plan, threshold, directions=np.eye(S)[:16])
    ts = []
    for _ in range(max(2, a.rounds // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, J = L.epeJacobianTiled(target, sites, zero, socs, plan, threshold)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    print(f"  epeJacobianTiled, {S} fragments: {show(ts, 1)}; per fragment {statistics.median(ts) / S:.3f} ms", flush=True)
    assert np.isfinite(J[~np.isnan(J)]).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels", type=int, default=24)
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 256, 1024])
    ap.add_argument("--levels", type=int, nargs="*", default=[8, 16])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 64])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda", 0)
    raster_timing(dev, a)
    iterate_timing(dev, a)


if __name__ == "__main__":
    main()
