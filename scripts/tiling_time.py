"""Times the batched Hopkins image and the tiling kernels on one MI355X, warm, in one process:

    timeout -k 10 900 python scripts/tiling_time.py [--rounds 5] [--kernels 32]

hopkinsIntensityBatch at 256^2 and 1024^2 tiles (K = 32, annular 0.4-0.8 source, ideal pupil, 25 nm pixels at 193 nm) for B = 1, 8
and 64 mask spectra against a loop of hopkinsIntensity over the same spectra -- the route every image took before the batch entry
existed.  The two are timed alternately, `rounds` times each, every window ending in a device synchronise and holding enough
calls to last about 0.2 s; the median and the spread (min ... max) of the per-tile time are printed.  Before timing, the batch is
compared with the loop on the same spectra (they are two routes to one image: equal to rounding, not bit for bit).

Stitch and seam: 64 tiles of 1024^2 with halo 128 (two planes), bytes over time against 4.1 TB/s -- the stitch reads and writes
count planes core^2 floats, the seam reads two lines of `core` floats from each of two tiles per (tile, plane, side).
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
import lithographysimulator_amd as L                                     # noqa: E402
from lithographysimulator_amd import tiling                              # noqa: E402

PEAK = 4.1e12


def window(fn, calls):
    """ms per call of `calls` calls between two synchronises."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def calls_for(fn, target_ms=200.0):
    fn()
    fn()
    one = window(fn, 3)
    return max(3, int(target_ms / max(one, 1e-3)))


def alternate(a, b, rounds):
    """(times of a, times of b) in ms per call, the two timed in turn."""
    na, nb = calls_for(a), calls_for(b)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(a, na))
        tb.append(window(b, nb))
    return ta, tb


def show(ts, per):
    return f"{statistics.median(ts) / per:.4f} ms ({min(ts) / per:.4f} ... {max(ts) / per:.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 64])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda", 0)
    wl, na, ps = 193.0, 0.7, 25.0
    for pn in a.sizes:
        source = L.LightSource(0.4, 0.8, pn, na, device=dev).generateAnnular()
        pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
        socs = L.socsKernels(pupil, source, kernels=a.kernels)
        _, N = L.Mask(torch.zeros((pn, pn), dtype=torch.int16), ps, dev).calculateEpsilonN(4.0 / pn, ps, wl)
        gen = torch.Generator().manual_seed(pn)
        B = max(a.batches)
        specs = torch.stack([L.Mask((torch.rand((pn, pn), generator=gen) < 0.3).to(torch.int16), ps, dev).fraunhofer(wl, True)
                             for _ in range(B)])
        batch = L.hopkinsIntensityBatch(specs[:2], socs, N)
        loop = torch.stack([L.hopkinsIntensity(specs[b], socs, N) for b in range(2)])
        gap = float((batch.double() - loop.double()).abs().max() / loop.double().max())
        print(f"pn {pn} N {N} K {socs.K} (captured {socs.captured:.4f}): batch vs loop of hopkinsIntensity {gap:.2e} of the image's "
              f"maximum", flush=True)
        for nb in a.batches:
            m = specs[:nb]
            tb, tl = alternate(lambda: L.hopkinsIntensityBatch(m, socs, N),
                               lambda: [L.hopkinsIntensity(m[b], socs, N) for b in range(nb)], a.rounds)
            ratio = statistics.median(tl) / statistics.median(tb)
            print(f"  B {nb:2d}: per tile, batch {show(tb, nb)}, loop {show(tl, nb)}; loop / batch {ratio:.2f}", flush=True)
    # stitch and seam
    pn, halo, count, planes = 1024, 128, 64, 2
    core = pn - 2 * halo
    nx = 8
    n = core * nx
    tiles = torch.rand((count, planes, pn, pn), dtype=torch.float32, device=dev)
    place = torch.tensor([((t // nx) * core, (t % nx) * core) for t in range(count)], dtype=torch.int32, device=dev)
    nbr = torch.tensor([(t + 1 if (t + 1) % nx else -1, t + nx if t + nx < count else -1) for t in range(count)], dtype=torch.int32,
                       device=dev)
    image = torch.zeros((planes, n, n), dtype=torch.float32, device=dev)
    ts, tm = alternate(lambda: tiling.stitchTiles(tiles, place, halo, core, image), lambda: tiling.seamTiles(tiles, nbr, halo, core),
                       a.rounds)
    sb = 2 * count * planes * core * core * 4
    pairs = int((nbr.cpu().numpy() >= 0).sum()) * planes
    mb = pairs * 4 * core * 4
    print(f"litho_tiles_stitch {count} tiles x {planes} planes, core {core}: {show(ts, 1)}; {sb / 1e9:.3f} GB moved, "
          f"{sb / (statistics.median(ts) * 1e-3) / 1e12:.2f} TB/s = {100 * sb / (statistics.median(ts) * 1e-3) / PEAK:.0f} % of 4.1 TB/s",
          flush=True)
    print(f"litho_tiles_seam {pairs} (pair, plane)s, core {core}: {show(tm, 1)}; {mb / 1e6:.2f} MB read, "
          f"{mb / (statistics.median(tm) * 1e-3) / 1e9:.1f} GB/s (half of the lines are strided columns: a line of the right seam "
          f"costs one 64-byte fetch per sample pair)", flush=True)
    assert np.isfinite(statistics.median(ts))


if __name__ == "__main__":
    main()
