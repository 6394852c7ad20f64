"""Times the batched mask gradient, the three tiling kernels of the tiled inverse-lithography loop and one whole iterate of
optimizeMaskTiled on one MI355X, warm, in one process:

    timeout -k 10 900 python scripts/tiled_ilt_time.py [--rounds 5] [--kernels 32]

hopkinsGradientBatch at 256^2 and 1024^2 tiles (K = 32, annular 0.4-0.8 source, ideal pupil, 25 nm pixels at 193 nm) for B = 1, 8
and 64 mask spectra (at 1024^2 the batches whose workspace stays under socs.STACK_BYTES per call are one call, larger ones are
chunked by the wrapper) against a loop of hopkinsGradient over the same spectra -- the route every window gradient would take
without the batch entry.  The two are timed alternately, `rounds` times each, every window ending in a device synchronise and
holding enough calls to last about 0.2 s; the median and the spread (min ... max) of the per-tile time are printed.  Before
timing, the batch is compared with the loop on the same spectra (two orders of transforms: equal to rounding, not bit for bit).

Cut, overlap-add and unstitch: 64 windows of 1024^2 with halo 128 (two planes for the unstitch), bytes over time against
4.1 TB/s.  One iterate: optimizeMaskTiled with iterations = 1 (two forward sweeps, one backward) on 4 x 4 windows of 256^2, halo
64, 193 / 8 nm pixels, host time between synchronises.
First measurements of an untuned path; the figures go into LABNOTES.md."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import lithographysimulator_amd as L                                     # noqa: E402
from lithographysimulator_amd import tiling                              # noqa: E402
from tiling_time import PEAK, alternate, calls_for, show, window          # noqa: E402


def rate(nbytes, ts):
    t = statistics.median(ts) * 1e-3
    return f"{nbytes / 1e9:.3f} GB moved, {nbytes / t / 1e12:.2f} TB/s = {100 * nbytes / t / PEAK:.0f} % of 4.1 TB/s"


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
        G = torch.randn((B, pn, pn), generator=gen, dtype=torch.float32).to(dev)
        batch = L.hopkinsGradientBatch(specs[:2], socs, N, G[:2])
        loop = torch.stack([L.hopkinsGradient(specs[b], socs, N, G[b]) for b in range(2)])
        gap = float((batch - loop).abs().max() / loop.abs().max())
        per_tile = (socs.K * 8 + 4) * pn * pn
        print(f"pn {pn} N {N} K {socs.K} (captured {socs.captured:.4f}): batch vs loop of hopkinsGradient {gap:.2e} of the gradient's "
              f"maximum; workspace {per_tile / 2 ** 20:.0f} MiB per tile", flush=True)
        for nb in a.batches:
            m, g = specs[:nb], G[:nb]
            tb, tl = alternate(lambda: L.hopkinsGradientBatch(m, socs, N, g),
                               lambda: [L.hopkinsGradient(m[b], socs, N, g[b]) for b in range(nb)], a.rounds)
            ratio = statistics.median(tl) / statistics.median(tb)
            print(f"  B {nb:2d}: per tile, batch {show(tb, nb)}, loop {show(tl, nb)}; loop / batch {ratio:.2f}", flush=True)
        del specs, G
    # cut, overlap-add, unstitch
    pn, halo, nx, planes = 1024, 128, 8, 2
    core, count = pn - 2 * halo, nx * nx
    rows = cols = core * nx
    place = torch.tensor([((t // nx) * core, (t % nx) * core) for t in range(count)], dtype=torch.int32, device=dev)
    plane = torch.view_as_complex(torch.rand((rows, cols, 2), dtype=torch.float32, device=dev))
    windows = tiling.cutTiles(plane, place, pn, halo)
    image = torch.rand((planes, rows, rows), dtype=torch.float32, device=dev)
    tc, to = alternate(lambda: tiling.cutTiles(plane, place, pn, halo), lambda: tiling.overlapAddTiles(windows, place, halo, rows, cols),
                       a.rounds)
    nu = calls_for(lambda: tiling.unstitchTiles(image, place, pn, halo, core))
    tu = [window(lambda: tiling.unstitchTiles(image, place, pn, halo, core), nu) for _ in range(a.rounds)]
    wb = count * pn * pn * 8
    print(f"litho_tiles_cut {count} windows of {pn}^2, halo {halo}: {show(tc, 1)}; {rate(wb + rows * cols * 8, tc)} (the plane read once, the windows "
          f"written; the allocation of the windows is inside the time)", flush=True)
    print(f"litho_tiles_overlap_add the same windows into {rows} x {cols}: {show(to, 1)}; {rate(wb + rows * cols * 8, to)}", flush=True)
    ub = count * planes * (pn * pn + core * core) * 4
    print(f"litho_tiles_unstitch {count} tiles x {planes} planes: {show(tu, 1)}; {rate(ub, tu)}", flush=True)
    del plane, windows, image
    # one iterate of the tiled loop
    pn, halo, ps, nx = 256, 64, 193.0 / 8.0, 4
    core = pn - 2 * halo
    source = L.LightSource(0.4, 0.8, pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
    socs = L.socsKernels(pupil, source, kernels=a.kernels)
    plan = L.planTiles((0.0, 0.0, nx * core * ps, nx * core * ps), pn, ps, wl, halo)
    gen = torch.Generator().manual_seed(7)
    target = (torch.rand((plan.n // 16, plan.n // 16), generator=gen) < 0.2).float().repeat_interleave(16, 0).repeat_interleave(16, 1)
    target = target.to(dev)
    open_mask = L.Mask(torch.ones((pn, pn), dtype=torch.int16), ps, dev)
    _, N = open_mask.calculateEpsilonN(open_mask.deltaK, ps, wl)
    clear = float(L.hopkinsIntensity(open_mask.fraunhofer(wl, True), socs, N)[pn // 2, pn // 2]) / socs.weight_sum

    def iterate():
        return L.optimizeMaskTiled(target, socs, plan, 0.3 * clear, iterations=1)
    res = iterate()
    ni = calls_for(iterate)
    ti = [window(iterate, ni) for _ in range(a.rounds)]
    print(f"optimizeMaskTiled, iterations = 1 (two forward sweeps and one backward) on {plan.nx} x {plan.ny} windows of {pn}^2, halo "
          f"{halo}, K {socs.K}: {show(ti, 1)} per call, {statistics.median(ti) / plan.count:.3f} ms per window; losses "
          f"{res.losses[0]:.5f} -> {res.losses[1]:.5f}", flush=True)


if __name__ == "__main__":
    main()
