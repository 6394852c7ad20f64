"""Tiled inverse lithography on one MI355X: a block of contacts and line ends several windows wide -> ONE pixel mask for the whole
block, optimised through windows with halos (one batched image and one batched mask gradient per chunk of windows, the window
gradients summed back into the global mask) -> EPE on the stitched image before and after -> the mask as GDSII.

    python examples/tiled_ilt.py [--pn 128] [--halo 32] [--blocks 2] [--kernels 24] [--iterations 20] [--out tiled_ilt.gds]

The block is `blocks` x `blocks` cores wide (cores of pn - 2 halo pixels); the default pixel, 193 / 8 nm, has epsilon = 1 -- at
25 nm the reference's resample chain is not translation invariant and neighbouring windows disagree whatever the halo
(tiling.py).  Features are placed across the core boundaries on purpose: their gradient reaches them through two windows."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lithographysimulator_amd as L                                     # noqa: E402
from lithographysimulator_amd import layout as LY                       # noqa: E402


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def block_layout(blocks, core_nm, cd):
    """Per core: two contacts inside, a contact across its right boundary and a line whose end crosses its upper boundary (where
    there is a neighbour)."""
    out = []
    for j in range(blocks):
        for i in range(blocks):
            x, y = i * core_nm, j * core_nm
            out += [rect(x + 0.25 * core_nm, y + 0.25 * core_nm, x + 0.25 * core_nm + cd, y + 0.25 * core_nm + cd),
                    rect(x + 0.25 * core_nm + 2 * cd, y + 0.25 * core_nm, x + 0.25 * core_nm + 3 * cd, y + 0.25 * core_nm + cd)]
            if i + 1 < blocks:
                out.append(rect(x + core_nm - 0.5 * cd, y + 0.6 * core_nm, x + core_nm + 0.5 * cd, y + 0.6 * core_nm + cd))
            if j + 1 < blocks:
                out.append(rect(x + 0.7 * core_nm, y + 0.55 * core_nm, x + 0.7 * core_nm + cd, y + core_nm + 1.5 * cd))
    return out


def rms_epe(image, threshold, sites, pixel):
    e = L.measureEPE(image, threshold, sites, pixel, exposed=True)[0, 0, :, 0]
    lost = int(torch.isnan(e).sum())
    e = e[~torch.isnan(e)]
    return (float(torch.sqrt((e * e).mean())) if e.numel() else float("nan")), lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=128)
    ap.add_argument("--pixel", type=float, default=193.0 / 8.0)
    ap.add_argument("--halo", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--kernels", type=int, default=24)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--threshold", type=float, default=0.3, help="fraction of the clear-field intensity")
    ap.add_argument("--out", default="/tmp/litho_tiled_ilt.gds")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na, pn, ps = 193.0, 0.7, a.pn, a.pixel
    core = pn - 2 * a.halo
    core_nm = core * ps
    polygons = block_layout(a.blocks, core_nm, 6 * ps)
    bounds = (0.0, 0.0, a.blocks * core_nm, a.blocks * core_nm)
    source = L.LightSource(0.4, 0.8, pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
    socs = L.socsKernels(pupil, source, kernels=a.kernels)
    # the target drawn as the mask: the tiled image of the polygons, its plan, and the seam read-out of this halo
    drawn = L.hopkinsImageTiled(polygons, socs, pn, ps, wl, bounds=bounds, halo=a.halo, normalize=True)
    plan = drawn.plan
    rows, cols = plan.ny * core, plan.nx * core
    print(f"{len(polygons)} polygons on {bounds[2]:.0f} x {bounds[3]:.0f} nm; {plan.nx} x {plan.ny} windows of {pn}^2 pixels of {ps:g} nm, "
          f"halo {a.halo}, cores of {core}; K {socs.K} (captured {socs.captured:.4f}); seamError {drawn.seamError:.5f}")
    open_mask = L.Mask(torch.ones((pn, pn), dtype=torch.int16), ps, dev)
    _, N = open_mask.calculateEpsilonN(open_mask.deltaK, ps, wl)
    clear = float(L.hopkinsIntensity(open_mask.fraunhofer(wl, True), socs, N)[pn // 2, pn // 2]) / socs.weight_sum
    threshold = a.threshold * clear
    # the target on the stitched grid: stitched pixel G shows raster pixel G - offset_px, a fraction of a pixel
    shift = plan.offset_px * ps
    target = torch.zeros((plan.n, plan.n), dtype=torch.float32, device=dev)
    side = 1 << (max(rows, cols, 16) - 1).bit_length()              # a square raster that holds the covered region
    shifted = L.rasterizeLayout(polygons, side, ps, (plan.origin[0] - shift, plan.origin[1] - shift), dev)
    target[:rows, :cols] = shifted[:rows, :cols].float()
    sites = drawn.sites(polygons, spacing=3 * ps)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = L.optimizeMaskTiled(target, socs, plan, threshold, iterations=a.iterations)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print("loss history: " + " ".join(f"{v:.5f}" for v in res.losses))
    after_image = L.maskImageTiled(res.transmission, socs, plan, normalize=True)
    before, lost_before = rms_epe(drawn.image, threshold, sites, ps)
    after, lost_after = rms_epe(after_image, threshold, sites, ps)
    print(f"{a.iterations} iterations over {plan.count} windows in {seconds:.2f} s ({seconds / (a.iterations + 1) * 1e3:.1f} ms each)")
    print(f"target drawn as the mask: loss {res.losses[0]:.5f}, RMS EPE {before:.2f} nm ({lost_before} of {len(sites)} sites without an edge)")
    print(f"optimised mask (iterate {res.best}): loss {res.losses[res.best]:.5f}, RMS EPE {after:.2f} nm ({lost_after} sites without an edge)")

    mask_nm = L.maskPolygons(plan, res.transmission.real.contiguous())
    lib = L.contoursToGDSII(polygons, layer=1, name="TOP")
    lib.structures["TOP"].elements += L.contoursToGDSII(mask_nm, layer=2, tolerance_nm=0.5, name="TOP").structures["TOP"].elements
    LY.writeGDSII(lib, a.out)
    back = LY.readGDSII(a.out)
    print(f"{a.out}: target on layer 1, optimised mask ({len(mask_nm)} polygons) on layer 2; {len(back.structures['TOP'].elements)} boundaries")


if __name__ == "__main__":
    main()
