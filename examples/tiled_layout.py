"""A layout several windows wide on one MI355X: synthetic layout -> tiled Hopkins image (windows with halos, one batch per chunk,
cores stitched) -> EPE on every edge of the whole block -> printed contours of the whole block as GDSII.

    python examples/tiled_layout.py [--pn 128] [--pixel 24.125] [--blocks 4] [--halos 16 32] [--kernels 24] [--out tiled.gds]

The layout is `blocks` x `blocks` cells of lines, an elbow and contacts, each cell a little different, about `blocks` / 2 windows
wide.  It is imaged once per halo and `seamError` -- the largest disagreement of neighbouring windows at the boundary of their
cores, relative to the image's maximum -- is printed for each: the halo's read-out.  The default pixel, 193 / 8 nm, has
epsilon = 1; at 25 nm the reference's resample chain is not translation invariant and the seams keep a few percent whatever the
halo (tiling.py)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lithographysimulator_amd as L                                     # noqa: E402
from lithographysimulator_amd import layout as LY                       # noqa: E402


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def cell(x, y, size, k):
    """One cell of the block at (x, y): three lines whose pitch depends on k, an elbow, two contacts."""
    u = size / 16.0
    pitch = (2.4 + 0.2 * (k % 3)) * u
    out = [rect(x + 2 * u + i * pitch, y + 2 * u, x + 2 * u + i * pitch + 1.1 * u, y + 9 * u) for i in range(3)]
    out.append(np.array([[x + 10 * u, y + 2 * u], [x + 14 * u, y + 2 * u], [x + 14 * u, y + 3.2 * u], [x + 11.2 * u, y + 3.2 * u],
                         [x + 11.2 * u, y + 8 * u], [x + 10 * u, y + 8 * u]]))
    out += [rect(x + (3 + 5 * j) * u, y + 11 * u, x + (5 + 5 * j) * u, y + 13 * u) for j in range(2)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=128)
    ap.add_argument("--pixel", type=float, default=193.0 / 8.0)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--halos", type=int, nargs="*", default=[16, 32])
    ap.add_argument("--kernels", type=int, default=24)
    ap.add_argument("--antialias", type=int, default=4, choices=(1, 2, 4, 8, 16))
    ap.add_argument("--threshold", type=float, default=0.3, help="fraction of the clear-field intensity")
    ap.add_argument("--out", default="/tmp/litho_tiled_layout.gds")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na, pn, ps = 193.0, 0.7, a.pn, a.pixel
    size = pn * ps / 2.0                                                 # a cell is half a window wide
    polygons = [q for j in range(a.blocks) for i in range(a.blocks) for q in cell(i * size, j * size, size, i + 2 * j)]
    bounds = (0.0, 0.0, a.blocks * size, a.blocks * size)
    source = L.LightSource(0.4, 0.8, pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
    socs = L.socsKernels(pupil, source, kernels=a.kernels)
    print(f"{len(polygons)} polygons on {bounds[2]:.0f} x {bounds[3]:.0f} nm; windows of {pn}^2 pixels of {ps:g} nm; K {socs.K} "
          f"(captured {socs.captured:.4f})")
    tiled = None
    for halo in a.halos:
        tiled = L.hopkinsImageTiled(polygons, socs, pn, ps, wl, bounds=bounds, halo=halo, antialias=a.antialias, normalize=True)
        p = tiled.plan
        print(f"halo {halo:3d}: {p.nx} x {p.ny} tiles with cores of {p.core} pixels, stitched image {p.n}^2; seamError {tiled.seamError:.5f}")
    # clear field: an open frame imaged as one window, the threshold's reference
    open_mask = L.Mask(torch.ones((pn, pn), dtype=torch.int16), ps, dev)
    _, N = open_mask.calculateEpsilonN(open_mask.deltaK, ps, wl)
    clear = float(L.hopkinsIntensity(open_mask.fraunhofer(wl, True), socs, N)[pn // 2, pn // 2]) / socs.weight_sum
    threshold = a.threshold * clear
    sites = tiled.sites(polygons, spacing=4 * ps)
    epe = L.measureEPE(tiled.image, threshold, sites, ps, exposed=True)[0, 0, :, 0].cpu().numpy()
    found = np.isfinite(epe)
    print(f"EPE at {len(sites)} sites on every edge of the block (threshold {a.threshold:g} of the clear field): {int(found.sum())} "
          f"crossings found, mean {epe[found].mean():+.1f} nm, rms {np.sqrt((epe[found] ** 2).mean()):.1f} nm, worst "
          f"{np.abs(epe[found]).max():.1f} nm")
    contours = L.traceContours(tiled.image, threshold)[0][0]
    printed = tiled.toLayout(contours)
    lib = L.contoursToGDSII(polygons, layer=1, name="TOP")
    lib.structures["TOP"].elements += L.contoursToGDSII(printed, layer=2, tolerance_nm=0.5, name="TOP").structures["TOP"].elements
    LY.writeGDSII(lib, a.out)
    print(f"{a.out}: {len(polygons)} target polygons on layer 1, {len(printed)} printed contours ({int(contours.holes.sum())} holes) "
          f"on layer 2")


if __name__ == "__main__":
    main()
