"""Model-based OPC of a layout block several windows wide on one MI355X: GDSII-style polygons in, corrected polygons out as GDSII,
EPE before and after.

    python examples/tiled_opc.py [--pn 128] [--blocks 4] [--halo 32] [--kernels 24] [--iterations 4] [--out tiled_opc.gds]

The layout is the 96-polygon block of examples/tiled_layout.py (`blocks` x `blocks` cells of lines, an elbow and contacts) at the
pixel size 193 / 8 nm, where epsilon = 1.  correctLayoutTiled moves every edge fragment of the whole block on ONE stitched image: per
iterate one upload of the culled edges, one raster launch, one batched Hopkins image, one post-process and one stitch per chunk of
windows, one EPE measurement.  Both update rules are run: the damped one, and the MEEF-matrix step on the exact Jacobian of the tiled
model (epeJacobianTiled), of which the share of entries that couple fragments and sites of DIFFERENT tiles is printed -- what a
per-tile block Jacobian would drop.  seamError of the corrected layout's image is the halo's read-out."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lithographysimulator_amd as L                                     # noqa: E402
from lithographysimulator_amd import layout as LY                       # noqa: E402
from tiled_layout import cell                                            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--halo", type=int, default=32)
    ap.add_argument("--kernels", type=int, default=24)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--spacing", type=float, default=8.0, help="fragment length in pixels")
    ap.add_argument("--max-bias", type=float, default=24.0, help="nm")
    ap.add_argument("--threshold", type=float, default=0.3, help="fraction of the clear-field intensity")
    ap.add_argument("--out", default="/tmp/litho_tiled_opc.gds")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na, pn, ps = 193.0, 0.7, a.pn, 193.0 / 8.0
    size = pn * ps / 2.0                                                 # a cell is half a window wide
    polygons = [q for j in range(a.blocks) for i in range(a.blocks) for q in cell(i * size, j * size, size, i + 2 * j)]
    source = L.LightSource(0.4, 0.8, pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
    socs = L.socsKernels(pupil, source, kernels=a.kernels)
    open_mask = L.Mask(torch.ones((pn, pn), dtype=torch.int16), ps, dev)
    _, N = open_mask.calculateEpsilonN(open_mask.deltaK, ps, wl)
    clear = float(L.hopkinsIntensity(open_mask.fraunhofer(wl, True), socs, N)[pn // 2, pn // 2]) / socs.weight_sum
    threshold = a.threshold * clear
    kw = dict(spacing=a.spacing * ps, maxBias=a.max_bias, halo=a.halo, iterations=a.iterations, normalize=True)
    results = {}
    for step in ("damped", "meef"):
        r = results[step] = L.correctLayoutTiled(polygons, socs, pn, ps, wl, threshold, step=step, **kw)
        p = r.plan
        if step == "damped":
            print(f"{len(polygons)} polygons, {len(r.sites)} fragments; {p.nx} x {p.ny} windows of {pn}^2 pixels of {ps:g} nm with cores of "
                  f"{p.core}; K {socs.K} (captured {socs.captured:.4f})")
        print(f"step {step:6s}: RMS EPE per iterate (nm) {[round(h[0], 3) for h in r.history]}, sites without an edge "
              f"{[h[2] for h in r.history]}; best iterate {r.best_iteration}")
    meef = results["meef"]
    p, J = meef.plan, meef.jacobian
    g = np.floor(meef.sites.sites_px[:, :2].astype(np.float64) - p.offset_px + 0.5)
    home = np.clip(g[:, 1] // p.core, 0, p.ny - 1) * p.nx + np.clip(g[:, 0] // p.core, 0, p.nx - 1)
    filled = np.isfinite(J) & (J != 0.0)
    across = filled & (home[:, None] != home[None, :])
    print(f"MEEF matrix {J.shape[0]} x {J.shape[1]}: {filled.mean():.1%} of its entries are non-zero, {across.sum() / filled.sum():.1%} of those "
          f"couple a site and a fragment of different tiles (largest {np.abs(J[across]).max():.3f} nm / nm against a median diagonal of "
          f"{np.nanmedian(np.diag(J)):.3f})")
    best = min(results.values(), key=lambda r: (r.history[r.best_iteration][2], r.history[r.best_iteration][0]))
    tiled = L.hopkinsImageTiled(best.polygons, socs, pn, ps, wl, bounds=p.bounds, halo=a.halo, antialias=16, normalize=True, origin=None)
    print(f"corrected layout: RMS EPE {best.history[best.best_iteration][0]:.3f} nm (before: {best.history[0][0]:.3f} nm); seamError "
          f"{tiled.seamError:.5f} at halo {a.halo}")
    lib = L.contoursToGDSII(polygons, layer=1, name="TOP")
    lib.structures["TOP"].elements += L.contoursToGDSII(best.polygons, layer=2, name="TOP").structures["TOP"].elements
    LY.writeGDSII(lib, a.out)
    print(f"{a.out}: {len(polygons)} target polygons on layer 1, {len(best.polygons)} corrected polygons on layer 2")


if __name__ == "__main__":
    main()
