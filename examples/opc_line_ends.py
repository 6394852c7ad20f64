"""Model-based OPC on one MI355X: a small Manhattan layout (three 150 nm lines at 400 nm pitch, an isolated line, an L
and a 200 nm contact) -> edge placement error of the uncorrected mask -> correctLayout -> EPE of the corrected mask ->
the corrected layout as GDSII.

    python examples/opc_line_ends.py [--pn 128] [--pixel 25] [--iterations 6] [--antialias 16] [--diffusion 0] [--out corrected.gds]

Line ends pull back and the contact prints small; the loop moves edge fragments of at most --spacing nm along their
normals until the printed contour (threshold 0.3 x clear field) lies on the drawn edges.  Prints the RMS and the largest
EPE of every iteration."""
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


def demo_layout():
    lines = [rect(400.0 + 400.0 * i, 600.0, 550.0 + 400.0 * i, 1800.0) for i in range(3)]
    ell = np.array([[1900.0, 2000.0], [2700.0, 2000.0], [2700.0, 2200.0], [2100.0, 2200.0], [2100.0, 2800.0], [1900.0, 2800.0]])
    return lines + [rect(2050.0, 500.0, 2200.0, 1700.0), ell, rect(700.0, 2300.0, 900.0, 2500.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=128)
    ap.add_argument("--pixel", type=float, default=25.0)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--spacing", type=float, default=150.0, help="longest edge fragment, nm")
    ap.add_argument("--max-bias", type=float, default=60.0)
    ap.add_argument("--antialias", type=int, default=16, choices=(1, 2, 4, 8, 16))
    ap.add_argument("--diffusion", type=float, default=0.0, metavar="NM")
    ap.add_argument("--threshold", type=float, default=0.3, help="fraction of the clear-field intensity")
    ap.add_argument("--out", default="/tmp/litho_opc_corrected.gds")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na = 193.0, 0.7
    polygons = demo_layout()
    origin = (0.0, 0.0)
    source = L.LightSource(0.4, 0.8, a.pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(a.pn, wl, na, None, dev).generatePupilFunction()
    # clear-field level: the same optics over an all-open mask (raw sums over the source points, like the loop's images)
    open_mask = L.Mask(torch.ones((a.pn, a.pn), dtype=torch.int16), a.pixel, dev)
    eps, N = open_mask.calculateEpsilonN(open_mask.deltaK, a.pixel, wl)
    clear = L.abbeIntensity(open_mask.fraunhofer(wl, True), pupil, L.sourceShifts(source, a.pn), N)
    threshold = a.threshold * float(clear[a.pn // 2, a.pn // 2])
    n_out, offset = L.imageRegistration(a.pn, a.pixel, wl)
    print(f"image {n_out} x {n_out}, shifted against the mask raster by {offset:+.4f} px = {offset * a.pixel:+.2f} nm")
    res = L.correctLayout(polygons, a.pn, a.pixel, origin, wl, pupil, source, threshold, spacing=a.spacing,
                          iterations=a.iterations, maxBias=a.max_bias, antialias=a.antialias, diffusionLength=a.diffusion)
    print(f"{len(res.sites)} sites on {len(polygons)} polygons")
    for it, (rms, worst, lost) in enumerate(res.history):
        print(f"iteration {it}: RMS EPE {rms:6.2f} nm, max {worst:6.2f} nm, {lost} sites without a printed edge"
              + ("   <- returned" if it == res.best_iteration else ""))
    print(f"EPE before: RMS {res.history[0][0]:.2f} nm; after: RMS {res.history[res.best_iteration][0]:.2f} nm; "
          f"biases {res.bias_nm.min():+.1f} .. {res.bias_nm.max():+.1f} nm")
    lib = LY.GdsLibrary("OPC", 1e-3, 1e-10)                              # database unit = 0.1 nm
    top = LY.GdsStructure("TOP")
    for layer, polys in ((1, polygons), (2, res.polygons)):              # layer 1: the target, layer 2: the corrected mask
        for q in polys:
            xy = np.rint(np.asarray(q) * 10.0).astype(np.int64)
            top.elements.append(LY.GdsElement("boundary", layer=layer, datatype=0, xy=np.concatenate([xy, xy[:1]])))
    lib.structures["TOP"] = top
    LY.writeGDSII(lib, a.out)
    back = LY.flattenLayout(LY.readGDSII(a.out), layers=[(2, 0)])
    print(f"{a.out}: target on layer 1, corrected mask on layer 2 ({sum(len(q) for q in back)} vertices)")


if __name__ == "__main__":
    main()
