"""The mask-error factor of line ends, and the correction loop with the MEEF matrix as its model, on one MI355X:

    python examples/meef_line_ends.py [--pn 128] [--pixel 25] [--iterations 6] [--kernels 64]

On the layout of examples/opc_line_ends.py (dense lines, an isolated line, an L, a contact) through K SOCS kernels it prints the
MEEF dCD_printed / dCD_mask of a dense line, of the isolated line and of a line end (the length of a dense line: its two ends
move), each from ONE forward-mode pass (maskErrorFactor), then the RMS edge placement error per iteration of correctLayout with
the damped fixed-point step (every fragment moves its own edge one for one) against step="meef" (one EPE Jacobian at the first
iterate, forward mode, one pass per fragment; then Levenberg-Marquardt steps on it)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lithographysimulator_amd as L                                     # noqa: E402
from opc_line_ends import demo_layout                                    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=128)
    ap.add_argument("--pixel", type=float, default=25.0)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--kernels", type=int, default=64)
    ap.add_argument("--spacing", type=float, default=150.0, help="longest edge fragment, nm")
    ap.add_argument("--max-bias", type=float, default=60.0)
    ap.add_argument("--threshold", type=float, default=0.3, help="fraction of the clear-field intensity")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na = 193.0, 0.7
    polygons, origin = demo_layout(), (0.0, 0.0)
    source = L.LightSource(0.0, 0.5, a.pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(a.pn, wl, na, None, dev).generatePupilFunction()
    socs = L.socsKernels(pupil, source, kernels=a.kernels)
    open_mask = L.Mask(torch.ones((a.pn, a.pn), dtype=torch.int16), a.pixel, dev)
    eps, N = open_mask.calculateEpsilonN(open_mask.deltaK, a.pixel, wl)
    clear = L.hopkinsIntensity(open_mask.fraunhofer(wl, True), socs, N)
    threshold = a.threshold * float(clear[a.pn // 2, a.pn // 2])
    print(f"{int(torch.count_nonzero(source))} source points -> {socs.K} kernels, captured {socs.captured:.4f} of trace T")

    def px(nm):
        return int(nm / a.pixel)
    # (row, col, axis): across the middle dense line, across the isolated line, along the middle dense line (its ends)
    gauges = {"dense line, width": (px(1200.0), px(875.0), 0), "isolated line, width": (px(1100.0), px(2125.0), 0),
              "dense line, length (line ends)": (px(1200.0), px(875.0), 1)}
    cd, meef = L.maskErrorFactor(polygons, list(gauges.values()), socs, a.pn, a.pixel, origin, wl, threshold)
    for name, c, m in zip(gauges, cd[0].tolist(), meef[0].tolist()):
        print(f"    {name:32s} CD {c:8.2f} nm, MEEF {m:5.2f}")
    kw = dict(spacing=a.spacing, maxBias=a.max_bias, iterations=a.iterations, model="socs", socs=socs)
    for step in ("damped", "meef"):
        res = L.correctLayout(polygons, a.pn, a.pixel, origin, wl, pupil, source, threshold, step=step, **kw)
        print(f"step {step}: best iteration {res.best_iteration}")
        for it, (rms, worst, lost) in enumerate(res.history):
            print(f"    iteration {it}: RMS EPE {rms:6.2f} nm, max {worst:6.2f} nm, {lost} sites without a printed edge")


if __name__ == "__main__":
    main()
