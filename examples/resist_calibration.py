"""Calibrating a chemically amplified resist to CDs measured through dose and focus, on one MI355X.

    python examples/resist_calibration.py [--n 32] [--depths 4] [--pixel 10] [--thickness 80] [--time 20] [--iterations 40]
                                          [--off 1.2] [--parameters kAmp acidDiffusionLength] [--method descent|lm]

A synthetic experiment.  The intensity is a line/space grating with a standing wave through the depth at two focus settings (the
second with less contrast), exposed at three doses.  A KNOWN resist prints it; the widths of the developed space at every dose,
focus and depth are the "measured" CDs.  The fit then starts from the same resist with the chosen parameters multiplied by
`--off` and runs calibrateResist: steepest descent with backtracking on the mean of (T / developTime - 1)^2 at the measured edges,
the gradient coming from resistParameterGradient's chain (development front -> rate law -> bake -> exposure, all in HIP).
`--method lm` takes Levenberg-Marquardt steps instead, on the Jacobian of the edge residuals from the forward mode (tangent.py).

It prints the measured CDs, the loss and the parameters before and after, the accepted steps, and the CDs the fitted resist
prints next to the measured ones."""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lithographysimulator_amd as L                                     # noqa: E402


def grating(n, D, pitch, contrast):
    """Bright spaces of `pitch` pixels period along x, a standing wave through the depth: fp32 [D, n, n]."""
    x = np.arange(n)
    lateral = 0.5 * (1.0 + contrast * np.cos(2.0 * math.pi * (x - n // 2) / pitch))
    depth = 1.0 + 0.25 * np.cos(2.0 * math.pi * (np.arange(D) + 0.5) / D * 1.5)
    return (depth[:, None, None] * lateral[None, None, :] * np.ones((1, n, 1))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--depths", type=int, default=4)
    ap.add_argument("--pixel", type=float, default=10.0)
    ap.add_argument("--thickness", type=float, default=80.0)
    ap.add_argument("--time", type=float, default=20.0, help="development time, s")
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--off", type=float, default=1.2, help="the factor on every fitted parameter at the start")
    ap.add_argument("--parameters", nargs="+", default=["kAmp", "acidDiffusionLength"])
    ap.add_argument("--method", choices=("descent", "lm"), default="descent")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, D, F, doses = a.n, a.depths, 2, (0.8, 1.0, 1.25)
    image = torch.from_numpy(np.concatenate([grating(n, D, 16, 0.8), grating(n, D, 16, 0.65)])).to(dev)     # [F D, n, n]
    truth = L.ChemicallyAmplifiedResist(C=2.0, quencher=0.15, kAmp=0.04, kQuench=5.0, kLoss=0.002, acidDiffusionLength=12.0,
                                        quencherDiffusionLength=4.0, verticalScale=1.0, bakeTime=60.0,
                                        mack=L.MackResist(C=1.0, rMax=120.0, rMin=0.05, q=5.0, mTh=0.4))
    steps = max(8, 2 * truth.minSteps(a.thickness, D, a.pixel))
    T = L.resistArrivalTimes(image, truth, a.thickness, a.pixel, doses, F, steps)
    prof = L.ResistProfile(T, None, 0, a.thickness, a.pixel, a.time, doses)
    gauge = (n // 2, n // 2, 0)
    cds = prof.cd([gauge]).cpu().numpy().reshape(len(doses), F, D, 5)
    measurements = [(di, fi, d, (n // 2, 0.5 * float(cds[di, fi, d, 1] + cds[di, fi, d, 2]), 0), float(cds[di, fi, d, 0]))
                    for di in range(len(doses)) for fi in range(F) for d in range(D)
                    if cds[di, fi, d, 0] > 0 and 0 < cds[di, fi, d, 1] and cds[di, fi, d, 2] < n - 1]
    print(f"{len(measurements)} CDs of the known resist (nm), dose x focus x depth; {steps} bake steps, {a.time:g} s of development")
    for di, dose in enumerate(doses):
        for fi in range(F):
            print(f"   dose {dose:4.2f} focus {fi}: " + " ".join(f"{cds[di, fi, d, 0]:7.2f}" for d in range(D)))
    start = L.resistWith(truth, **{k: a.off * L.resistParameter(truth, k) for k in a.parameters})
    fitted, history = L.calibrateResist(image, start, a.thickness, a.pixel, a.time, measurements, parameters=a.parameters, doses=doses,
                                        focalPlanes=F, iterations=a.iterations, steps=steps, method=a.method)
    accepted = [h for h in history if h["accepted"]]
    print(f"-- {len(history)} evaluations, {len(accepted)} accepted")
    for h in accepted:
        print(f"   loss {h['loss']:.4e}  step {h['step']:.4f}  " + (f"damping {h['damping']:.0e}  " if "damping" in h else "") + "  ".join(f"{k} {v:.5g}" for k, v in h["parameters"].items()))
    print(f"-- loss {history[0]['loss']:.4e} -> {accepted[-1]['loss']:.4e}")
    for k in a.parameters:
        print(f"   {k}: start {L.resistParameter(start, k):.5g}, fitted {L.resistParameter(fitted, k):.5g}, known {L.resistParameter(truth, k):.5g}")
    T = L.resistArrivalTimes(image, fitted, a.thickness, a.pixel, doses, F, steps)
    got = L.ResistProfile(T, None, 0, a.thickness, a.pixel, a.time, doses).cd([gauge]).cpu().numpy()
    got = got.reshape(len(doses), F, D, 5)
    worst = max(abs(float(got[di, fi, d, 0]) - cd) for di, fi, d, _, cd in measurements)
    print(f"-- the fitted resist prints the measured CDs within {worst:.2f} nm")


if __name__ == "__main__":
    main()
