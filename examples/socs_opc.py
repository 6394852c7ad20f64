"""The line-end correction of examples/opc_line_ends.py under both imaging models on one MI355X: the Abbe sum (one field per
source point, every iteration) and Hopkins imaging (the optical setting factored once into K SOCS kernels, K fields per
iteration).

    python examples/socs_opc.py [--pn 128] [--pixel 25] [--iterations 6] [--kernels 64] [--antialias 16]

Prints the captured fraction of the kernels, the RMS edge placement error of every iteration under either model, and what each
costs: the set-up (socsKernels, once per optical setting) and the time per iteration (raster, mask spectrum, image, EPE).  A
truncated kernel set is an approximation: its EPE differs from the Abbe model's by what `captured` leaves out."""
import argparse
import os
import sys
import time

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
    ap.add_argument("--antialias", type=int, default=16, choices=(1, 2, 4, 8, 16))
    ap.add_argument("--threshold", type=float, default=0.3, help="fraction of the clear-field intensity")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na = 193.0, 0.7
    polygons, origin = demo_layout(), (0.0, 0.0)
    source = L.LightSource(0.4, 0.8, a.pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(a.pn, wl, na, None, dev).generatePupilFunction()
    open_mask = L.Mask(torch.ones((a.pn, a.pn), dtype=torch.int16), a.pixel, dev)
    eps, N = open_mask.calculateEpsilonN(open_mask.deltaK, a.pixel, wl)
    clear = L.abbeIntensity(open_mask.fraunhofer(wl, True), pupil, L.sourceShifts(source, a.pn), N)
    threshold = a.threshold * float(clear[a.pn // 2, a.pn // 2])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    socs = L.socsKernels(pupil, source, kernels=a.kernels)
    torch.cuda.synchronize()
    print(f"{int(torch.count_nonzero(source))} source points -> {socs.K} kernels, captured {socs.captured:.4f} of trace T; "
          f"set-up {time.perf_counter() - t0:.2f} s (paid again inside correctLayout below)")
    for model in ("abbe", "socs"):
        kw = dict(spacing=a.spacing, maxBias=a.max_bias, antialias=a.antialias, model=model, kernels=a.kernels)
        L.correctLayout(polygons, a.pn, a.pixel, origin, wl, pupil, source, threshold, iterations=1, **kw)      # warm
        times = []
        for iterations in (1, a.iterations + 1):                        # the difference of the two runs is the iterations alone
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = L.correctLayout(polygons, a.pn, a.pixel, origin, wl, pupil, source, threshold, iterations=iterations, **kw)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        per_iteration = (times[1] - times[0]) / a.iterations
        print(f"model {model}: {per_iteration * 1e3:.2f} ms per iteration, {times[0] - per_iteration:.2f} s before the first")
        for it, (rms, worst, lost) in enumerate(res.history[:a.iterations]):
            print(f"    iteration {it}: RMS EPE {rms:6.2f} nm, max {worst:6.2f} nm, {lost} sites without a printed edge")


if __name__ == "__main__":
    main()
