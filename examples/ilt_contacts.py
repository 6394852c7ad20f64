"""Pixel-based inverse lithography on one MI355X: a few contacts and a line end near the resolution limit -> the mask that prints
them, by steepest descent through Hopkins imaging (the optical setting factored once into SOCS kernels, then K fields and K
adjoint fields per iteration).

    python examples/ilt_contacts.py [--pn 128] [--pixel 25] [--kernels 48] [--iterations 40] [--out ilt_mask.gds]

Prints the loss and the RMS edge placement error of the target drawn as the mask and of the optimised mask, then traces the
optimised (continuous) mask at transmission 0.5 and writes it as GDSII: the target on layer 1, the mask on layer 2."""
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


def demo_layout():
    """Four 150 nm contacts (lambda / NA = 276 nm: 0.54 of it), two of them 150 nm apart, and a 150 nm line whose end faces one."""
    contacts = [rect(x, y, x + 150.0, y + 150.0) for x, y in ((800.0, 800.0), (1100.0, 800.0), (800.0, 1500.0), (2000.0, 2200.0))]
    return contacts + [rect(1500.0, 1000.0, 1650.0, 2000.0)]


def rms_epe(image, threshold, sites, pixel):
    e = L.measureEPE(image, threshold, sites, pixel)[0, 0, :, 0]
    lost = int(torch.isnan(e).sum())
    e = e[~torch.isnan(e)]
    return (float(torch.sqrt((e * e).mean())) if e.numel() else float("nan")), lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=128)
    ap.add_argument("--pixel", type=float, default=25.0)
    ap.add_argument("--kernels", type=int, default=48)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--threshold", type=float, default=0.3, help="fraction of the clear-field intensity")
    ap.add_argument("--out", default="/tmp/litho_ilt_mask.gds")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na = 193.0, 0.7
    polygons, origin = demo_layout(), (0.0, 0.0)
    source = L.LightSource(0.4, 0.8, a.pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(a.pn, wl, na, None, dev).generatePupilFunction()
    t0 = time.perf_counter()
    socs = L.socsKernels(pupil, source, kernels=a.kernels)
    torch.cuda.synchronize()
    print(f"{int(torch.count_nonzero(source))} source points -> {socs.K} kernels, captured {socs.captured:.4f} of trace T, "
          f"{time.perf_counter() - t0:.2f} s")

    open_mask = L.Mask(torch.ones((a.pn, a.pn), dtype=torch.int16), a.pixel, dev)
    deltaK = open_mask.deltaK
    clear = L.hopkinsImage(open_mask, open_mask.fraunhofer(wl, True), socs, a.pixel, deltaK, wl, normalize=True)
    n_out = clear.shape[-1]
    threshold = a.threshold * float(clear[n_out // 2, n_out // 2])
    # the target on the image grid: image pixel J shows mask pixel J - offset (imageRegistration), a fraction of a pixel
    _, offset = L.imageRegistration(a.pn, a.pixel, wl)
    drawn = L.rasterizeLayout(polygons, a.pn, a.pixel, origin, dev)
    shifted = L.rasterizeLayout(polygons, a.pn, a.pixel, (origin[0] - offset * a.pixel, origin[1] - offset * a.pixel), dev)
    target = torch.zeros((n_out, n_out), dtype=torch.float32, device=dev)
    k = min(a.pn, n_out)
    target[:k, :k] = shifted[:k, :k].float()
    sites = L.layoutSites(polygons, 75.0, a.pixel, origin, a.pn, wl)

    def image_of(transmission):
        mask = L.Mask(transmission=transmission, pixelSize=a.pixel, device=dev)
        return L.hopkinsImage(mask, mask.fraunhofer(wl, True), socs, a.pixel, deltaK, wl, normalize=True)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = L.optimizeMask(target, socs, a.pixel, deltaK, wl, threshold, iterations=a.iterations)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    before, lost_before = rms_epe(image_of(drawn.to(torch.complex64)), threshold, sites, a.pixel)
    after, lost_after = rms_epe(image_of(res.transmission), threshold, sites, a.pixel)
    print(f"{a.iterations} iterations in {seconds:.2f} s ({seconds / (a.iterations + 1) * 1e3:.1f} ms each)")
    print(f"target drawn as the mask: loss {res.losses[0]:.5f}, RMS EPE {before:.2f} nm ({lost_before} of {len(sites)} sites without an edge)")
    print(f"optimised mask (iterate {res.best}): loss {res.losses[res.best]:.5f}, RMS EPE {after:.2f} nm ({lost_after} sites without an edge)")

    traced = L.traceContours(res.transmission.real.contiguous(), 0.5)[0][0]
    # mask-raster pixel (r, c) has its centre at origin + (c + 0.5, r + 0.5) pixel (rasterizeLayout)
    mask_nm = [(np.asarray(q, dtype=np.float64) + 0.5) * a.pixel + np.array(origin) for q in traced.polygons]
    lib = L.contoursToGDSII(polygons, layer=1, name="TOP")
    lib.structures["TOP"].elements += L.contoursToGDSII(mask_nm, layer=2, tolerance_nm=0.5, name="TOP").structures["TOP"].elements
    LY.writeGDSII(lib, a.out)
    back = LY.readGDSII(a.out)
    print(f"{a.out}: target on layer 1, optimised mask ({len(traced)} polygons, {int(traced.holes.sum())} holes) on layer 2; "
          f"{len(back.structures['TOP'].elements)} boundaries")


if __name__ == "__main__":
    main()
