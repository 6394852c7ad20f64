"""GDSII in, GDSII out on one MI355X: a small layout -> area-coverage mask -> Abbe image at three focal planes -> printed
contours at three doses as polygons -> the target, the nominal print and the process-variation band in one GDSII file.

    python examples/printed_contours.py [--pn 128] [--pixel 25] [--antialias 8] [--defocus 80] [--dose 0.1] [--out printed.gds]

Layer 1: the target; layer 2: the contour at nominal dose and focus (holes on datatype 1); layer 3: the outer and layer 4 the
inner edge of the PV band (what prints under any / under every condition).  Prints the printed area of every feature
against its drawn area, features that vanished or merged, and the band's area."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lithographysimulator_amd as L                                     # noqa: E402
from lithographysimulator_amd import layout as LY                       # noqa: E402
from lithographysimulator_amd.contours import signedArea                # noqa: E402


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def demo_layout():
    lines = [rect(400.0 + 400.0 * i, 600.0, 550.0 + 400.0 * i, 1800.0) for i in range(3)]
    ell = np.array([[1900.0, 2000.0], [2700.0, 2000.0], [2700.0, 2200.0], [2100.0, 2200.0], [2100.0, 2800.0], [1900.0, 2800.0]])
    frame = [rect(500.0, 2100.0, 1300.0, 2250.0), rect(500.0, 2650.0, 1300.0, 2800.0), rect(500.0, 2250.0, 650.0, 2650.0),
             rect(1150.0, 2250.0, 1300.0, 2650.0)]                      # a closed frame: prints with a hole
    return lines + [rect(2050.0, 500.0, 2200.0, 1700.0), ell] + frame


def inside(polygon, x, y):
    q = np.asarray(polygon)
    a, b = q, np.roll(q, -1, axis=0)
    hit = ((a[:, 1] <= y) != (b[:, 1] <= y)) & (x < a[:, 0] + (y - a[:, 1]) * (b[:, 0] - a[:, 0]) / np.where(b[:, 1] != a[:, 1], b[:, 1] - a[:, 1], 1.0))
    return bool(hit.sum() % 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=128)
    ap.add_argument("--pixel", type=float, default=25.0)
    ap.add_argument("--antialias", type=int, default=8, choices=(1, 2, 4, 8, 16))
    ap.add_argument("--defocus", type=float, default=80.0, metavar="NM")
    ap.add_argument("--dose", type=float, default=0.1, help="relative dose variation")
    ap.add_argument("--threshold", type=float, default=0.3, help="fraction of the clear-field intensity")
    ap.add_argument("--tolerance", type=float, default=0.5, metavar="NM", help="contour simplification")
    ap.add_argument("--out", default="/tmp/litho_printed_contours.gds")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na = 193.0, 0.7
    polygons = demo_layout()
    origin = (0.0, 0.0)
    raster = L.rasterizeLayout(polygons, a.pn, a.pixel, origin, dev, antialias=a.antialias)
    mask = L.Mask(pixelSize=a.pixel, device=dev, transmission=raster) if raster.is_floating_point() else L.Mask(raster, a.pixel, dev)
    eps, N = mask.calculateEpsilonN(mask.deltaK, a.pixel, wl)
    shifts = L.sourceShifts(L.LightSource(0.4, 0.8, a.pn, na, device=dev).generateAnnular(), a.pn)
    zero = torch.zeros(5, dtype=torch.float16)
    pupils = L.throughFocusPupils(a.pn, wl, na, zero, [-a.defocus, 0.0, a.defocus], dev)
    image = L.postProcess(L.abbeIntensity(mask.fraunhofer(wl, True), pupils, shifts, N), eps)      # [3, n, n]
    open_mask = L.Mask(torch.ones((a.pn, a.pn), dtype=torch.int16), a.pixel, dev)
    clear = L.abbeIntensity(open_mask.fraunhofer(wl, True), pupils[1], shifts, N)
    threshold = a.threshold * float(clear[a.pn // 2, a.pn // 2])
    doses = [1.0 - a.dose, 1.0, 1.0 + a.dose]

    traced = L.traceContours(image, threshold, doses)                   # [dose][plane]
    nominal = traced[1][1]
    outer, inner, band_px = L.processVariationBand(image, threshold, doses)
    to_nm = lambda c: L.contoursToLayout(c, a.pixel, origin, a.pn, wl)  # noqa: E731
    nominal_nm, outer_nm, inner_nm = to_nm(nominal), to_nm(outer), to_nm(inner)
    px_area = (abs(signedArea(to_nm([rect(0, 0, 1, 1)])[0])))           # nm^2 per image pixel^2

    print(f"{len(nominal)} printed polygons at nominal dose and focus ({int(nominal.holes.sum())} holes), "
          f"{sum(len(q) for q in nominal.polygons)} vertices")
    owners = [[k for k, q in enumerate(polygons) if inside(q, *p.mean(axis=0))] for p in nominal_nm]
    for k, q in enumerate(polygons):
        mine = [i for i, own in enumerate(owners) if k in own and not nominal.holes[i]]
        drawn = abs(signedArea(q))
        if not mine:
            print(f"feature {k}: drawn {drawn:9.0f} nm^2 -- did not print")
            continue
        printed = sum(signedArea(nominal_nm[i]) for i in mine)
        print(f"feature {k}: drawn {drawn:9.0f} nm^2, printed {printed:9.0f} nm^2 ({100.0 * printed / drawn:5.1f} %)"
              + ("  (part of a merged print)" if any(len(owners[i]) > 1 for i in mine) else ""))
    for d, per_dose in zip(doses, traced):
        print(f"dose {d:.2f}: printed area " + ", ".join(f"{c.total_area_px * px_area:9.0f}" for c in per_dose) + " nm^2 at the three focal planes")
    print(f"PV band over {len(doses)} doses x 3 focal planes: {band_px * px_area:.0f} nm^2 "
          f"(outer {outer.total_area_px * px_area:.0f}, inner {inner.total_area_px * px_area:.0f})")

    lib = L.contoursToGDSII(polygons, layer=1, name="TOP")
    cell = lib.structures["TOP"]
    for layer, polys in ((2, nominal_nm), (3, outer_nm), (4, inner_nm)):
        part = L.contoursToGDSII(polys, layer=layer, tolerance_nm=a.tolerance, name="TOP")
        cell.elements += part.structures["TOP"].elements
    LY.writeGDSII(lib, a.out)
    back = LY.readGDSII(a.out)
    print(f"{a.out}: target on layer 1, nominal contour on layer 2, PV band on layers 3 (outer) and 4 (inner); "
          f"{len(back.structures['TOP'].elements)} boundaries")


if __name__ == "__main__":
    main()
