"""One dense line/space grating near the resolution limit at NA 1.35 in water, imaged through one mask with the scalar model and
with x, y, TE, TM and unpolarised light: image contrast and the printed line width (sub-pixel CD) of each, on one MI355X.

    python examples/vector_contrast.py [--pn 64] [--pixel 25] [--pitch 5] [--na 1.35] [--index 1.44] [--threshold 0.3]

Default: vertical lines on a 125 nm pitch (in the project's 193 nm / 25 nm-pixel units), an x dipole (sigma 0.6-0.9, +-17 degrees),
so the image is two beams that meet at about 2 x 49 degrees.  TE light (y-polarised at the poles) keeps the scalar model's
contrast; TM light loses it as cos 2 theta; unpolarised light is their mean.  The classic outcome is TE > unpolarised > TM.
Every setting is factored at full rank (vectorSocsKernels; K is printed), so the figures carry no truncation error."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lithographysimulator_amd as L                                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=64)
    ap.add_argument("--pixel", type=float, default=25.0)
    ap.add_argument("--pitch", type=int, default=5, help="grating pitch in pixels (lines are half of it, rounded down)")
    ap.add_argument("--na", type=float, default=1.35)
    ap.add_argument("--index", type=float, default=1.44, help="refractive index of the image medium (water at 193 nm)")
    ap.add_argument("--threshold", type=float, default=0.3, help="resist threshold as a fraction of the clear-field intensity")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, pn = 193.0, a.pn
    cols = torch.arange(pn)
    geo = (cols % a.pitch < a.pitch // 2)[None, :].expand(pn, pn).to(torch.int16).contiguous()
    mask = L.Mask(geo, a.pixel, dev)
    open_field = L.Mask(torch.ones((pn, pn), dtype=torch.int16), a.pixel, dev)
    eps, N = mask.calculateEpsilonN(4 / pn, a.pixel, wl)
    k = (torch.arange(pn, dtype=torch.float64) - pn // 2) * 4.0 / pn
    sx, sy = k[None, :].expand(pn, pn), k[:, None].expand(pn, pn)
    ring = L.LightSource(0.6, 0.9, pn, 0.7, device=dev).generateAnnular()
    source = (ring.cpu() != 0) & (sy.abs() <= 0.3 * sx.abs())                            # the two poles on the x axis
    pupil = L.Pupil(pn, wl, 0.7, None, dev).generatePupilFunction()
    S = int(source.sum())
    sigma_f = 4.0 * N / (a.pitch * pn)
    sin_t = a.na * sigma_f / (2 * a.index)
    print(f"{a.pitch * a.pixel:g} nm pitch: first orders at sigma {sigma_f:.3f}, {S} source points, FFT size {N}; NA {a.na} in index "
          f"{a.index}: symmetric two-beam half-angle asin({sin_t:.3f})")
    settings = {"scalar": L.socsKernels(pupil, source.to(dev), kernels=S, oversample=0)}
    for mode in ("x", "y", "te", "tm", "unpolarized"):
        settings[mode] = L.vectorSocsKernels(pupil, source.to(dev), a.na, polarization=mode, mediumIndex=a.index, kernels=5 * S,
                                             oversample=0)
    contrasts = {}
    for name, socs in settings.items():
        level = float(L.hopkinsImage(open_field, open_field.fraunhofer(wl, True), socs, a.pixel, mask.deltaK, wl)[pn // 2, pn // 2])
        image = L.hopkinsImage(mask, mask.fraunhofer(wl, True), socs, a.pixel, mask.deltaK, wl) / level
        n = image.shape[0]
        row = image[n // 2, n // 2 - 2 * a.pitch:n // 2 + 2 * a.pitch]
        contrasts[name] = float((row.max() - row.min()) / (row.max() + row.min()))
        col = n // 2 - 2 * a.pitch + int(row.argmax())                                    # the brightest line near the centre
        cd = float(L.measureCD(image, a.threshold, [(n // 2, col, 0)], a.pixel, exposed=True)[0, 0, 0, 0])
        printed = f"bright line {cd:6.1f} nm wide" if 0 < cd < a.pitch * a.pixel else "grating not resolved at this threshold"
        print(f"{name:12s}: K {socs.K:3d}  contrast {contrasts[name]:.3f}  (min {float(row.min()):.3f} max {float(row.max()):.3f} of the "
              f"clear field)  {printed}")
    order = sorted(("te", "unpolarized", "tm"), key=lambda m: -contrasts[m])
    print("contrast order: " + " > ".join(order))


if __name__ == "__main__":
    main()
