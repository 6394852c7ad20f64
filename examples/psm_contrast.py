"""One sub-resolution grating as a binary mask, as a 6 % attenuated phase-shift mask and as an alternating-aperture mask:
image contrast and the printed line width (sub-pixel CD) of each, on one MI355X.

    python examples/psm_contrast.py [--pn 64] [--pixel 25] [--pitch 6] [--sigma 0.3] [--threshold 0.3]

Default: 75 nm lines on a 150 nm pitch at 193 nm, NA 0.7, a small conventional source.  The binary mask's first orders
fall outside the pupil (nothing but the zero order gets through: no image); the alternating mask halves the frequency
of its orders and resolves the grating; the attenuated mask sits in between."""
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
    ap.add_argument("--pitch", type=int, default=6, help="grating pitch in pixels (lines are half of it)")
    ap.add_argument("--sigma", type=float, default=0.3, help="outer radius of the conventional source")
    ap.add_argument("--threshold", type=float, default=0.3, help="resist threshold as a fraction of the clear-field intensity")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na, pn = 193.0, 0.7, a.pn
    cols = torch.arange(pn)
    clear = cols % a.pitch < a.pitch // 2
    geo = clear[None, :].expand(pn, pn).to(torch.int16).contiguous()                      # full-height vertical lines
    shifter = (clear & ((cols // a.pitch) % 2 == 1))[None, :].expand(pn, pn).to(torch.int16).contiguous()
    masks = {
        "binary": L.Mask(geo, a.pixel, dev),
        "attenuated 6 %": L.Mask(pixelSize=a.pixel, device=dev, transmission=L.attenuatedPSM(geo, 0.06)),
        "alternating": L.Mask(pixelSize=a.pixel, device=dev, transmission=L.alternatingPSM(geo, shifter)),
    }
    source = L.LightSource(0.0, a.sigma, pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
    shifts = L.sourceShifts(source, pn)
    eps, N = masks["binary"].calculateEpsilonN(4 / pn, a.pixel, wl)
    open_field = L.Mask(torch.ones((pn, pn), dtype=torch.int16), a.pixel, dev)
    level = float(L.abbeIntensity(open_field.fraunhofer(wl, True), pupil, shifts, N)[pn // 2, pn // 2])
    print(f"{a.pitch * a.pixel:g} nm pitch, {wl:g} nm, NA {na}, sigma {a.sigma}: {shifts.shape[0]} source points, FFT size {N}")
    for name, mask in masks.items():
        image = L.postProcess(L.abbeIntensity(mask.fraunhofer(wl, True), pupil, shifts, N), eps) / level
        n = image.shape[0]
        row = image[n // 2, n // 2 - 2 * a.pitch:n // 2 + 2 * a.pitch]
        contrast = float((row.max() - row.min()) / (row.max() + row.min()))
        col = n // 2 - 2 * a.pitch + int(row.argmax())                                    # the brightest line near the centre
        cd = float(L.measureCD(image, a.threshold, [(n // 2, col, 0)], a.pixel, exposed=True)[0, 0, 0, 0])
        printed = f"bright line {cd:6.1f} nm wide" if 0 < cd < a.pitch * a.pixel else "grating not resolved at this threshold"
        print(f"{name:15s}: contrast {contrast:.3f}  (min {float(row.min()):.3f} max {float(row.max()):.3f} of the clear field)  {printed}")


if __name__ == "__main__":
    main()
