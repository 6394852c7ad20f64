"""A grey-level (freeform) illuminator: Gaussian-apodised annulus -> mask -> aerial image -> resist contour, on one MI355X.

    python examples/freeform_source.py [--pn 512] [--pixel 25] [--width 0.5] [--threshold 0.3]

The reference's source is a bitmap (imageformation.py:59): every lit pixel counts once.  Here the source map holds per-point
INTENSITY weights -- the annulus 0.4 <= sigma <= 0.8 multiplied by exp(-sigma^2 / width) -- and the image is
sum_s w_s |E_s|^2 (abbeImage(..., weighted=True)).  Prints the image statistics and the printed line width on the centre row
for the apodised source and, for comparison, for the plain annulus; saves nothing."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lithographysimulator_amd as L                                     # noqa: E402
from lithographysimulator_amd.synthetic import lines_mask                # noqa: E402


def centre_width(contour, pixel):
    """Width in nm of the run of unexposed pixels through the centre of the centre row (0 if the centre is exposed)."""
    row = contour[contour.shape[0] // 2].to(torch.int32).cpu()
    c = row.shape[0] // 2
    if int(row[c]) != 0:
        return 0.0
    lo = c
    while lo > 0 and int(row[lo - 1]) == 0:
        lo -= 1
    hi = c
    while hi < row.shape[0] - 1 and int(row[hi + 1]) == 0:
        hi += 1
    return (hi - lo + 1) * pixel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=512)
    ap.add_argument("--pixel", type=float, default=25.0)
    ap.add_argument("--width", type=float, default=0.5, help="1/e width of the apodisation in sigma^2")
    ap.add_argument("--threshold", type=float, default=0.3, help="resist threshold as a fraction of the clear-field intensity")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na, pn = 193.0, 0.7, a.pn
    mask = L.Mask(lines_mask(pn), a.pixel, dev)
    mft = mask.fraunhofer(wl, True)
    eps, N = mask.calculateEpsilonN(mask.deltaK, a.pixel, wl)
    pupil = L.Pupil(pn, wl, na, torch.tensor([0, 0, 0, 0, 30], dtype=torch.float16), dev).generatePupilFunction()
    annulus = L.LightSource(0.4, 0.8, pn, na, device=dev).generateAnnular()
    sigma = (torch.arange(pn, dtype=torch.float32, device=dev) - pn // 2) * (4.0 / pn)
    apodised = torch.exp(-(sigma[:, None] ** 2 + sigma[None, :] ** 2) / a.width) * annulus.to(torch.float32)
    clear_mask = L.Mask(torch.ones((pn, pn), dtype=torch.int16), a.pixel, dev)
    clear_ft = clear_mask.fraunhofer(wl, True)
    for name, source, weighted in (("plain annulus (bitmap)", annulus, False), ("Gaussian-apodised annulus", apodised, True)):
        # normalize=True: divided by the number of source points, or by the sum of the weights -- the clear field is then
        # comparable between the two sources
        image = L.abbeImage(mask, mft, pupil, source, a.pixel, mask.deltaK, wl, True, dev, normalize=True, weighted=weighted)
        clear = L.abbeImage(clear_mask, clear_ft, pupil, source, a.pixel, mask.deltaK, wl, True, dev, normalize=True, weighted=weighted)
        level = float(clear[clear.shape[0] // 2, clear.shape[1] // 2])
        contour = (image >= a.threshold * level).to(torch.uint8)
        mid = image[image.shape[0] // 2]
        shifts, weights = L.sourceWeights(source.to(torch.float32), pn)
        print(f"{name}: {shifts.shape[0]} source points, sum of weights {float(weights.sum()):.1f}, FFT size {N}; image / clear field: "
              f"min {float(image.min()) / level:.3f} max {float(image.max()) / level:.3f}; contrast on the centre row "
              f"{float((mid.max() - mid.min()) / (mid.max() + mid.min())):.3f}; "
              f"printed line width at the centre {centre_width(contour, a.pixel):.0f} nm")


if __name__ == "__main__":
    main()
