"""A dense grating at NA 1.35 in water imaged INTO a resist film on silicon, with and without a bottom anti-reflective coating
(BARC), on one MI355X: contrast of the depth-averaged (bulk) image for TE, TM and unpolarised light, the standing wave through
the depth, and the swing curve of the bulk dose over resist thickness.

    python examples/film_swing.py [--pn 32] [--pixel 25] [--pitch 5] [--na 1.35] [--index 1.44] [--thickness 120] [--depths 8]

The stack is water / resist (n 1.70, k 0.02) / [BARC (n 1.82, k 0.34), 40 nm] / silicon (n 0.88, k 2.78).  The film stack changes
only the six pupil planes (filmPupils); everything downstream is the vector Hopkins code as it was.  The bulk image
sum_d w_d I(z_d) over the midpoints of `depths` equal slabs comes from ONE kernel set (vectorSocsKernels(depthWeights=)): K fields
per image, not depths x K -- the example prints how far it is from the mean of the per-depth images.  The swing curve is the
clear-field bulk dose against resist thickness for the centre point of a conventional source, whose period is
lambda / (2 n_resist) at normal incidence (the finite field's spectrum spreads over neighbouring pupil cells, which see a
slightly longer period: half a per cent here); the BARC flattens it."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lithographysimulator_amd as L                                     # noqa: E402

RESIST, BARC, SILICON = (1.70, 0.02), (1.82, 0.34, 40.0), (0.88, 2.78)


def film(thickness, barc):
    return L.FilmStack([RESIST + (thickness,)] + ([BARC] if barc else []), SILICON, resist=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=32)
    ap.add_argument("--pixel", type=float, default=25.0)
    ap.add_argument("--pitch", type=int, default=5, help="grating pitch in pixels (lines are half of it, rounded down)")
    ap.add_argument("--na", type=float, default=1.35)
    ap.add_argument("--index", type=float, default=1.44, help="refractive index of the medium above the stack (water at 193 nm)")
    ap.add_argument("--thickness", type=float, default=120.0, help="resist thickness, nm")
    ap.add_argument("--depths", type=int, default=8, help="depth samples through the resist")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, pn, D = 193.0, a.pn, a.depths
    cols = torch.arange(pn)
    geo = (cols % a.pitch < a.pitch // 2)[None, :].expand(pn, pn).to(torch.int16).contiguous()
    mask = L.Mask(geo, a.pixel, dev)
    open_field = L.Mask(torch.ones((pn, pn), dtype=torch.int16), a.pixel, dev)
    eps, N = mask.calculateEpsilonN(4 / pn, a.pixel, wl)
    k = (torch.arange(pn, dtype=torch.float64) - pn // 2) * 4.0 / pn
    sx, sy = k[None, :].expand(pn, pn), k[:, None].expand(pn, pn)
    ring = L.LightSource(0.6, 0.9, pn, 0.7, device=dev).generateAnnular()
    source = ((ring.cpu() != 0) & (sy.abs() <= 0.3 * sx.abs())).to(dev)                    # the two poles on the x axis
    pupil = L.Pupil(pn, wl, 0.7, None, dev).generatePupilFunction()
    S = int(source.sum())
    mft, oft = mask.fraunhofer(wl, True), open_field.fraunhofer(wl, True)
    weights = [1.0 / D] * D
    optics = dict(mediumIndex=a.index, wavelength=wl, oversample=0)

    print(f"{a.pitch * a.pixel:g} nm pitch, x dipole of {S} points, NA {a.na} in index {a.index}, {a.thickness:g} nm of resist, "
          f"{D} depths; bulk image = one kernel set per setting")
    for barc in (False, True):
        stack = film(a.thickness, barc)
        depths = stack.depths(D)
        print(f"-- {'with' if barc else 'without'} BARC")
        for mode in ("te", "tm", "unpolarized"):
            # The rank bound (3 or 5) S per depth, D times that for the bulk operator -- but never more vectors than the grid
            # has room for: beyond the dimension of the kernels' support the subspace iteration has nothing left to span.
            rank = (5 if mode == "unpolarized" else 3) * S
            bulk = L.vectorSocsKernels(pupil, source, a.na, polarization=mode, kernels=min(rank * D, pn * pn // 2), film=stack,
                                       depths=depths, depthWeights=weights, **optics)
            level = float(L.hopkinsImage(open_field, oft, bulk, a.pixel, mask.deltaK, wl)[pn // 2, pn // 2])
            image = L.hopkinsImage(mask, mft, bulk, a.pixel, mask.deltaK, wl) / level
            n = image.shape[0]
            row = image[n // 2, n // 2 - 2 * a.pitch:n // 2 + 2 * a.pitch]
            contrast = float((row.max() - row.min()) / (row.max() + row.min()))
            line = f"{mode:12s}: bulk K {bulk.K:4d}  contrast {contrast:.3f}  captured {bulk.captured:.6f}"
            if mode == "unpolarized":
                per = L.vectorSocsKernels(pupil, source, a.na, polarization=mode, kernels=rank, film=stack, depths=depths, **optics)
                raw = L.hopkinsIntensity(mft, per, N)
                mean = sum(w * raw[d] for d, w in enumerate(weights))
                one = L.hopkinsIntensity(mft, bulk, N)
                line += f"  (bulk vs mean of {D} per-depth images: {float((one - mean).abs().max() / mean.max()):.1e} of the maximum)"
                clear = L.hopkinsIntensity(oft, per, N).mean(dim=(1, 2))
                wave = "  ".join(f"{z:5.1f}: {float(v / clear.mean()):.3f}" for z, v in zip(depths, clear))
            print(line)
        print(f"clear-field intensity against depth (nm below the resist top, relative to its mean), unpolarised:\n  {wave}")

    # swing curve: clear field, the centre point of a conventional source, bulk dose against resist thickness
    centre = torch.zeros((pn, pn), dtype=torch.float32, device=dev)
    centre[pn // 2, pn // 2] = 1.0
    step = 3.0
    thicknesses = [80.0 + step * i for i in range(61)]
    print(f"swing curve: clear-field bulk dose, on-axis source point, resist {thicknesses[0]:g} ... {thicknesses[-1]:g} nm")
    for barc in (False, True):
        dose = []
        for t in thicknesses:
            stack = film(t, barc)
            bulk = L.vectorSocsKernels(pupil, centre, a.na, polarization="unpolarized", kernels=5 * D, film=stack, depths=stack.depths(D),
                                       depthWeights=weights, **optics)
            dose.append(float(L.hopkinsIntensity(oft, bulk, N).mean()))
        peaks = []
        for i in range(1, len(dose) - 1):
            if dose[i] > dose[i - 1] and dose[i] >= dose[i + 1]:                              # parabola through three samples
                lo, mid, hi = dose[i - 1], dose[i], dose[i + 1]
                peaks.append(thicknesses[i] + step * 0.5 * (lo - hi) / (lo - 2.0 * mid + hi))
        swing = (max(dose) - min(dose)) / (sum(dose) / len(dose))
        tag = "with BARC   " if barc else "without BARC"
        print(f"  {tag}: swing (max - min) / mean {swing:.3f}; maxima at " + ", ".join(f"{p:.1f}" for p in peaks) + " nm")
        print("    " + " ".join(f"{v / max(dose):.2f}" for v in dose[::3]))
        if not barc and len(peaks) > 1:
            period, want = (peaks[-1] - peaks[0]) / (len(peaks) - 1), wl / (2.0 * RESIST[0])
            print(f"    period {period:.2f} nm; lambda / (2 n_resist) = {want:.2f} nm; off by {100.0 * abs(period / want - 1.0):.2f} %")


if __name__ == "__main__":
    main()
