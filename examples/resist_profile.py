"""The resist profile of a dense grating: the line/space pattern of examples/film_swing.py imaged at 8 depths inside the resist,
with and without a bottom anti-reflective coating (BARC), exposed (Dill C), developed with Mack's rate model and measured, on
one MI355X.

    python examples/resist_profile.py [--pn 32] [--pixel 25] [--pitch 5] [--thickness 120] [--depths 8] [--dose 1.0]
                                      [--time 15] [--sigma-z 20]

For each stack it prints the width of the developed space per depth (measureCD on the planes of the arrival time T, threshold =
the development time), the side-wall angles, the top loss (how much of the unexposed line's top is developed away) and whether
the space clears to the substrate, once without and once with vertical diffusion of the latent image (a post-exposure bake;
--sigma-z, no flux through the layer faces).  On bare silicon the standing wave has a node in the middle of the resist where
space and line are equally dark: without vertical diffusion the developer stops there, with it the space clears but keeps a
waist at the node.  The BARC weakens the standing wave: the space clears either way, its width scallops with depth (it is not
monotonic) without vertical diffusion and tapers smoothly to a foot with it.  "scallop" is the largest distance of CD(z) from its
least-squares line."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lithographysimulator_amd as L                                     # noqa: E402

RESIST, BARC, SILICON = (1.70, 0.02), (1.82, 0.34, 40.0), (0.88, 2.78)
WL = 193.0


def film(thickness, barc):
    return L.FilmStack([RESIST + (thickness,)] + ([BARC] if barc else []), SILICON, resist=0)


def grating_image(dev, stack, D, pn=32, pixel=25.0, pitch=5, na=1.35, index=1.44):
    """The unpolarised image of the grating at the D midpoint depths of `stack`'s resist, fp32 [D, n, n], in units of the
    clear-field intensity averaged over the depth."""
    geo = (torch.arange(pn) % pitch < pitch // 2)[None, :].expand(pn, pn).to(torch.int16).contiguous()
    mask = L.Mask(geo, pixel, dev)
    open_field = L.Mask(torch.ones((pn, pn), dtype=torch.int16), pixel, dev)
    k = (torch.arange(pn, dtype=torch.float64) - pn // 2) * 4.0 / pn
    sx, sy = k[None, :].expand(pn, pn), k[:, None].expand(pn, pn)
    ring = L.LightSource(0.6, 0.9, pn, 0.7, device=dev).generateAnnular()
    source = ((ring.cpu() != 0) & (sy.abs() <= 0.3 * sx.abs())).to(dev)                    # the two poles on the x axis
    pupil = L.Pupil(pn, WL, 0.7, None, dev).generatePupilFunction()
    kernels = L.vectorSocsKernels(pupil, source, na, polarization="unpolarized", kernels=5 * int(source.sum()), film=stack,
                                  depths=stack.depths(D), mediumIndex=index, wavelength=WL, oversample=0)
    image = L.hopkinsImage(mask, mask.fraunhofer(WL, True), kernels, pixel, mask.deltaK, WL)
    clear = L.hopkinsImage(open_field, open_field.fraunhofer(WL, True), kernels, pixel, mask.deltaK, WL)
    return (image / clear.mean()).contiguous()


def scallop(z, cd):
    """Largest distance of CD(z) from its least-squares line, nm."""
    ok = cd > 0
    if ok.sum() < 3:
        return float("nan")
    fit = np.polyval(np.polyfit(z[ok], cd[ok], 1), z[ok])
    return float(np.abs(cd[ok] - fit).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=32)
    ap.add_argument("--pixel", type=float, default=25.0)
    ap.add_argument("--pitch", type=int, default=5, help="grating pitch in pixels (lines are half of it, rounded down)")
    ap.add_argument("--thickness", type=float, default=120.0, help="resist thickness, nm")
    ap.add_argument("--depths", type=int, default=8, help="planes through the resist")
    ap.add_argument("--dose", type=float, default=1.0)
    ap.add_argument("--time", type=float, default=15.0, help="development time, s")
    ap.add_argument("--sigma-z", type=float, default=20.0, help="vertical diffusion length of the latent image, nm")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    D = a.depths
    print(f"{a.pitch * a.pixel:g} nm pitch, {a.thickness:g} nm of resist at {D} depths, dose {a.dose:g}, {a.time:g} s of development; "
          "Mack: r_max 100, r_min 0.05 nm/s, q 15, m_th 0.2, C 4; lateral diffusion 5 nm")
    for barc in (False, True):
        stack = film(a.thickness, barc)
        z = np.array(stack.depths(D))
        image = grating_image(dev, stack, D, a.pn, a.pixel, a.pitch)
        n = image.shape[-1]
        print(f"-- {'with' if barc else 'without'} BARC: intensity through the depth at the space centre / the line centre")
        row = n // 2
        seg = image[:, row, n // 2 - a.pitch:n // 2 + a.pitch]
        print("   " + "  ".join(f"{float(seg[d].max()):.2f}/{float(seg[d].min()):.2f}" for d in range(D)))
        for sigma_z in (0.0, a.sigma_z):
            resist = L.MackResist(C=4.0, rMax=100.0, rMin=0.05, q=15.0, mTh=0.2, diffusionLength=5.0, verticalDiffusionLength=sigma_z)
            prof = L.resistProfile(image, resist, stack, a.pixel, a.time, doses=(a.dose,))
            T0 = prof.T[0, 0, 0, row, n // 2 - a.pitch:n // 2 + a.pitch]
            c_space = n // 2 - a.pitch + int(torch.argmin(T0))
            c_line = n // 2 - a.pitch + int(torch.argmax(T0))
            cd = prof.cd([(row, c_space, 0)])[0, :, 0, 0].cpu().numpy().astype(np.float64)
            angle = prof.sidewallAngle((row, c_space, 0))[0, 0]
            depth = prof.depth[0, 0, row]
            print(f"   sigma_z {sigma_z:4.1f} nm ({prof.launches} solver launches): space CD per depth (nm)  "
                  + " ".join(f"{v:6.1f}" for v in cd))
            print(f"      scallop {scallop(z, cd):.2f} nm; side-wall angles {angle[0]:.1f} / {angle[1]:.1f} deg; top loss "
                  f"{float(depth[c_line]):.1f} nm; the space is developed to {float(depth[c_space]):.1f} of {a.thickness:g} nm"
                  + (" (cleared)" if float(depth[c_space]) >= a.thickness else ""))


if __name__ == "__main__":
    main()
