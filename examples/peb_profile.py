"""A chemically amplified resist on the dense grating of examples/resist_profile.py: the line/space pattern imaged at 8 depths
inside 120 nm of resist on bare silicon (a strong standing wave), exposed, baked with the acid-quencher reaction-diffusion model
and developed, with and without base quencher, on one MI355X.

    python examples/peb_profile.py [--pn 32] [--pixel 25] [--pitch 5] [--thickness 120] [--depths 8] [--time 15]
                                   [--quencher 0.15] [--sigma 10] [--vertical 1.5]

It prints
  * the standing wave on the side wall before and after the bake: the acid the exposure releases (h0) and the acid dose the bake
    accumulates (a / bakeTime) through the depth, at the space centre and at the feature edge, with the swing
    (max - min) / (max + min) of each -- the vertical diffusion of the bake is what flattens it;
  * the width of the developed space through dose without and with quencher, at the plane where the image has the most contrast, the dose
    to size (where the space is as wide as drawn) and the slope dCD / d ln(dose) there: the quencher removes the acid below a
    dose threshold, which moves the dose to size up and changes how fast the space opens around it;
  * the profile at the dose to size of the quenched resist: CD per depth and side-wall angles."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lithographysimulator_amd as L                                     # noqa: E402
from resist_profile import film, grating_image, scallop                  # noqa: E402


def swing(column):
    """(max - min) / (max + min) of a quantity through the depth."""
    return float((column.max() - column.min()) / (column.max() + column.min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=32)
    ap.add_argument("--pixel", type=float, default=25.0)
    ap.add_argument("--pitch", type=int, default=5, help="grating pitch in pixels (lines are half of it, rounded down)")
    ap.add_argument("--thickness", type=float, default=120.0, help="resist thickness, nm")
    ap.add_argument("--depths", type=int, default=8, help="planes through the resist")
    ap.add_argument("--time", type=float, default=15.0, help="development time, s")
    ap.add_argument("--quencher", type=float, default=0.15, help="base quencher relative to the PAG")
    ap.add_argument("--sigma", type=float, default=10.0, help="acid diffusion length, nm")
    ap.add_argument("--vertical", type=float, default=1.5, help="vertical diffusion length / lateral")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    D, bake_time = a.depths, 60.0
    stack = film(a.thickness, False)
    z = np.array(stack.depths(D))
    image = grating_image(dev, stack, D, a.pn, a.pixel, a.pitch)
    n = image.shape[-1]
    row = n // 2
    seg = image.sum(0)[row, n // 2 - a.pitch:n // 2 + a.pitch]             # summed over the depth: the node planes have no contrast
    c_space, c_line = n // 2 - a.pitch + int(torch.argmax(seg)), n // 2 - a.pitch + int(torch.argmin(seg))
    best = int(torch.argmax(image[:, row, c_space] - image[:, row, c_line]))  # the plane with the most contrast
    C = 4.0
    mack = L.MackResist(C=1.0, rMax=100.0, rMin=0.05, q=10.0, mTh=0.5)

    def resist(q0):
        return L.ChemicallyAmplifiedResist(C=C, quencher=q0, kAmp=0.025, kQuench=5.0, kLoss=0.002, acidDiffusionLength=a.sigma,
                                           quencherDiffusionLength=0.3 * a.sigma, verticalScale=a.vertical, bakeTime=bake_time, mack=mack)

    print(f"{a.pitch * a.pixel:g} nm pitch, {a.thickness:g} nm of resist on bare silicon at {D} depths; C {C:g}, kAmp 0.025 /s, kQuench 5 /s, kLoss 0.002 /s, "
          f"acid sigma {a.sigma:g} nm (x {a.vertical:g} vertically), quencher sigma {0.3 * a.sigma:g} nm, {bake_time:g} s bake; "
          f"Mack r_max 100, r_min 0.05 nm/s, q 10, m_th 0.5; {a.time:g} s of development")
    c_edge = (c_space + c_line) // 2
    print(f"-- the standing wave through the depth (dose 1) at the space centre and at the feature edge (column {c_edge}), before the bake "
          "(the acid h0 the exposure releases) and after it (the accumulated acid dose a / bakeTime); swing = (max - min) / (max + min)")
    h0 = L.peb.exposeAcid(image, C)[0]
    for q0 in (0.0, a.quencher):
        bake = L.postExposureBake(image, resist(q0), stack.thickness, a.pixel)
        mean = bake.acidDose[0] / bake_time
        for name, col in (("space centre", c_space), ("feature edge", c_edge)):
            print(f"   quencher {q0:4.2f} {name}: before " + " ".join(f"{float(v):5.3f}" for v in h0[:, row, col]) + f"  swing {swing(h0[:, row, col]):.3f}")
            print("                              after  " + " ".join(f"{float(v):5.3f}" for v in mean[:, row, col]) + f"  swing {swing(mean[:, row, col]):.3f}")
    doses = [round(float(d), 3) for d in np.geomspace(0.25, 4.0, 21)]
    drawn = (a.pitch - a.pitch // 2) * a.pixel
    print(f"-- CD of the developed space at plane {best} (the most image contrast) through dose, nm (drawn: {drawn:g})")
    print("   dose          " + " ".join(f"{d:6.2f}" for d in doses))
    sized = {}
    for q0 in (0.0, a.quencher):
        prof = L.resistProfile(image, resist(q0), stack, a.pixel, a.time, doses=doses)
        cd = prof.cd([(row, c_space, 0)])[:, best, 0, 0].cpu().numpy().astype(np.float64)
        print(f"   quencher {q0:4.2f} " + " ".join(f"{v:6.1f}" for v in cd))
        above = np.nonzero(cd >= drawn)[0]
        if len(above) and above[0] > 0 and cd[above[0] - 1] > 0:
            i = above[0]
            slope = (cd[i] - cd[i - 1]) / np.log(doses[i] / doses[i - 1])
            size = doses[i - 1] * np.exp((drawn - cd[i - 1]) / slope)
            sized[q0] = (float(size), float(slope))
            print(f"      dose to size {size:.2f}; dCD / d ln(dose) there {slope:.1f} nm")
        else:
            print("      the space does not pass its drawn width inside this dose range")
    if len(sized) == 2:
        (d0, s0), (d1, s1) = sized[0.0], sized[a.quencher]
        print(f"   the quencher moves the dose to size from {d0:.2f} to {d1:.2f}; the slope there is {s1 / s0:.2f} x the unquenched one")
    dose = sized.get(a.quencher, (1.0, 0.0))[0]
    prof = L.resistProfile(image, resist(a.quencher), stack, a.pixel, a.time, doses=(dose,))
    cd = prof.cd([(row, c_space, 0)])[0, :, 0, 0].cpu().numpy().astype(np.float64)
    angle = prof.sidewallAngle((row, c_space, 0))[0, 0]
    depth = prof.depth[0, 0, row]
    print(f"-- the quenched resist at dose {dose:.2f} ({prof.launches} solver launches): space CD per depth (nm) " + " ".join(f"{v:6.1f}" for v in cd))
    print(f"      scallop {scallop(z, cd):.2f} nm; side-wall angles {angle[0]:.1f} / {angle[1]:.1f} deg; top loss {float(depth[c_line]):.1f} nm; "
          f"the space is developed to {float(depth[c_space]):.1f} of {a.thickness:g} nm" + (" (cleared)" if float(depth[c_space]) >= a.thickness else ""))


if __name__ == "__main__":
    main()
