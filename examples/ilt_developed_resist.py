"""Inverse lithography against the developed resist profile on one MI355X: the grating and film stack of
examples/ilt_baked_resist.py, the mask optimised once against the latent image after the bake (bakedResistModel: the loss sits
on the deprotection that development thresholds) and once against the developed profile itself (developedResistModel: the loss
sits on the arrival time of the development front, with the gradient carried through the front solver, the rate and the bake).

    python examples/ilt_developed_resist.py [--pn 32] [--pixel 25] [--pitch 5] [--thickness 120] [--depths 4] [--dose 0.45]
                                            [--quencher 0.15] [--iterations 40] [--time 15] [--level 0.35]

The profile model runs twice: from the drawn mask, and from the mask the latent-image model found (optimizeMask(initial=)).  A
cell that develops later than twice the development time has no gradient (the margin is clamped there), so from a drawn mask
whose spaces are far from opening the profile model has little to pull on; the latent-image model finds the basin and the
profile model refines in it.  For each run it prints the loss before and after the descent and the cost of an iteration; then,
for the drawn mask and for the optimised masks, the profile loss, the width of the developed space per depth and whether the
space clears -- that is, whether it is open at the bottom plane (ResistProfile.cd: resistProfile's bake, Mack development and
metrology).  The latent-image model needs a deprotection level chosen by hand (--level: where the developer all but stops); the
profile model needs none -- its threshold is the development time."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lithographysimulator_amd as L                                     # noqa: E402
from resist_profile import WL, film                                      # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=32)
    ap.add_argument("--pixel", type=float, default=25.0)
    ap.add_argument("--pitch", type=int, default=5, help="grating pitch in pixels (spaces are half of it, rounded down)")
    ap.add_argument("--thickness", type=float, default=120.0, help="resist thickness, nm")
    ap.add_argument("--depths", type=int, default=4, help="planes through the resist")
    ap.add_argument("--dose", type=float, default=0.45, help="exposure dose in units of the clear field")
    ap.add_argument("--quencher", type=float, default=0.15, help="base quencher relative to the PAG")
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--time", type=float, default=15.0, help="development time, s")
    ap.add_argument("--level", type=float, default=0.35, help="the deprotection 1 - m that the latent-image loss takes as the threshold")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    pn, D = a.pn, a.depths
    stack = film(a.thickness, False)
    geo = (torch.arange(pn) % a.pitch < a.pitch // 2)[None, :].expand(pn, pn).to(torch.int16).contiguous()
    drawn = L.Mask(geo, a.pixel, dev)
    deltaK = drawn.deltaK
    k = (torch.arange(pn, dtype=torch.float64) - pn // 2) * 4.0 / pn
    sx, sy = k[None, :].expand(pn, pn), k[:, None].expand(pn, pn)
    ring = L.LightSource(0.6, 0.9, pn, 0.7, device=dev).generateAnnular()
    source = ((ring.cpu() != 0) & (sy.abs() <= 0.3 * sx.abs())).to(dev)                    # the two poles on the x axis
    pupil = L.Pupil(pn, WL, 0.7, None, dev).generatePupilFunction()
    socs = L.vectorSocsKernels(pupil, source, 1.35, polarization="unpolarized", kernels=5 * int(source.sum()), film=stack,
                               depths=stack.depths(D), mediumIndex=1.44, wavelength=WL, oversample=0)

    def image_of(transmission):
        mask = L.Mask(transmission=transmission, pixelSize=a.pixel, device=dev)
        return L.hopkinsImage(mask, mask.fraunhofer(WL, True), socs, a.pixel, deltaK, WL)

    clear = float(image_of(torch.ones((pn, pn), dtype=torch.complex64, device=dev)).mean())
    n_out = image_of(geo.to(dev).to(torch.complex64)).shape[-1]
    target = torch.zeros((n_out, n_out), dtype=torch.float32, device=dev)
    m = min(pn, n_out)
    target[:m, :m] = geo[:m, :m].float().to(dev)
    row, c_space = n_out // 2, (n_out // 2 // a.pitch) * a.pitch                              # a space starts at every multiple of the pitch
    mack = L.MackResist(C=1.0, rMax=100.0, rMin=0.05, q=10.0, mTh=0.5)
    resist = L.ChemicallyAmplifiedResist(C=4.0, quencher=a.quencher, kAmp=0.025, kQuench=5.0, kLoss=0.002, acidDiffusionLength=10.0,
                                         quencherDiffusionLength=3.0, verticalScale=1.5, bakeTime=60.0, mack=mack)
    print(f"{a.pitch * a.pixel:g} nm pitch, {a.thickness:g} nm of resist on bare silicon at {D} depths, dose {a.dose:g} of the clear field, "
          f"quencher {a.quencher:g}, {socs.K} kernels per depth; {a.iterations} iterations; {a.time:g} s of development")
    common = dict(intensityScale=a.dose / clear, normalize=False)
    latent = L.bakedResistModel(socs, resist, stack.thickness, a.pixel, deltaK, WL, **common)
    profile = L.developedResistModel(socs, resist, stack.thickness, a.pixel, deltaK, WL, a.time, **common)
    lat, seconds = timed(lambda: L.optimizeMask(target, socs, a.pixel, deltaK, WL, a.level, iterations=a.iterations, imager=latent[0],
                                                adjoint=latent[1]))
    print(f"latent-image model (deprotection level {a.level:g}): loss {lat.losses[0]:.5f} -> {lat.losses[lat.best]:.5f} (iterate {lat.best}), "
          f"{seconds / (a.iterations + 1) * 1e3:.1f} ms per iteration")
    dev_res, seconds = timed(lambda: L.optimizeMask(target, socs, a.pixel, deltaK, WL, 0.0, iterations=a.iterations, imager=profile[0],
                                                    adjoint=profile[1]))
    print(f"developed-profile model (development margin, threshold 0): loss {dev_res.losses[0]:.5f} -> {dev_res.losses[dev_res.best]:.5f} "
          f"(iterate {dev_res.best}), {seconds / (a.iterations + 1) * 1e3:.1f} ms per iteration")

    refined, seconds = timed(lambda: L.optimizeMask(target, socs, a.pixel, deltaK, WL, 0.0, iterations=a.iterations, imager=profile[0],
                                                    adjoint=profile[1], initial=lat.theta))
    print(f"developed-profile model from the latent-image model's mask: loss {refined.losses[0]:.5f} -> {refined.losses[refined.best]:.5f} "
          f"(iterate {refined.best}), {seconds / (a.iterations + 1) * 1e3:.1f} ms per iteration")

    def profile_loss(transmission):
        s = torch.sigmoid(25.0 * profile[0](transmission))
        return float(((s - target) ** 2).mean())

    for name, t in (("drawn mask", geo.to(dev).to(torch.complex64)), ("latent-image-model mask", lat.transmission),
                    ("developed-profile-model mask", dev_res.transmission), ("latent, then profile model", refined.transmission)):
        prof = L.resistProfile(image_of(t) / clear, resist, stack, a.pixel, a.time, doses=(a.dose,))
        cd = prof.cd([(row, c_space, 0)])[0, :, 0, 0].cpu().numpy()
        clears = bool(cd[-1] > 0.0)
        print(f"   {name:30s} profile loss {profile_loss(t):.5f}; developed space CD per depth (nm; drawn {a.pitch // 2 * a.pixel:g}): "
              + " ".join(f"{v:6.1f}" for v in cd) + f"; the space {'clears' if clears else 'does NOT clear'}")


if __name__ == "__main__":
    main()
