"""Inverse lithography against a chemically amplified resist on one MI355X: the dense grating of examples/resist_profile.py imaged
at a few depths inside 120 nm of resist on bare silicon, the mask optimised once against the constant-threshold resist that
optimizeMask has by default and once through the post-exposure bake (bakedResistModel: exposure, acid-quencher
reaction-diffusion, the inhibitor that development thresholds), without and with base quencher.

    python examples/ilt_baked_resist.py [--pn 32] [--pixel 25] [--pitch 5] [--thickness 120] [--depths 4] [--dose 0.45]
                                        [--quencher 0.15] [--iterations 40] [--time 15] [--level 0.35]

The target is the drawn grating on the image grid (the sub-pixel registration offset of the image is ignored).  For each resist
it prints the loss of the baked-resist model (mean squared distance of the deprotection 1 - m, through a sigmoid at --level, from
the target, over all depths) before and after the descent and the cost of an iteration; then the width of the developed space per
depth (resistProfile: bake, Mack development, metrology) for the drawn mask, for the mask the threshold model finds and for the
mask the baked-resist model finds.  Development itself is not differentiated: --level is the deprotection at which the developer
all but stops within the development time (Mack's rate with q = 10, m_th = 0.5 falls below 1 nm/s near 1 - m = 0.33), which is
below 1 - m_th because the front keeps moving sideways for the whole development time."""
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
    ap.add_argument("--level", type=float, default=0.35, help="the deprotection 1 - m that the loss takes as the printing threshold")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    pn, D, bake_time = a.pn, a.depths, 60.0
    stack = film(a.thickness, False)
    geo = (torch.arange(pn) % a.pitch < a.pitch // 2)[None, :].expand(pn, pn).to(torch.int16).contiguous()
    drawn = L.Mask(geo, a.pixel, dev)
    open_field = L.Mask(torch.ones((pn, pn), dtype=torch.int16), a.pixel, dev)
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
    level, steep = a.level, 25.0 / a.level                                                   # optimizeMask's default slope

    def resist(q0):
        return L.ChemicallyAmplifiedResist(C=4.0, quencher=q0, kAmp=0.025, kQuench=5.0, kLoss=0.002, acidDiffusionLength=10.0,
                                           quencherDiffusionLength=3.0, verticalScale=1.5, bakeTime=bake_time, mack=mack)

    print(f"{a.pitch * a.pixel:g} nm pitch, {a.thickness:g} nm of resist on bare silicon at {D} depths, dose {a.dose:g} of the clear field, "
          f"{socs.K} kernels per depth; {a.iterations} iterations; {a.time:g} s of development")
    # the constant-threshold resist: the image level that dose x I must reach; the bake plays no part
    # (here: the level half way between the space centre and the line centre of the drawn mask's image, over all depths)
    I0 = image_of(geo.to(dev).to(torch.complex64))
    threshold = 0.5 * float(I0[:, row, c_space:c_space + a.pitch].amax(-1).mean() + I0[:, row, c_space:c_space + a.pitch].amin(-1).mean())
    thr, seconds = timed(lambda: L.optimizeMask(target, socs, a.pixel, deltaK, WL, threshold, iterations=a.iterations, normalize=False))
    print(f"threshold model (threshold {threshold / clear:.2f} of the clear field): loss {thr.losses[0]:.5f} -> {thr.losses[thr.best]:.5f} (iterate {thr.best}), "
          f"{seconds / (a.iterations + 1) * 1e3:.1f} ms per iteration")
    for q0 in (0.0, a.quencher):
        r = resist(q0)
        imager, adjoint = L.bakedResistModel(socs, r, stack.thickness, a.pixel, deltaK, WL, intensityScale=a.dose / clear, normalize=False)

        def loss_of(transmission):
            s = torch.sigmoid(steep * (imager(transmission) - level))
            return float(((s - target) ** 2).mean())

        res, seconds = timed(lambda: L.optimizeMask(target, socs, a.pixel, deltaK, WL, level, iterations=a.iterations, imager=imager,
                                                    adjoint=adjoint))
        print(f"-- quencher {q0:4.2f} ({L.postExposureBake(image_of(thr.transmission), r, stack.thickness, a.pixel).steps} bake steps): "
              f"baked-resist model loss {res.losses[0]:.5f} -> {res.losses[res.best]:.5f} (iterate {res.best}), "
              f"{seconds / (a.iterations + 1) * 1e3:.1f} ms per iteration; the threshold model's mask scores {loss_of(thr.transmission):.5f}")
        for name, t in (("drawn mask", geo.to(dev).to(torch.complex64)), ("threshold-model mask", thr.transmission),
                        ("baked-resist-model mask", res.transmission)):
            prof = L.resistProfile(image_of(t) / clear, r, stack, a.pixel, a.time, doses=(a.dose,))
            cd = prof.cd([(row, c_space, 0)])[0, :, 0, 0].cpu().numpy()
            print(f"   {name:24s} developed space CD per depth (nm; drawn {a.pitch // 2 * a.pixel:g}): " + " ".join(f"{v:6.1f}" for v in cd))


if __name__ == "__main__":
    main()
