"""Aberration retrieval from through-focus aerial images of a known mask, on one MI355X.

    python examples/aberration_fit.py [--pn 64] [--pixel 20] [--iterations 20] [--step 0.02]

A scanner with a little coma, astigmatism and spherical aberration (Zernike terms OSA 8, 5 and 12, a few hundredths of a wave)
images a seeded attenuated phase-shift mask under an annular source at three defocus planes.  Those three images are the
measurement; fitAberrations starts from a perfect lens and descends the coefficients with the pupil gradient (one forward and one
adjoint field per source point and iterate, litho_pupil_vjp) until its model images match.  Prints the truth, the recovered
coefficients, the losses and, for the start, the sensitivities dl/dc_j of aberrationGradient.  An odd term such as coma needs an
asymmetric pattern or defocus to show in the image; the even terms separate through focus.  Saves nothing."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lithographysimulator_amd as L                                     # noqa: E402
from lithographysimulator_amd.synthetic import bernoulli_mask            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=64)
    ap.add_argument("--pixel", type=float, default=20.0)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--step", type=float, default=0.02, help="first step length in waves")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na, pn = 193.0, 0.7, a.pn
    terms, truth = (5, 8, 12), torch.tensor([0.02, 0.03, -0.02], device=dev)
    defocus = torch.tensor([-0.15, 0.0, 0.15], device=dev)                  # waves of Z4 per plane
    transmission = L.attenuatedPSM(bernoulli_mask(pn)).to(dev)
    mask = L.Mask(transmission=transmission, pixelSize=a.pixel, device=dev)
    epsilon, N = mask.calculateEpsilonN(mask.deltaK, a.pixel, wl)
    M = mask.fraunhofer(wl, True)
    source = L.LightSource(0.4, 0.8, pn, na, device=dev).generateAnnular().to(torch.float32)
    shifts, weights = L.sourceShifts(source != 0, pn), source[source != 0].contiguous()
    basis = L.zernikeBasis(terms, pn, dev)
    base = defocus[:, None, None] * L.zernikeBasis((4,), pn, dev)

    def pupils(c):
        return torch.stack([L.generatePhi(W, pn, dev) for W in base + torch.tensordot(c, basis, dims=1)])

    def image(c):
        return L.postProcess(L.abbeIntensity(M, pupils(c), shifts, N, weights=weights) / float(weights.sum()), epsilon)

    measured = image(truth)
    # the sensitivities at the start, through the explicit calls the loop is made of
    c0 = torch.zeros(len(terms), device=dev)
    diff = image(c0) - measured
    G = L.postProcessAdjoint(2.0 * diff / diff.numel(), pn, epsilon) / float(weights.sum())
    P0 = pupils(c0)
    sens = L.aberrationGradient(L.pupilGradient(M, P0, shifts, N, G, weights=weights), P0, basis)
    res = L.fitAberrations(measured, transmission, source, basis, a.pixel, mask.deltaK, wl, baseWavefront=base, iterations=a.iterations,
                           step=a.step)
    print(f"pn {pn}, {shifts.shape[0]} source points, {len(defocus)} planes, Zernike terms (OSA) {terms}")
    print(f"dl/dc at a perfect lens: {['%.4e' % v for v in sens.tolist()]}")
    print(f"truth      {['%+.4f' % v for v in truth.tolist()]} waves")
    print(f"recovered  {['%+.4f' % v for v in res.coefficients.tolist()]} waves (iterate {res.best} of {len(res.losses) - 1})")
    print(f"losses     {['%.3e' % v for v in res.losses]}")
    print(f"steps      {['%.4g' % v for v in res.steps]}")


if __name__ == "__main__":
    main()
