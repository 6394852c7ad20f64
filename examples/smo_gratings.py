"""Source optimisation and the alternating source-mask loop on a dense grating, on one MI355X.

    python examples/smo_gratings.py [--pn 64] [--pixel 25] [--pitch 8] [--iterations 20] [--rounds 2]

A vertical line-space grating near the resolution limit (pitch 8 pixels of 25 nm = 200 nm at 193 nm, NA 0.7: k1 = 0.36) under a
conventional disc of candidate source points (sigma <= 0.9).  Only the source points whose shifted pupil passes both the zeroth
and one first diffraction order form the grating's image; the rest add background, and at a threshold of 0.45 of the clear field
the uniform disc does not print the lines.  optimizeSource descends the weights of the candidates with optimizeMask's loss, and
the weight moves into the two poles along the grating's frequency axis (the x axis of the source): the script prints the loss
before and after and the share of the total weight inside the two poles, then runs two rounds of optimizeSourceMask from the
drawn mask.  Saves nothing."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lithographysimulator_amd as L                                     # noqa: E402


def pole_share(source, pn, na, wl, pixel, pitch):
    """Share of the total weight in the two poles: the source pixels from which a first diffraction order falls inside the pupil
    next to the zeroth, (|sigma_x| - f)^2 + sigma_y^2 <= 1 with f = lambda / (pitch NA) the order spacing in pupil radii -- two
    lenses centred near sigma_x = +-f / 2.  The source grid spans sigma in [-2, 2) (4 / pn per pixel), x along the columns."""
    f = wl / (pitch * pixel * na)
    s = (torch.arange(pn, dtype=torch.float32, device=source.device) - pn // 2) * (4.0 / pn)
    sy, sx = s[:, None], s[None, :]
    poles = (sx.abs() - f) ** 2 + sy ** 2 <= 1.0
    return float(source[poles].sum() / source.sum()), float(poles.float().mean()), f / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=64)
    ap.add_argument("--pixel", type=float, default=25.0)
    ap.add_argument("--pitch", type=int, default=8, help="grating pitch in pixels")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.45, help="fraction of the clear-field intensity")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na, pn = 193.0, 0.7, a.pn
    cols = (torch.arange(pn) % a.pitch) < a.pitch // 2
    geometry = cols[None, :].expand(pn, pn).to(torch.int16).contiguous()
    mask = L.Mask(geometry, a.pixel, dev)
    deltaK = mask.deltaK
    pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
    disc = L.LightSource(0.0, 0.9, pn, na, device=dev).generateAnnular()
    open_mask = L.Mask(torch.ones((pn, pn), dtype=torch.int16), a.pixel, dev)
    clear = L.abbeImage(open_mask, open_mask.fraunhofer(wl, True), pupil, disc, a.pixel, deltaK, wl, True, dev, normalize=True)
    n_out = clear.shape[-1]
    threshold = a.threshold * float(clear[n_out // 2, n_out // 2])
    target = torch.zeros((n_out, n_out), dtype=torch.float32, device=dev)
    k = min(pn, n_out)
    target[:k, :k] = geometry[:k, :k].to(dev).float()

    res = L.optimizeSource(target, geometry.to(dev).to(torch.complex64), pupil, disc, a.pixel, deltaK, wl, threshold,
                           iterations=a.iterations)
    before, area, sigma0 = pole_share(disc.to(torch.float32), pn, na, wl, a.pixel, a.pitch)
    after, _, _ = pole_share(res.source, pn, na, wl, a.pixel, a.pitch)
    print(f"{int(disc.sum())} candidate source points, pitch {a.pitch * a.pixel:.0f} nm, poles at sigma = +-{sigma0:.2f}")
    print(f"optimizeSource, {a.iterations} iterations: loss {res.losses[0]:.5f} -> {res.losses[res.best]:.5f} (iterate {res.best})")
    print(f"share of the total weight inside the two poles: {before:.3f} (uniform disc) -> {after:.3f}; "
          f"{int((res.source > 0).sum())} points keep a weight")

    theta0 = torch.where(geometry.to(dev) > 0, 1.0, -1.0).to(torch.float32)
    src, ilt = L.optimizeSourceMask(target, pupil, disc, a.pixel, deltaK, wl, threshold, rounds=a.rounds, kernels=24,
                                    sourceIterations=a.iterations, maskIterations=a.iterations, initialTheta=theta0)
    share, _, _ = pole_share(src.source, pn, na, wl, a.pixel, a.pitch)
    print(f"optimizeSourceMask, {a.rounds} rounds: last source stage {src.losses[0]:.5f} -> {src.losses[src.best]:.5f}, last mask stage "
          f"{ilt.losses[0]:.5f} -> {ilt.losses[ilt.best]:.5f}; weight inside the poles {share:.3f}")


if __name__ == "__main__":
    main()
