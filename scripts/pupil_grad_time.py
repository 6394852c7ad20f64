"""Times the pupil-gradient path on one MI355X, warm, with device events, in one process:

    timeout -k 10 600 python scripts/pupil_grad_time.py [--repeats 5]

pupilGradient (litho_pupil_vjp) on the lists of scripts/source_grad_time.py -- the full list of the benchmark's 256^2 source (annular
0-0.5: 3,233 points) and a 4,096-point sub-list of the quasar 0.4-0.8 source at 2048^2 (a defocused pupil, 25 nm pixels at 193 nm, a
seeded Bernoulli mask) -- and, as yardsticks in the same run on the same list, sourceSensitivities and one abbeIntensity.  Before
timing, the identity the gradient rests on is cross-checked on the timed inputs: Re <g, P> against 2 <G, abbeIntensity(weights=w)>.
Printed: microseconds per source point for the three, the ratios, and the bytes the passes of the pupil gradient must move per point
against the 4.1 TB/s the project has measured: the forward field (pupil read and field written, an in-place transpose, a row pass
in place, a transpose: 16 + 16 + 16 + 16 = 64 pn^2 bytes), the adjoint (the same with the field and G read: 68 pn^2) and the
reducing pass (the adjoint read once: 8 pn^2; grad read and written once per chunk, the mask spectrum from cache) -- 140 pn^2 per
point, what litho_socs_vjp moves per kernel (148 pn^2: its reducing pass reads the kernel too) and 3.2 times a source sensitivity.
aberrationGradient (litho_pupil_project) with 37 terms is timed once per size as well.  The figures go into LABNOTES.md."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lithographysimulator_amd as L                                     # noqa: E402
from lithographysimulator_amd.synthetic import bernoulli_mask            # noqa: E402

MEASURED_BANDWIDTH = 4.1e12      # bytes / s, the project's measured streaming rate (LABNOTES)
BYTES_PER_CELL = 64 + 68 + 8     # see the head of the file


def events(fn, repeats, warm=2):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeats                                       # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na, ps = 193.0, 0.7, 25.0
    for pn, kind, limit in ((256, "annular", None), (2048, "quasar", 4096)):
        src = L.LightSource(0.0, 0.5, pn, na, device=dev) if kind == "annular" else L.LightSource(0.4, 0.8, pn, na, device=dev)
        bitmap = src.generateAnnular() if kind == "annular" else src.generateQuasar(4, -math.pi / 8)
        sh = L.sourceShifts(bitmap, pn)
        total = sh.shape[0]
        if limit is not None:
            sh = sh[(torch.arange(limit, device=dev) * total) // limit].contiguous()
        S = sh.shape[0]
        pupil = L.Pupil(pn, wl, na, torch.tensor([0, 0, 0, 0, 30], dtype=torch.float16), dev).generatePupilFunction()
        mask = L.Mask(bernoulli_mask(pn), ps, dev)
        _, N = mask.calculateEpsilonN(mask.deltaK, ps, wl)
        M = mask.fraunhofer(wl, True)
        gen = torch.Generator(device=dev).manual_seed(1)
        G = torch.randn((pn, pn), generator=gen, dtype=torch.float32, device=dev)
        w = 0.25 + torch.rand(S, generator=gen, dtype=torch.float32, device=dev)
        image = L.abbeIntensity(M, pupil, sh, N, weights=w)
        g = L.pupilGradient(M, pupil, sh, N, G, weights=w)
        lhs = float((g.real.double() * pupil.real.double() + g.imag.double() * pupil.imag.double()).sum())
        rhs = 2.0 * float((G.double() * image.double()).sum())
        scale = 2.0 * float((G.double().abs() * image.double()).sum())
        print(f"pn {pn} N {N} {kind} {S} of {total} points: Re<g, P> {lhs:.6e}, 2<G, I_w> {rhs:.6e}, difference {abs(lhs - rhs) / scale:.1e} "
              f"of 2 sum |G| I_w", flush=True)
        plan = L.PlanCache()
        t_fwd = events(lambda: L.abbeIntensity(M, pupil, sh, N, plan=plan), a.repeats)
        t_sens = events(lambda: L.sourceSensitivities(M, pupil, sh, N, G), a.repeats)
        t_grad = events(lambda: L.pupilGradient(M, pupil, sh, N, G, weights=w), a.repeats)
        per_point = t_grad * 1e3 / S
        bytes_point = float(BYTES_PER_CELL) * pn * pn
        floor_us = bytes_point / MEASURED_BANDWIDTH * 1e6
        print(f"pn {pn} N {N}: pupilGradient {t_grad:.3f} ms = {per_point:.3f} us per source point; sourceSensitivities {t_sens:.3f} ms = "
              f"{t_sens * 1e3 / S:.3f} us per point; abbeIntensity {t_fwd:.3f} ms = {t_fwd * 1e3 / S:.3f} us per point; one gradient = "
              f"{t_grad / t_fwd:.2f} forward images = {t_grad / t_sens:.2f} source gradients; the passes move {bytes_point / 1e6:.2f} MB "
              f"per point = {floor_us:.3f} us at 4.1 TB/s ({bytes_point / (per_point * 1e-6) / 1e12:.2f} TB/s achieved)", flush=True)
        basis = L.zernikeBasis(range(37), pn, dev)
        t_proj = events(lambda: L.aberrationGradient(g, pupil, basis), a.repeats)
        print(f"pn {pn}: aberrationGradient, 37 terms, {t_proj * 1e3:.1f} us per call ({(16 * 3 + 37 * 4) * pn * pn / (t_proj * 1e-3) / 1e12:.2f} "
              f"TB/s over the gradient and the pupil read once per tile of 16 terms and the basis once)", flush=True)


if __name__ == "__main__":
    main()
