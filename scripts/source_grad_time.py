"""Times the source-gradient path on one MI355X, warm, with device events, in one process:

    timeout -k 10 600 python scripts/source_grad_time.py [--repeats 5]

sourceSensitivities (litho_source_sensitivity) on the full list of the benchmark's 256^2 source (annular 0-0.5: 3,233 points) and on
a 4,096-point sub-list of the quasar 0.4-0.8 source at 2048^2 (ideal pupil, 25 nm pixels at 193 nm, a seeded Bernoulli mask), and as the
yardstick one abbeIntensity of the same list at the same size in the same run.  Before timing, the linearity the gradient rests on
is cross-checked on the timed inputs: <G, abbeIntensity(weights=w)> against w . sens.  Printed: microseconds per source point for
both, their ratio, the bytes the passes of the sensitivity path must move per point (one rolled pupil plane read, the field
written, transposed in place and read again, one plane of G^T: 44 pn^2 bytes; the mask spectrum stays in cache) against the
4.1 TB/s the project has measured, and from the per-point time the cost of one full-source gradient at 2048^2 (198,108
points).  The figures go into LABNOTES.md."""
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
FULL_SOURCE_2048 = 198108


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
        pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
        mask = L.Mask(bernoulli_mask(pn), ps, dev)
        _, N = mask.calculateEpsilonN(mask.deltaK, ps, wl)
        M = mask.fraunhofer(wl, True)
        gen = torch.Generator(device=dev).manual_seed(1)
        G = torch.randn((pn, pn), generator=gen, dtype=torch.float32, device=dev)
        w = 0.25 + torch.rand(S, generator=gen, dtype=torch.float32, device=dev)
        image = L.abbeIntensity(M, pupil, sh, N, weights=w)
        sens = L.sourceSensitivities(M, pupil, sh, N, G)
        lhs, rhs = float((G.double() * image.double()).sum()), float((w.double() * sens.double()).sum())
        scale = float((G.double().abs() * image.double()).sum())
        print(f"pn {pn} N {N} {kind} {S} of {total} points: <G, I_w> {lhs:.6e}, w . sens {rhs:.6e}, difference {abs(lhs - rhs) / scale:.1e} "
              f"of sum |G| I_w", flush=True)
        plan = L.PlanCache()
        t_fwd = events(lambda: L.abbeIntensity(M, pupil, sh, N, plan=plan), a.repeats)
        t_sens = events(lambda: L.sourceSensitivities(M, pupil, sh, N, G), a.repeats)
        per_point = t_sens * 1e3 / S
        bytes_point = 44.0 * pn * pn
        floor_us = bytes_point / MEASURED_BANDWIDTH * 1e6
        print(f"pn {pn} N {N}: sourceSensitivities {t_sens:.3f} ms = {per_point:.3f} us per source point; abbeIntensity {t_fwd:.3f} ms = "
              f"{t_fwd * 1e3 / S:.3f} us per point; ratio {t_sens / t_fwd:.2f} forward images; the passes move {bytes_point / 1e6:.2f} MB "
              f"per point = {floor_us:.3f} us at 4.1 TB/s ({bytes_point / (per_point * 1e-6) / 1e12:.2f} TB/s achieved)", flush=True)
        if pn == 2048:
            print(f"projected full-source gradient at 2048^2, {FULL_SOURCE_2048} points: {per_point * FULL_SOURCE_2048 / 1e6:.2f} s "
                  f"(forward image at the same rate: {t_fwd * 1e3 / S * FULL_SOURCE_2048 / 1e6:.2f} s)", flush=True)


if __name__ == "__main__":
    main()
