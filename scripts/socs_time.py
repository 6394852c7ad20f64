"""What Hopkins imaging costs and saves: set-up time of socsKernels and per-image time of hopkinsIntensity, beside the unchanged
abbeIntensity on the same operands (mask spectrum, pupil, source), at two of the benchmark's geometries.

    python scripts/socs_time.py [--configs cfg1,cfg3] [--reps 20] [--abbe-reps 3]

cfg1: 256^2 Bernoulli mask, circular source sigma 0.5, ideal pupil, K = 32 and 64; cfg3: 2048^2 Bernoulli mask, quasar(4, -pi/8)
0.4-0.8, the 10-term demo pupil, K = 64 and 256.  Set-up = one socsKernels call, host clock around a device synchronise (it waits
for the host-side eigenproblems anyway).  Per image = device events around `reps` back-to-back calls after two warm-up calls
(the first plans), both paths through their plan caches.  The image error printed is max |hopkins - abbe| / max abbe: the price
of truncating at K (`captured` = the kept share of trace T), not a rounding figure."""
import argparse
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEMO_AB = [0, 0, 0.01, 0, 100, 0.01, 0, 0.01, 0.01, 0.01]
WL, NA, PS = 193.0, 0.7, 25
CONFIGS = {"cfg1": (256, "circ", None, (32, 64)), "cfg3": (2048, "quasar", DEMO_AB, (64, 256))}


def per_call_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg1,cfg3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--abbe-reps", type=int, default=3)
    args = ap.parse_args()
    import lithographysimulator_amd as L
    from lithographysimulator_amd.synthetic import bernoulli_mask

    dev = torch.device("cuda", 0)
    print("| geometry | source points | K | captured | set-up s | hopkins ms / image | abbe ms / image | ratio | max diff / max |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in args.configs.split(","):
        pn, kind, ab, ks = CONFIGS[name]
        mask = L.Mask(bernoulli_mask(pn), PS, dev)
        mft = mask.fraunhofer(WL, True)
        eps, N = mask.calculateEpsilonN(mask.deltaK, PS, WL)
        src = L.LightSource(0.0, 0.5, pn, NA, device=dev) if kind == "circ" else L.LightSource(0.4, 0.8, pn, NA, device=dev)
        bitmap = src.generateAnnular() if kind == "circ" else src.generateQuasar(4, -math.pi / 8)
        pupil = L.Pupil(pn, WL, NA, torch.tensor(ab, dtype=torch.float16) if ab else None, dev).generatePupilFunction()
        shifts = L.sourceShifts(bitmap, pn)
        cache = L.PlanCache()
        want = L.abbeIntensity(mft, pupil, shifts, N, plan=cache)[0].clone()
        L.abbeIntensity(mft, pupil, shifts, N, plan=cache)
        torch.cuda.synchronize()
        abbe_ms = per_call_ms(lambda: L.abbeIntensity(mft, pupil, shifts, N, plan=cache), args.abbe_reps)
        for K in ks:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            socs = L.socsKernels(pupil, bitmap, kernels=K)
            torch.cuda.synchronize()
            setup = time.perf_counter() - t0
            got = L.hopkinsIntensity(mft, socs, N).clone()
            L.hopkinsIntensity(mft, socs, N)
            torch.cuda.synchronize()
            hop_ms = per_call_ms(lambda: L.hopkinsIntensity(mft, socs, N), args.reps)
            diff = float((got - want).abs().max() / want.max())
            print(f"| {name} {pn}^2 N {N} | {shifts.shape[0]} | {socs.K} | {socs.captured:.4f} | {setup:.2f} | {hop_ms:.3f} | "
                  f"{abbe_ms:.3f} | {abbe_ms / hop_ms:.1f} | {diff:.2e} |", flush=True)
            del socs, got
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
