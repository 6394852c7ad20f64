"""What the post-exposure bake costs at 2048^2: milliseconds per bake of S = 32 steps at D = 8 and 16 planes, the direct kernel
(one step per launch) against the fused kernel at s = 2, 3, 4 steps per launch, and the bytes a step moves.

    python scripts/peb_time.py [--n 2048] [--steps 32] [--reps 10] [--rounds 3]

litho_peb_bake is called directly into preallocated buffers on a random acid volume with both species diffusing and a finite
kQuench.  Per (D, s): two warm-up calls, then `reps` back-to-back calls between device events; the variants of one D are timed
in turn, `rounds` times over, in one process on one device, and the table gives the median and the range of the rounds.  Bytes per
step: the direct kernel reads h, q, a and writes h, q, a once each (the neighbours come from the caches): 24 D n^2; the fused
kernel reads h and q of a (16 + 2 s)^2 window per 16^2 tile, reads a and writes h, q, a once per s steps:
(8 (16 + 2 s)^2 / 256 + 16) D n^2 / s.  A variant whose LDS does not fit a workgroup is left out.  First measurements of untuned
kernels; no target is set."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 4.1


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from lithographysimulator_amd import _native as nat

    dev = torch.device("cuda", 0)
    n, S, thickness, pixel = args.n, args.steps, 120.0, 25.0
    lib, st = nat.lib(), nat.stream_ptr(dev)
    print("| D | steps per launch | LDS KiB | ms per bake (median, range) | ms per step | GB per step | share of 4.1 TB/s |")
    print("|---|---|---|---|---|---|---|")
    for D in (8, 16):
        torch.manual_seed(D)
        h0 = torch.rand((1, D, n, n), dtype=torch.float32, device=dev)
        h, q, a = torch.empty_like(h0), torch.empty_like(h0), torch.empty_like(h0)
        nbytes = int(lib.litho_peb_work_bytes(1, D, n))
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        least = lib.litho_peb_min_steps(20.0, 5.0, 0.5, thickness, D, pixel)
        assert 1 <= least <= S, least

        def bake(s):
            return lib.litho_peb_bake(nat.ptr(h0), 1, D, n, thickness, pixel, 0.1, 5.0, 0.01, 20.0, 5.0, 0.5, 60.0, S, s, nat.ptr(h), nat.ptr(q),
                                      nat.ptr(a), nat.ptr(work), nbytes, st)

        variants = [s for s in (1, 2, 3, 4) if bake(s) == nat.LITHO_OK]
        torch.cuda.synchronize()
        times = {s: [] for s in variants}
        for s in variants:
            bake(s), bake(s)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for s in variants:
                times[s].append(event_ms(lambda: bake(s), args.reps))
        auto = lib.litho_peb_steps_per_launch(D)
        for s in variants:
            ms = statistics.median(times[s])
            lds = 0 if s == 1 else D * (4 * (16 + 2 * s) ** 2 + 256) * 4 / 1024
            gb = (24.0 if s == 1 else (8.0 * (16 + 2 * s) ** 2 / 256 + 16.0) / s) * D * n * n / 1e9
            per = ms / S
            print(f"| {D} | {s}{' (automatic)' if s == auto else ''} | {lds:.1f} | {ms:.3f} ({min(times[s]):.3f} ... {max(times[s]):.3f}) | {per:.4f} | "
                  f"{gb:.3f} | {100.0 * gb / (per * 1e-3) / (HBM_TBS * 1e3):.1f} % |", flush=True)


if __name__ == "__main__":
    main()
