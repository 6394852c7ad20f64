"""What the gradient through the post-exposure bake costs at 2048^2: milliseconds per litho_peb_bake_vjp of S = 32 steps at D = 8 and
16 planes with the state kept every c = 1, ceil(sqrt S) and S steps, against the forward bake timed in the same process, with the
bytes a call moves and its workspace.

    python scripts/peb_grad_time.py [--n 2048] [--steps 32] [--reps 5] [--rounds 3]

Both entry points are called directly into preallocated buffers on a random acid volume with both species diffusing, a finite
kQuench and all three cotangents given (the setting of scripts/peb_time.py).  Per D: two warm-up calls of every variant, then
`reps` back-to-back calls between device events, the variants in turn, `rounds` times over, in one process on one device; the
table gives the median and the range of the rounds.  Bytes, counted from the launches as the host code makes them (the neighbours
come from the caches), per cell: a forward-sweep step reads h, q and writes h, q (16; the first reads no q); a taped step writes
hd, qd on top (24; the last of a segment writes no state: 16); a backward step reads hbar, qbar, abar, hd, qd and writes hbar,
qbar (28).  The forward bake moves 24 per step.  No target is set: the figure of merit is the ratio to the forward bake of the
same run.  First measurement of untuned kernels."""
import argparse
import math
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


def vjp_bytes_per_cell(S, c):
    """Bytes per cell of one litho_peb_bake_vjp with all cotangents given, launch by launch."""
    nc = (S + c - 1) // c
    total = 16 * (nc - 1) * c - (4 if nc > 1 else 0)                          # the forward sweep; its first step reads no q
    for j in range(nc):
        k0, k1 = j * c, min(S, j * c + c)
        total += 24 * (k1 - k0) - 8 - (4 if j == 0 else 0)                    # taped steps; the last writes no state
        total += 28 * (k1 - k0)                                               # backward steps
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from lithographysimulator_amd import _native as nat

    dev = torch.device("cuda", 0)
    n, S, thickness, pixel = args.n, args.steps, 120.0, 25.0
    lib, st = nat.lib(), nat.stream_ptr(dev)
    physical = (thickness, pixel, 0.1, 5.0, 0.01, 20.0, 5.0, 0.5, 60.0)
    print("| D | call | workspace GiB | ms per call (median, range) | x forward bake | GB per call | share of 4.1 TB/s |")
    print("|---|---|---|---|---|---|---|")
    for D in (8, 16):
        torch.manual_seed(D)
        cells = D * n * n
        h0 = torch.rand((1, D, n, n), dtype=torch.float32, device=dev)
        gh, gq = torch.rand_like(h0) - 0.5, torch.rand_like(h0) - 0.5
        ga = (torch.rand_like(h0) - 0.5) / 60.0
        h, q, a = torch.empty_like(h0), torch.empty_like(h0), torch.empty_like(h0)
        out_h, out_q = torch.empty_like(h0), torch.empty_like(h0)
        assert 1 <= lib.litho_peb_min_steps(20.0, 5.0, 0.5, thickness, D, pixel) <= S
        fwd_bytes = int(lib.litho_peb_work_bytes(1, D, n))
        cs = sorted({1, math.isqrt(S - 1) + 1, S})
        vjp_work = {c: int(lib.litho_peb_vjp_work_bytes(1, D, n, S, c)) for c in cs}
        work = torch.empty(max([fwd_bytes] + list(vjp_work.values())), dtype=torch.uint8, device=dev)

        def forward():
            return lib.litho_peb_bake(nat.ptr(h0), 1, D, n, *physical, S, 1, nat.ptr(h), nat.ptr(q), nat.ptr(a), nat.ptr(work), fwd_bytes, st)

        def backward(c):
            return lib.litho_peb_bake_vjp(nat.ptr(h0), 1, D, n, *physical, S, c, nat.ptr(gh), nat.ptr(gq), nat.ptr(ga), nat.ptr(out_h),
                                          nat.ptr(out_q), nat.ptr(work), vjp_work[c], st)

        variants = {"forward bake": forward}
        variants.update({f"vjp c = {c}": (lambda c=c: backward(c)) for c in cs})
        for fn in variants.values():
            assert fn() == nat.LITHO_OK and fn() == nat.LITHO_OK
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                times[name].append(event_ms(fn, args.reps))
        base = statistics.median(times["forward bake"])
        for name in variants:
            ms = statistics.median(times[name])
            c = int(name.split("=")[1]) if "=" in name else None
            gb = (24 * S if c is None else vjp_bytes_per_cell(S, c)) * cells / 1e9
            ws = (fwd_bytes if c is None else vjp_work[c]) / 2 ** 30
            print(f"| {D} | {name} | {ws:.2f} | {ms:.3f} ({min(times[name]):.3f} ... {max(times[name]):.3f}) | {ms / base:.2f} | {gb:.2f} | "
                  f"{100.0 * gb / (ms * 1e-3) / (HBM_TBS * 1e3):.1f} % |", flush=True)


if __name__ == "__main__":
    main()
