"""What the resist-parameter gradients cost at 2048^2: milliseconds per litho_peb_bake_vjp_params of S = 32 steps at D = 8 and 16
planes against litho_peb_bake_vjp of the same run (both with the state kept every ceil(sqrt S) steps), and per
litho_develop_rate_vjp_params against litho_develop_rate_vjp, with the bytes a call moves.

    python scripts/resist_param_grad_time.py [--n 2048] [--steps 32] [--reps 5] [--rounds 3]

The entry points are called directly into preallocated buffers on a random acid volume with both species diffusing, a finite
kQuench and all three cotangents given (the setting of scripts/peb_grad_time.py, whose byte count of litho_peb_bake_vjp is used).
Per D: two warm-up calls of every variant, then `reps` back-to-back calls between device events, the variants in turn, `rounds`
times over, in one process on one device; the table gives the median and the range of the rounds.  Bytes per cell on top of
litho_peb_bake_vjp: a backward step also reads the state h_k and q_k at the cell (8; the first step has no q), the neighbours
coming from the caches; the six doubles per workgroup are 48 bytes per 256 cells and step.  The rate law: the vjp reads x and the
cotangent and writes grad_x (12 per cell and gain, x once), the parameter sums read the same two and write nothing per cell.
No target is set: the figure of merit is the ratio to the existing call of the same run.  First measurement of untuned kernels."""
import argparse
import ctypes
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
HBM_TBS = 4.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from lithographysimulator_amd import _native as nat
    from peb_grad_time import event_ms, vjp_bytes_per_cell

    dev = torch.device("cuda", 0)
    n, S, thickness, pixel = args.n, args.steps, 120.0, 25.0
    lib, st = nat.lib(), nat.stream_ptr(dev)
    physical = (thickness, pixel, 0.1, 5.0, 0.01, 20.0, 5.0, 0.5, 60.0)
    mack = (0.05, 120.0, 0.05, 5.0, 0.4, 1.0, 1.0, thickness)                  # kAmp, rMax, rMin, q, mTh, surface factor off
    one = (ctypes.c_float * 1)(1.0)
    print("| D | call | workspace GiB | ms per call (median, range) | x the existing call | GB per call | share of 4.1 TB/s |")
    print("|---|---|---|---|---|---|---|")
    for D in (8, 16):
        torch.manual_seed(D)
        cells = D * n * n
        h0 = torch.rand((1, D, n, n), dtype=torch.float32, device=dev)
        gh, gq = torch.rand_like(h0) - 0.5, torch.rand_like(h0) - 0.5
        ga = (torch.rand_like(h0) - 0.5) / 60.0
        dose = torch.rand_like(h0) * 60.0
        out_h, out_q = torch.empty_like(h0), torch.empty_like(h0)
        out_s = torch.empty((1, 6), dtype=torch.float64, device=dev)
        sums = torch.empty((D, 6), dtype=torch.float64, device=dev)
        assert 1 <= lib.litho_peb_min_steps(20.0, 5.0, 0.5, thickness, D, pixel) <= S
        c = math.isqrt(S - 1) + 1
        sizes = {"vjp": int(lib.litho_peb_vjp_work_bytes(1, D, n, S, c)), "vjp params": int(lib.litho_peb_vjp_params_work_bytes(1, D, n, S, c)),
                 "rate vjp": 0, "rate params": int(lib.litho_develop_rate_params_work_bytes(1, D, n, 1))}
        work = torch.empty(max(sizes.values()), dtype=torch.uint8, device=dev)

        def vjp():
            return lib.litho_peb_bake_vjp(nat.ptr(h0), 1, D, n, *physical, S, c, nat.ptr(gh), nat.ptr(gq), nat.ptr(ga), nat.ptr(out_h),
                                          nat.ptr(out_q), nat.ptr(work), sizes["vjp"], st)

        def vjp_params():
            return lib.litho_peb_bake_vjp_params(nat.ptr(h0), 1, D, n, *physical, S, c, nat.ptr(gh), nat.ptr(gq), nat.ptr(ga), nat.ptr(out_h),
                                                 nat.ptr(out_q), nat.ptr(out_s), nat.ptr(work), sizes["vjp params"], st)

        def rate_vjp():
            return lib.litho_develop_rate_vjp(nat.ptr(dose), 1, D, n, one, 1, *mack, nat.ptr(gh), nat.ptr(out_h), st)

        def rate_params():
            return lib.litho_develop_rate_vjp_params(nat.ptr(dose), 1, D, n, one, 1, *mack, nat.ptr(gh), nat.ptr(sums), nat.ptr(work),
                                                     sizes["rate params"], st)

        variants = {"vjp": vjp, "vjp params": vjp_params, "rate vjp": rate_vjp, "rate params": rate_params}
        for fn in variants.values():
            assert fn() == nat.LITHO_OK and fn() == nat.LITHO_OK
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                times[name].append(event_ms(fn, args.reps))
        per_cell = {"vjp": vjp_bytes_per_cell(S, c), "vjp params": vjp_bytes_per_cell(S, c) + 8 * S - 4 + 48.0 * S / 256, "rate vjp": 12,
                    "rate params": 8 + 48.0 / 256}
        base = {"vjp": "vjp", "vjp params": "vjp", "rate vjp": "rate vjp", "rate params": "rate vjp"}
        for name in variants:
            ms = statistics.median(times[name])
            gb = per_cell[name] * cells / 1e9
            print(f"| {D} | {name}{f' c = {c}' if name.startswith('vjp') else ''} | {sizes[name] / 2 ** 30:.2f} | {ms:.3f} "
                  f"({min(times[name]):.3f} ... {max(times[name]):.3f}) | {ms / statistics.median(times[base[name]]):.2f} | {gb:.2f} | "
                  f"{100.0 * gb / (ms * 1e-3) / (HBM_TBS * 1e3):.1f} % |", flush=True)


if __name__ == "__main__":
    main()
