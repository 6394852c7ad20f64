"""What resist development costs at 2048^2: milliseconds per stage (latent-image diffusion, rate, arrival time, developed depth)
at D = 8 and 16 planes, the solver's launch count, and the bytes a solver launch moves as a share of the 4.1 TB/s measured on the
MI355X.

    python scripts/develop_time.py [--n 2048] [--reps 20]

The volume is the image of examples/resist_profile.py (the 125 nm grating in 120 nm of resist without a BARC) tiled to n^2.  The
C entry points are called directly into preallocated buffers: device events around `reps` back-to-back calls after two warm-up
calls.  litho_develop_time waits for the device by itself (it reads its change flags back every fourth launch), so its time is
wall time per call and includes those waits.  A solver launch reads T and s and writes T: (2 . 4 + 4) D n^2 bytes.  First
measurements of untuned kernels; no target is set."""
import argparse
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
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
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat
    from resist_profile import film, grating_image

    dev = torch.device("cuda", 0)
    n, thickness, pixel, t_dev = args.n, 120.0, 25.0, 15.0
    lib, st = nat.lib(), nat.stream_ptr(dev)
    stack = film(thickness, False)
    gains = (ctypes.c_float * 1)(1.0)
    print("| D | diffuse ms | rate ms | time ms | launches | ms / launch | GB / launch | share of 4.1 TB/s | depth ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for D in (8, 16):
        small = grating_image(dev, stack, D)
        m = small.shape[-1]
        reps_xy = -(-n // m)
        image = small.repeat(1, reps_xy, reps_xy)[:, :n, :n].contiguous()
        lat, s, T = torch.empty_like(image), torch.empty_like(image), torch.empty_like(image)
        work = torch.empty_like(image)
        depth = torch.empty((n, n), dtype=torch.float32, device=dev)
        hz = thickness / D
        nbytes = int(lib.litho_develop_work_bytes(1, D, n, 1024))
        swork = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        launches = ctypes.c_int(0)

        def diffuse():
            nat.check(lib.litho_latent_diffuse(nat.ptr(image), 1, D, n, 5.0 / pixel, 20.0 / hz, nat.ptr(lat), nat.ptr(work),
                                               work.numel() * 4, st), "litho_latent_diffuse")

        def rate():
            nat.check(lib.litho_develop_rate(nat.ptr(lat), 1, D, n, gains, 1, 4.0, 100.0, 0.05, 15.0, 0.2, 1.0, thickness, thickness,
                                             nat.ptr(s), st), "litho_develop_rate")

        def solve():
            nat.check(lib.litho_develop_time(nat.ptr(s), 1, D, n, thickness, pixel, 1024, nat.ptr(T), nat.ptr(swork), nbytes,
                                             ctypes.byref(launches), st), "litho_develop_time")

        def developed():
            nat.check(lib.litho_developed_depth(nat.ptr(T), 1, D, n, thickness, t_dev, nat.ptr(depth), st), "litho_developed_depth")

        ms = {}
        for name, fn in (("diffuse", diffuse), ("rate", rate)):
            fn(), fn()
            torch.cuda.synchronize()
            ms[name] = event_ms(fn, args.reps)
        solve(), solve()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            solve()
        torch.cuda.synchronize()
        ms["time"] = (time.perf_counter() - t0) * 1e3 / args.reps
        developed(), developed()
        torch.cuda.synchronize()
        ms["depth"] = event_ms(developed, args.reps)
        # the group of launches that finds the fixed point is always run to its end: launches rounded up to a multiple of four
        ran = -(-launches.value // 4) * 4
        gb = 12.0 * D * n * n / 1e9
        per = ms["time"] / ran
        print(f"| {D} | {ms['diffuse']:.3f} | {ms['rate']:.3f} | {ms['time']:.3f} | {launches.value} (ran {ran}) | {per:.3f} | {gb:.3f} | "
              f"{100.0 * gb / (per * 1e-3) / (HBM_TBS * 1e3):.1f} % | {ms['depth']:.3f} |", flush=True)


if __name__ == "__main__":
    main()
