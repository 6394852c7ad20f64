"""What the gradient through development costs at 2048^2: milliseconds for the adjoint solve (litho_develop_time_vjp: the link pass,
the gather iteration, the closing product), its launch count and milliseconds per launch, and the rate backwards
(litho_develop_rate_vjp), beside the forward developmentTime of the same run, at D = 8 and 16 planes.

    python scripts/develop_grad_time.py [--n 2048] [--reps 10]

The volume is that of scripts/develop_time.py (the image of examples/resist_profile.py tiled to n^2); the cotangent is 1 on every
cell that develops within 15 s.  The C entry points are called directly into preallocated buffers.  Both solvers wait for the
device by themselves (they read their change flags back every fourth launch), so their times are wall time per call, after two
warm-up calls, and include those waits; the group of launches that finds the fixed point is always run to its end.  The link
pass and the closing product are timed on their own by a call whose launch cap is 1 (it ends with LITHO_E_NOCONV after the link
pass and one gather launch) -- an upper bound for the link pass.  A gather launch reads the links (16 B per cell), the cotangent
and lambda and writes lambda: 28 D n^2 bytes.  First measurements of untuned kernels; no target is set."""
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


def wall_ms(fn, reps):
    fn(), fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import lithographysimulator_amd as L                                  # noqa: F401
    from lithographysimulator_amd import _native as nat
    from resist_profile import film, grating_image

    dev = torch.device("cuda", 0)
    n, thickness, pixel, t_dev = args.n, 120.0, 25.0, 15.0
    lib, st = nat.lib(), nat.stream_ptr(dev)
    stack = film(thickness, False)
    gains = (ctypes.c_float * 1)(1.0)
    print("| D | forward ms | launches | adjoint ms | launches | ms / launch | GB / launch | share of 4.1 TB/s | links + 1 launch ms | rate vjp ms |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for D in (8, 16):
        small = grating_image(dev, stack, D)
        m = small.shape[-1]
        reps_xy = -(-n // m)
        image = small.repeat(1, reps_xy, reps_xy)[:, :n, :n].contiguous()
        s, T, gs, gx = (torch.empty_like(image) for _ in range(4))
        fbytes = int(lib.litho_develop_work_bytes(1, D, n, 1024))
        fwork = torch.empty(fbytes, dtype=torch.uint8, device=dev)
        bbytes = int(lib.litho_develop_vjp_work_bytes(1, D, n, 1024))
        bwork = torch.empty(bbytes, dtype=torch.uint8, device=dev)
        fl, bl = ctypes.c_int(0), ctypes.c_int(0)
        rate_args = (1, D, n, gains, 1, 4.0, 100.0, 0.05, 15.0, 0.2, 1.0, thickness, thickness)
        nat.check(lib.litho_develop_rate(nat.ptr(image), *rate_args, nat.ptr(s), st), "litho_develop_rate")

        def forward():
            nat.check(lib.litho_develop_time(nat.ptr(s), 1, D, n, thickness, pixel, 1024, nat.ptr(T), nat.ptr(fwork), fbytes,
                                             ctypes.byref(fl), st), "litho_develop_time")

        ms = {"forward": wall_ms(forward, args.reps)}
        g = (T <= t_dev).to(torch.float32).contiguous()

        def adjoint(cap=1024):
            rc = lib.litho_develop_time_vjp(nat.ptr(s), nat.ptr(T), nat.ptr(g), 1, D, n, thickness, pixel, cap, nat.ptr(gs), nat.ptr(bwork),
                                            bbytes, ctypes.byref(bl), st)
            if not (cap == 1 and rc == nat.E_NOCONV):
                nat.check(rc, "litho_develop_time_vjp")

        ms["links"] = wall_ms(lambda: adjoint(1), args.reps)
        ms["adjoint"] = wall_ms(adjoint, args.reps)

        def rate_vjp():
            nat.check(lib.litho_develop_rate_vjp(nat.ptr(image), *rate_args, nat.ptr(gs), nat.ptr(gx), st), "litho_develop_rate_vjp")

        rate_vjp(), rate_vjp()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            rate_vjp()
        b.record()
        b.synchronize()
        ms["rate"] = a.elapsed_time(b) / args.reps
        ran = -(-bl.value // 4) * 4
        gb = 28.0 * D * n * n / 1e9
        per = ms["adjoint"] / ran
        print(f"| {D} | {ms['forward']:.3f} | {fl.value} | {ms['adjoint']:.3f} | {bl.value} (ran {ran}) | {per:.3f} | {gb:.3f} | "
              f"{100.0 * gb / (per * 1e-3) / (HBM_TBS * 1e3):.1f} % | {ms['links']:.3f} | {ms['rate']:.3f} |", flush=True)


if __name__ == "__main__":
    main()
