"""What the film stack costs at set-up: litho_film_pupils at 2048^2 for L = 3 and 16 layers and D = 1 and 8 depths, beside
litho_vector_pupils writing the same number of planes (D defocus values), which is the homogeneous medium's cost for the same bytes.

    python scripts/film_time.py [--pn 2048] [--reps 200]

The C entry points are called directly into one preallocated output, so nothing but their own host work and launches is inside
the window: device events around `reps` back-to-back calls after three warm-up calls.  Both kernels read one pupil value per
cell and write 6 D complex64 values per cell; the achieved store bandwidth is 48 D pn^2 bytes over the time per call.  The film
kernel runs the two thin-film recursions once per cell (complex double arithmetic, L square roots and L exponentials) and then
two complex exponentials per depth; litho_vector_pupils runs one square root and one sincos per cell and plane.  For the
kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python scripts/film_time.py --reps 20`
(k_film_pupils, k_vector_pupils)."""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEMO_AB = [0, 0, 0.01, 0, 100, 0.01, 0, 0.01, 0.01, 0.01]
WL, NA = 193.0, 0.7
VNA, INDEX = 1.35, 1.44
SILICON = (0.88, 2.78)


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
    ap.add_argument("--pn", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat

    dev = torch.device("cuda", 0)
    pn = args.pn
    pupil = L.Pupil(pn, WL, NA, torch.tensor(DEMO_AB, dtype=torch.float16), dev).generatePupilFunction().to(torch.complex64).contiguous()
    stacks = {3: L.FilmStack([(1.55, 0.0, 35.0), (1.70, 0.02, 100.0), (1.82, 0.34, 40.0)], SILICON, 1),
              16: L.FilmStack([(1.45 + 0.05 * ((5 * i) % 7), 0.03 * ((3 * i) % 4), 12.0 + 7.0 * ((7 * i) % 5)) for i in range(16)],
                              SILICON, 8)}
    lib, st = nat.lib(), nat.stream_ptr(dev)
    print("| kernel | L | D | ms / call | GB/s stored |")
    print("|---|---|---|---|---|")
    for D in (1, 8):
        gbytes = 48.0 * D * pn * pn / 1e9
        out = torch.empty((D, 6, pn, pn), dtype=torch.complex64, device=dev)
        stackP = pupil[None].expand(D, pn, pn).contiguous()
        zs = (ctypes.c_double * D)(*[10.0 * d for d in range(D)])

        def homogeneous():
            nat.check(lib.litho_vector_pupils(nat.ptr(stackP), D, pn, VNA, INDEX, 1, zs, WL, nat.ptr(out), st), "litho_vector_pupils")

        calls = [("litho_vector_pupils", "-", homogeneous)]
        for count, stack in stacks.items():
            layers = (ctypes.c_double * (3 * count))(*[v for layer in stack.layers for v in layer])
            depths = (ctypes.c_double * D)(*stack.depths(D))

            def film(stack=stack, layers=layers, depths=depths, count=count):
                nat.check(lib.litho_film_pupils(nat.ptr(pupil), 1, pn, VNA, INDEX, 1, layers, count, stack.substrate[0], stack.substrate[1],
                                                stack.resist, depths, D, None, WL, nat.ptr(out), st), "litho_film_pupils")

            calls.append(("litho_film_pupils", count, film))
        for name, count, fn in calls:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ms = per_call_ms(fn, args.reps)
            print(f"| {name} | {count} | {D} | {ms:.4f} | {gbytes / (ms * 1e-3):.0f} |", flush=True)


if __name__ == "__main__":
    main()
