"""What the contour tracer costs: device-event times of litho_contour_count and litho_contour_emit, each on its own.

    python scripts/contour_time.py [--n 2048] [--planes 5] [--doses 0.9,1.0,1.1] [--pitch 64] [--reps 30]

The image is synthetic and deterministic: lines of `pitch` pixels with a slow modulation along them and a contrast that
falls off with the plane's distance from the middle one, traced at T = 0.5 -- about 2 n^2 / pitch vertices per image.  The
calls repeat on one stack after a warm-up, so a stack that fits the last-level cache is read from there, not from HBM.
Bytes are the ones each pass must move: count reads the stack once and writes one 8-byte mask word and one 4-byte prefix per
64 edges plus the record totals; emit reads those back, the stack at most once more, and writes 12 bytes per vertex.  The
fraction is of the 4.1 TB/s that config 4 reaches (LABNOTES)."""
import argparse
import ctypes
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, HBM_REACHED = 0.5, 4.1e12


def timed(fn, reps):
    """Per-call milliseconds of `reps` calls of fn, one event pair each."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def line_stack(n, planes, pitch, dev):
    y, x = torch.meshgrid(torch.arange(n, device=dev, dtype=torch.float32), torch.arange(n, device=dev, dtype=torch.float32),
                          indexing="ij")
    mid = (planes - 1) / 2
    return torch.stack([0.5 + (0.4 - 0.03 * abs(p - mid)) * torch.cos(2 * math.pi * x / pitch)
                        + 0.05 * torch.cos(2 * math.pi * y / 300 + p) for p in range(planes)]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--planes", type=int, default=5)
    ap.add_argument("--doses", default="0.9,1.0,1.1")
    ap.add_argument("--pitch", type=float, default=64.0)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat

    dev = torch.device("cuda", 0)
    n, planes = args.n, args.planes
    doses = [float(d) for d in args.doses.split(",")]
    images = planes * len(doses)
    img = line_stack(n, planes, args.pitch, dev)
    lib = nat.lib()
    arr = (ctypes.c_float * len(doses))(*doses)
    nbytes = int(lib.litho_contour_work_bytes(n, planes, len(doses)))
    work = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    counts = torch.empty((images,), dtype=torch.int64, device=dev)
    call = (nat.ptr(img), planes, n, arr, len(doses), T, 1, nat.ptr(work), nbytes)
    xy, nxt, offsets = L.contourVertices(img, T, doses, True)                  # warm, and the sizes of the outputs
    V = int(offsets[-1])
    offs = offsets.ctypes.data_as(ctypes.c_void_p)
    with torch.cuda.device(dev):
        st = nat.stream_ptr(dev)

        def count():
            nat.check(lib.litho_contour_count(*call, nat.ptr(counts), st), "litho_contour_count")

        def emit():
            nat.check(lib.litho_contour_emit(*call, offs, nat.ptr(xy), nat.ptr(nxt), st), "litho_contour_emit")

        for fn in (count, emit):
            timed(fn, 3)
        t_count, t_emit = timed(count, args.reps), timed(emit, args.reps)
    again = L.contourVertices(img, T, doses, True)
    assert torch.equal(xy, again[0]) and torch.equal(nxt, again[1])            # the timed calls wrote what the wrapper writes

    W = (n + 1 + 63) // 64
    stack = planes * n * n * 4
    words = images * (n + 1) * 2 * W * 12
    totals = images * (n + 1) * 8
    moved = {"count": stack + words + totals, "emit": words + totals + stack + V * 12}
    print(f"n {n}, planes {planes}, doses {doses}: {images} images, {V} vertices ({V / images:.0f} per image), "
          f"workspace {nbytes / 1e6:.1f} MB; stack {stack / 1e6:.1f} MB, words {words / 1e6:.1f} MB, outputs {V * 12 / 1e6:.1f} MB")
    for name, ts in (("count", t_count), ("emit", t_emit)):
        med, b = float(np.median(ts)), moved[name]
        print(f"{name:5s}: median {med:.4f} ms (min {min(ts):.4f}), {med / images * 1e3:.1f} us per image; must move "
              f"{b / 1e6:.1f} MB: {b / med / 1e9:.3f} TB/s, {100 * b / (med * 1e-3) / HBM_REACHED:.1f} % of 4.1 TB/s")


if __name__ == "__main__":
    main()
