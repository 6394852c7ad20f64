"""What the resist model costs: device-event times of the fused diffused-image pass and of the edge finder.

    python scripts/resist_time.py [--planes 32] [--pn 2048] [--reps 20] [--out FILE]

(a) litho_postprocess_resist (image + contour; the kernel is the parent commit's, untouched) against
(b) litho_postprocess_resist_diffused at sigma = 30 nm (R = 5) writing D + contour -- same bytes in and out --, alternating
    a, b, a, b in one process after a warm-up, plus (c) the same at sigma = 200 nm (R = 32) and (d) contour only at R = 5;
(e) measureCD for planes x 64 gauges x 3 doses against (f) the pixel bossungCurves loop over the same 64 gauges.
Bytes/s are against the algorithm's own traffic, 4 pn^2 read + 5 n^2 written per plane."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PS, WL = 25, 193.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=32)
    ap.add_argument("--pn", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat
    dev = torch.device("cuda", 0)
    planes, pn = args.planes, args.pn
    eps, _ = nat.epsilon_n(4 / pn, PS, WL)
    gen = torch.Generator().manual_seed(1)
    raw = torch.rand(planes, pn, pn, generator=gen).to(dev)
    image, resist = L.resistContour(raw, eps, 0.5, return_image=True)
    n = image.shape[-1]
    lib, st = nat.lib(), nat.stream_ptr(dev)
    P = nat.ptr

    def plain():
        lib.litho_postprocess_resist(P(raw), planes, pn, eps, 1.0, 0.5, P(image), P(resist), st)

    def diffused(sigma_nm, with_image=True):
        def call():
            rc = lib.litho_postprocess_resist_diffused(P(raw), planes, pn, eps, 1.0, 0.5, sigma_nm / PS,
                                                       P(image) if with_image else None, P(resist), st)
            assert rc == 0
        return call

    legs = {"a plain image+contour": plain, "b diffused R=5 D+contour": diffused(30.0), "c diffused R=32 D+contour": diffused(200.0),
            "d diffused R=5 contour only": diffused(30.0, False)}
    for fn in legs.values():                                              # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.reps):                                            # alternate the legs
        for k, fn in legs.items():
            times[k] += timed(fn, 1)
    lines = [f"resist_time: {planes} x {pn}^2 raw -> {n}^2, {args.reps} alternating repetitions, device events, {torch.cuda.get_device_name(dev)}"]
    own = planes * (4 * pn * pn + 5 * n * n)
    for k, t in times.items():
        t = sorted(t)
        med = t[len(t) // 2]
        b = own - (planes * 4 * n * n if k.startswith("d") else 0)
        lines.append(f"  {k:30s} median {med:8.3f} ms  min {t[0]:8.3f}  max {t[-1]:8.3f}   {b / med / 1e9:7.3f} TB/s of own bytes ({b / 1e6:.0f} MB)")
    ma = sorted(times["a plain image+contour"])[args.reps // 2]
    for k in list(times)[1:]:
        lines.append(f"  ratio {k.split()[0]} / a = {sorted(times[k])[args.reps // 2] / ma:.3f}")

    # the edge finder: 64 gauges across the grid, rows and columns, three doses
    D = L.resistContour(raw, eps, 0.5, return_image=True, diffusionLength=30.0, pixelSize=PS)[0]
    gauges = [(n // 2 + 13 * (i - 32), (37 * i + 11) % n, i % 2) for i in range(64)]
    g_dev = torch.tensor(gauges, dtype=torch.int32, device=dev)
    doses = [0.8, 1.0, 1.25]
    cd = lambda: L.measureCD(D, 0.5, g_dev, PS, doses=doses)              # noqa: E731
    cd()
    t = sorted(timed(cd, args.reps))
    lines.append(f"  e measureCD {planes} planes x 64 gauges x 3 doses: median {t[len(t) // 2]:.3f} ms  min {t[0]:.3f}  max {t[-1]:.3f}")

    def pixel_loop():
        for r, c, _ in gauges:
            L.bossungCurves(raw, eps, 0.5, doses, PS, row=r, column=c)
    pixel_loop()
    t = sorted(timed(pixel_loop, 3))
    lines.append(f"  f pixel bossungCurves, 64 row gauges x 3 doses (192 threshold passes): median {t[1]:.1f} ms  min {t[0]:.1f}  max {t[-1]:.1f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
