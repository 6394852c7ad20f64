"""What the area-coverage rasteriser costs against the only other route to the same array.

    python scripts/coverage_time.py [--pn 2048] [--s 8] [--reps 10] [--out FILE]

(a) rasterizeLayout(antialias=s) at pn^2 (default workspace ceiling: bands), against
(b) the binary rasteriser at (pn s)^2 and pixel / s followed by a torch s x s block mean -- the route a caller had before --
for a sparse layout (about 300 random polygons) and a dense one (an array of about 1e5 rectangles), alternating a, b in
one process after a warm-up.  Two figures per leg: the whole call (host clock around a call that ends in a device
synchronise: edge list on the host, upload, kernels) and the device part alone (edges already on the device, device
events around the C entry, for (b) including the block mean).  The two results are compared bit for bit first.  Peak
device memory per leg from the caching allocator's high-water mark."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PS = 25.0


def sparse_layout(pn, n=300, seed=11):
    rng = np.random.default_rng(seed)
    span = pn * PS
    polys = []
    for i in range(n):
        cx, cy = rng.uniform(0.0, span, 2)
        if i % 3 == 0:
            w, h = rng.uniform(0.01 * span, 0.3 * span, 2)
            polys.append(np.array([[cx, cy], [cx + w, cy], [cx + w, cy + h], [cx, cy + h]]))
        elif i % 3 == 1:
            polys.append(np.array([cx, cy]) + rng.uniform(-0.2 * span, 0.2 * span, (3, 2)))
        else:
            k = int(rng.integers(5, 12))
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            rad = rng.uniform(0.02 * span, 0.2 * span, k)
            polys.append(np.array([cx, cy]) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1))
    return polys


def dense_layout(pn, per_side=316):
    """per_side^2 rectangles on a regular pitch, none on the pixel lattice (widths and offsets in odd nanometres)."""
    pitch = pn * PS / per_side
    i, j = np.meshgrid(np.arange(per_side), np.arange(per_side), indexing="ij")
    x, y = (i.reshape(-1) * pitch + 7.0), (j.reshape(-1) * pitch + 3.0)
    w, h = 0.43 * pitch + (i.reshape(-1) % 5), 0.61 * pitch + (j.reshape(-1) % 3)
    return list(np.stack([np.stack([x, y], 1), np.stack([x + w, y], 1), np.stack([x + w, y + h], 1), np.stack([x, y + h], 1)], axis=1))


def host_timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pn", type=int, default=2048)
    ap.add_argument("--s", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat
    from lithographysimulator_amd import layout as LY
    dev = torch.device("cuda", 0)
    pn, s = args.pn, args.s
    lib, st, P = nat.lib(), nat.stream_ptr(dev), nat.ptr
    lines = [f"coverage_time: {pn}^2, antialias {s} (sub-grid {pn * s}^2), {args.reps} alternating repetitions, {torch.cuda.get_device_name(dev)}"]
    for name, polys in (("sparse", sparse_layout(pn)), ("dense", dense_layout(pn))):
        new = lambda: L.rasterizeLayout(polys, pn, PS, origin=(0.0, 0.0), device=dev, antialias=s)                      # noqa: E731
        old = lambda: L.rasterizeLayout(polys, pn * s, PS / s, origin=(0.0, 0.0), device=dev).reshape(pn, s, pn, s).to(torch.float32).mean(dim=(1, 3))  # noqa: E731
        peak = {}
        for k, fn in (("a", new), ("b", old)):                             # warm-up, equality, peak memory
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            r = fn()
            torch.cuda.synchronize(dev)
            peak[k] = torch.cuda.max_memory_allocated(dev) - base
            if k == "a":
                ra = r
            else:
                assert torch.equal(ra, r), "the two routes differ"
            del r
        edges = LY.polygonEdges(polys)
        ed = torch.from_numpy(edges.reshape(-1)).to(dev)
        wb_new = min(nat.rasterize_coverage_work_bytes(pn, s, pn), LY.COVERAGE_WORK_BYTES)
        work_new = torch.empty(wb_new, dtype=torch.uint8, device=dev)
        cov = torch.empty((pn, pn), dtype=torch.float32, device=dev)
        work_old = torch.empty(nat.rasterize_work_bytes(pn * s), dtype=torch.uint8, device=dev)
        geo = torch.empty((pn * s, pn * s), dtype=torch.int16, device=dev)

        def dev_new():
            assert lib.litho_rasterize_coverage(P(ed), len(edges), pn, 0.0, 0.0, PS, s, P(work_new), wb_new, P(cov), st) == 0

        def dev_old():
            assert lib.litho_rasterize_edges(P(ed), len(edges), pn * s, 0.0, 0.0, PS / s, P(work_old), work_old.numel(), P(geo), st) == 0
            return geo.reshape(pn, s, pn, s).to(torch.float32).mean(dim=(1, 3))

        for _ in range(2):
            dev_new(), dev_old()
        torch.cuda.synchronize(dev)
        t = {k: [] for k in ("a call", "b call", "a device", "b device")}
        for _ in range(args.reps):
            t["a call"].append(host_timed(new, dev))
            t["b call"].append(host_timed(old, dev))
            t["a device"].append(event_timed(dev_new))
            t["b device"].append(event_timed(dev_old))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        lines.append(f"  {name}: {len(polys)} polygons, {len(edges)} edges, covered fraction {float(ra.mean()):.4f}; results identical")
        for k, v in t.items():
            lines.append(f"    {k:9s} median {med[k]:9.3f} ms  min {min(v):9.3f}  max {max(v):9.3f}")
        lines.append(f"    ratio b / a: whole call {med['b call'] / med['a call']:.2f}, device part {med['b device'] / med['a device']:.2f}")
        lines.append(f"    peak device memory of one call: a {peak['a'] / 2**20:.0f} MiB (workspace {wb_new / 2**20:.0f} MiB), "
                     f"b {peak['b'] / 2**20:.0f} MiB (workspace {work_old.numel() / 2**20:.0f} MiB + int16 raster {geo.numel() * 2 / 2**20:.0f} MiB + the block mean's temporaries)")
        del work_new, work_old, geo, cov, ed, ra
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
