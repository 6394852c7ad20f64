#!/usr/bin/env python3
"""Headline benchmark: Abbe source-points x image-pixels per second on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg1..cfg5] [--shard i/n] [--points K]
                    [--dump-outputs DIR] [--full [--no-cpu-baseline] [--no-extra]]

One "step" = one complete abbeImage call (source-list compaction, Abbe accumulation over every source point --
and every through-focus plane -- of the configuration, all-reduce when N > 1, post-process) on synthetic inputs
that are resident in HBM when the timed region starts.  Default workload = BASELINE config 3, the one the
roofline target is quoted on: 2048x2048 bernoulli mask, quasar source sigma 0.4-0.8 (S = 198,108), 10-term
Zernike-aberrated pupil.  With N > 1 (one rank per GPU, RCCL) the source list is split into N contiguous shards
and the partial intensities are summed by ONE all-reduce: total work is fixed -> "strong".

Launching: under torch.distributed.run the ranks read RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the
environment.  Started as a plain process with --gpus N > 1, this file starts the N ranks ITSELF as fresh child
processes (before anything in the parent touches the GPU), waits for them and relays rank 0's JSON line.

A plain run sets up, warms up, times the K steps, writes the last step's image under --dump-outputs DIR (DIR/image.npy,
float32; an image above 64 MB as a fixed, seeded sample: DIR/image_sample.npy and its flat indices DIR/image_sample_index.npy)
and prints the headline line.  Everything else below is measured with --full only.

Rank 0 prints one JSON line (contract in the task statement); with --full it also carries
  roofline        the dominant kernel (name reported by the library, litho_abbe_last_kernels) against the bound the
                  counters and microbenchmarks show: fp32 VALU issue.  achieved = nominal FFT flops (5 N log2 N per
                  transformed line) of one launch / its HIP-event-timed duration, peak = 157.3 TFLOP/s fp32 vector.
                  Beside it, as top-level keys: `traffic` = PMC-measured L2 memory-side bytes per launch of THIS
                  workload (profiles/traffic.json: rocprofv3 --pmc passes over this very command; Infinity-Cache hits
                  INCLUDED, so this is fabric traffic, not HBM traffic), `fabric_frac` = traffic / time / 8 TB/s,
                  `effective_40B_over_peak` = the SURVEY 8d 40-byte model over kernel time / 8 TB/s (labelled
                  effective: most of those bytes are never moved), `copy_ceiling_GBs` = this box's own 1 GiB copy rate;
  cpu_baseline    (N = 1) the oracle's torch-CPU op chain, i.e. a port of the reference loop, on a bounded sample, with
                  the GPU-vs-CPU parity of that sample taken on the SAME evaluation path the timed step ran;
  extra_workloads (default workload only) two or more timed steps each of config 1, config 2, one rank's shard of config 4
                  and the config 5 stack (mean by host clock + per-step HIP-event times and their median), so that every
                  BASELINE configuration has a driver-observed number with more than one sample;
  ranks           (N > 1) per-rank step time, compute time and all-reduce time of one instrumented step;
  prediction      the N-GPU step stated in advance, against the measured one;
  step_ms         for short steps (config 1), whose events are taken in a pass of K more steps of their own.
"""
import argparse
import contextlib
import json
import math
import os
import socket
import statistics
import subprocess
import sys
import time
from datetime import timedelta

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WL, NA, PS = 193.0, 0.7, 25
DEMO_AB = [0, 0, 0.01, 0, 100, 0.01, 0, 0.01, 0.01, 0.01]
DEFOCUS_NM = [-310 + 20 * k for k in range(32)]           # config 5
WORKLOADS = {
    # name: (pn, source kind, aberrations, planes, description)
    "cfg1": (256, "circ", None, 1, "256x256 bernoulli mask, circular source sigma 0.5, ideal pupil (the reference's CPU-runnable case)"),
    "cfg2": (1024, "annular", [0, 0, 0, 0, 100], 1, "1024x1024 bernoulli mask, annular 0.4-0.8, defocus-only pupil"),
    "cfg3": (2048, "quasar", DEMO_AB, 1, "2048x2048 bernoulli mask, quasar(4,-pi/8) 0.4-0.8, 10-term Zernike pupil"),
    "cfg4": (4096, "annular", [0, 0, 0, 0, 100], 1, "4096x4096 bernoulli mask, annular 0.4-0.8, defocus-only pupil"),
    "cfg5": (2048, "quasar", DEMO_AB, 32, "2048x2048 bernoulli mask x 32-plane through-focus stack (defocus -310..310 nm), quasar(4,-pi/8) 0.4-0.8"),
    # NOT a BASELINE configuration: config 3's optics on a mask whose size is not a power of two -- evaluated embedded in the
    # 2048^2 grid; rides in extra_workloads so that the path has a driver-observed number
    "odd2000": (2000, "quasar", DEMO_AB, 1, "NOT A BASELINE CONFIG: 2000x2000 bernoulli mask (not a power of two: embedded evaluation), quasar(4,-pi/8) 0.4-0.8, 10-term Zernike pupil"),
}
HBM_PEAK_GBS = 8000.0                 # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
VALU_PEAK_TFLOPS = 157.3              # MI355X_MICROARCH.md: peak fp32 vector
# Algorithmic bytes per source-point*pixel: 40 for the fused pipeline =
# x-pass 24 (read mask window 8 + pupil window 8, write intermediate 8) + y-pass 16 (read
# intermediate 8, read-modify-write intensity 8).
ALGO_BYTES = {"xpass": 24.0, "ypass": 16.0}
# BASELINE.md's absolute target: >= 60 % of the HBM roofline under the 40-byte model at 2048^2 = 0.6 * 8e12 / 40 per GPU
TARGET_ABS_PER_GPU = 1.2e11
# launch geometry that PMC bytes per item depend on besides the kernel names (profiles/traffic.json entries carry it)
GEOMETRY_KEYS = ("batch", "groups_per_plane", "xchunk", "planes_in_flight", "coarse_grid", "variant")


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="number of ranks (default: WORLD_SIZE when launched under torch.distributed.run, else 1)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="cfg3", choices=list(WORKLOADS))
    ap.add_argument("--shard", default=None, metavar="i/n",
                    help="single GPU only: process shard i of n of the source list (the per-rank work of the n-GPU run, "
                         "without the all-reduce)")
    ap.add_argument("--points", type=int, default=0,
                    help="profiling aid: only the first K consecutive source points (the JSON line is then marked partial)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the image of the last one as DIR/<name>.npy (float32, at most 64 MB)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: roofline, CPU baseline, extra workloads, per-rank view, prediction")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline leg")
    ap.add_argument("--no-extra", action="store_true",
                    help="--full without the extra_workloads leg (configs 1, 2, 4-shard, 5) of the default single-GPU run")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


DUMP_LIMIT_BYTES = 64_000_000
DUMP_SAMPLE = 1 << 22                 # elements of a sampled output: 16 MB of values + 32 MB of float64 indices
DUMP_SEED = 20240601


def dump_outputs(dirname, outputs):
    """What the timed path returned, as DIR/<name>.npy in float32.  An output above DUMP_LIMIT_BYTES is written as a fixed, seeded
    sample of its elements (<name>_sample.npy) with their flat row-major indices (<name>_sample_index.npy, float64): the same
    shape gives the same indices in every run, so two builds compare element for element.  Returns what was written."""
    import numpy as np
    import torch
    os.makedirs(dirname, exist_ok=True)
    written = {}
    for name, t in outputs.items():
        t = t.detach().float()
        if t.numel() * 4 <= DUMP_LIMIT_BYTES:
            np.save(os.path.join(dirname, f"{name}.npy"), t.cpu().numpy())
            written[name] = {"file": f"{name}.npy", "shape": list(t.shape), "sampled": False}
            continue
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(t.numel(), DUMP_SAMPLE, replace=False))
        vals = t.reshape(-1)[torch.from_numpy(idx).to(t.device)].cpu().numpy()
        np.save(os.path.join(dirname, f"{name}_sample.npy"), vals)
        np.save(os.path.join(dirname, f"{name}_sample_index.npy"), idx.astype(np.float64))
        written[name] = {"file": f"{name}_sample.npy", "index_file": f"{name}_sample_index.npy", "shape": list(t.shape),
                         "sampled": True, "sample_elements": DUMP_SAMPLE, "seed": DUMP_SEED}
    return written


def spawn_ranks(args):
    """Parent of a plain `python bench.py --gpus N`: start N fresh rank processes (this process has not touched the
    GPU and never will), relay rank 0's stdout, exit with the worst return code.  If one rank dies the others are
    ended (by PID) instead of waiting for a rendezvous that cannot complete."""
    import tempfile
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    out0 = tempfile.TemporaryFile(mode="w+")
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=out0 if r == 0 else subprocess.DEVNULL))
    worst = 0
    live = list(procs)
    while live:
        time.sleep(0.2)
        for p in list(live):
            rc = p.poll()
            if rc is None:
                continue
            live.remove(p)
            if rc != 0:
                worst = max(worst, abs(rc) or 1)
                for q in live:
                    q.terminate()
    out0.seek(0)
    sys.stdout.write(out0.read())
    sys.stdout.flush()
    sys.exit(worst)


RENDEZVOUS_TIMEOUT_S = int(os.environ.get("LITHO_BENCH_TIMEOUT_S", "300"))


def die(rank, what, exc=None):
    """End THIS rank with a non-zero code and its name on stderr (never a re-exec: the process has touched the GPU).
    os._exit: a process group whose peer is gone can hang in its destructor."""
    sys.stderr.write(f"bench.py: rank {rank}: {what}" + (f": {exc!r}" if exc is not None else "") + "\n")
    sys.stderr.flush()
    sys.stdout.flush()
    os._exit(3)


def check_in(store, rank, world, phase, timeout_s=None):
    """Bounded host-side rendezvous through the process group's store: every rank posts a key and waits until all keys of the
    phase are there; after timeout_s the ranks that never arrived are NAMED and this rank exits non-zero -- a missing peer
    costs minutes, not the lease (a collective would wait for its own, longer, watchdog)."""
    if store is None:
        return
    timeout_s = RENDEZVOUS_TIMEOUT_S if timeout_s is None else timeout_s
    try:
        store.set(f"litho_bench/{phase}/{rank}", "1")
        deadline = time.monotonic() + timeout_s
        while True:
            missing = [r for r in range(world) if not store.check([f"litho_bench/{phase}/{r}"])]
            if not missing:
                return
            if time.monotonic() > deadline:
                die(rank, f"phase '{phase}': rank(s) {missing} of {world} did not arrive within {timeout_s} s")
            time.sleep(0.002)
    except SystemExit:
        raise
    except Exception as exc:                                     # the store itself is gone: its server rank died
        die(rank, f"phase '{phase}': rendezvous store unreachable", exc)


SHORT_STEP_MS = 5.0


def event_timed_steps(torch, step, steps):
    """K more steps with a HIP event in front of each (and one behind the last): per-step times on the launch stream.  Used for
    SHORT steps only (config 1: 0.46 ms), where an event marker between two images is itself 3-5 % of the step (the packet drains
    the queue) and therefore stays OUT of the fenced region `value` is taken from; long steps carry their marks inside it."""
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    for i in range(steps):
        marks[i].record()
        step()
    marks[steps].record()
    torch.cuda.synchronize()
    return [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]


class Workload:
    """Synthetic inputs of one BASELINE configuration, resident on the device."""

    def __init__(self, name, dev):
        import torch
        import lithographysimulator_amd as L
        from lithographysimulator_amd.synthetic import bernoulli_mask
        self.name = name
        self.pn, skind, ab, self.planes, self.desc = WORKLOADS[name]
        pn = self.pn
        with contextlib.redirect_stdout(sys.stderr):         # the object API prints reference-style notices
            self.mask = L.Mask(bernoulli_mask(pn), PS, dev)
            self.maskFT = self.mask.fraunhofer(WL, True)
            self.epsilon, self.N = self.mask.calculateEpsilonN(self.mask.deltaK, PS, WL)
            if skind == "circ":
                self.bitmap = L.LightSource(0.0, 0.5, pn, NA, device=dev).generateAnnular()
            else:
                ls = L.LightSource(0.4, 0.8, pn, NA, device=dev)
                self.bitmap = ls.generateAnnular() if skind == "annular" else ls.generateQuasar(4, -math.pi / 8)
            if self.planes == 1:
                self.pupil = L.Pupil(pn, WL, NA, None if ab is None else torch.tensor(ab, dtype=torch.float16), dev).generatePupilFunction()
            else:
                self.pupil = L.throughFocusPupils(pn, WL, NA, torch.tensor(ab, dtype=torch.float16),
                                                  [float(d) for d in DEFOCUS_NM[:self.planes]], dev)
        self.S_full = int(self.bitmap.sum())
        self.dev = dev
        torch.cuda.synchronize()

    def step(self, lo=0, hi=None, group=None, plan_cache=None):
        """One complete image: the whole source list through abbeImage, or the slice [lo, hi) through the three calls
        abbeImage makes per rank."""
        import lithographysimulator_amd as L
        if hi is None or (lo, hi) == (0, self.S_full):
            return L.abbeImage(self.mask, self.maskFT, self.pupil, self.bitmap, PS, self.mask.deltaK, WL, True, self.dev, group=group,
                               plan_cache=plan_cache)
        sh = L.sourceShifts(self.bitmap, self.pn)[lo:hi]
        return L.postProcess(L.abbeIntensity(self.maskFT, self.pupil, sh, self.N), self.epsilon)


def kernel_profile(nat, prof, plan, pn, N, pe=None):
    """Per-kernel-class figures of one profiled call (HIP events recorded by the library on the launch stream).
    pe: the grid the engine ran at when the problem was evaluated embedded (a mask size other than N and N / 2)."""
    pe = pe or pn
    lines = {"xpass": plan["box_rows"], "ypass": pe}            # lines transformed per T item
    n_exec = pe if plan.get("coarse_grid") else N                # coarse-grid path: pe-point transforms on the grid q = 2 v
    line_flops = 5.0 * n_exec * math.log2(n_exec)                # nominal FFT flops of one transformed line
    kern = {}
    for k in ("xpass", "ypass"):
        launches = max(1, prof[f"{k}_launches"])
        items = prof[f"{k}_points"]                              # T items = source points x planes
        avg_ms = prof[f"{k}_ms"] / launches
        per_launch = items / launches
        flops = line_flops * lines[k] * per_launch
        algo_bytes = ALGO_BYTES[k] * pn * pn * per_launch
        kern[k] = {"kernel": prof[f"{k}_kernel"], "avg_launch_ms": avg_ms, "launches": launches, "items_per_launch": per_launch,
                   "nominal_flops_per_launch": flops,
                   "achieved_TFLOPs": flops / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0,
                   "algorithmic_bytes_per_launch": algo_bytes,
                   "effective_GBs": algo_bytes / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0,
                   "total_ms": prof[f"{k}_ms"]}
    return kern, n_exec


def attach_traffic(workload, kern, plan):
    """PMC-derived memory-side bytes (rocprofv3 --pmc passes over this very command: profiles/traffic.json) onto the kernel
    records of one workload; returns the entry's provenance string.  Counters are only meaningful for the kernel AND the launch
    geometry they were collected on: an entry made for another kernel (a renamed / re-parametrised variant since the capture)
    or for another batch / group count / chunk (a host-side change that leaves the kernel names alone) is dropped, not reused."""
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if not os.path.exists(tpath):
        return None
    try:
        entry = json.load(open(tpath)).get(workload, {})
    except Exception:
        return None
    src = entry.get("source")
    if entry.get("commit"):
        src = f"{src} [captured at commit {entry['commit']}]"
    geo = entry.get("geometry")
    geo_now = {k: plan.get(k) for k in GEOMETRY_KEYS}
    for k in kern:
        per_item = entry.get(k + "_bytes_per_item")
        made_for = entry.get(k + "_kernel")
        if made_for is not None and made_for != kern[k]["kernel"]:
            kern[k]["traffic_stale"] = f"profiles/traffic.json holds counters of {made_for}, this run launched {kern[k]['kernel']}"
            continue
        if geo is None or any(geo.get(g) != geo_now[g] for g in GEOMETRY_KEYS):
            kern[k]["traffic_stale"] = f"profiles/traffic.json was captured with launch geometry {geo}, this run planned {geo_now}"
            continue
        if per_item is not None and kern[k]["avg_launch_ms"] > 0:
            kern[k]["traffic"] = per_item * kern[k]["items_per_launch"]
            kern[k]["fabric_GBs"] = kern[k]["traffic"] / (kern[k]["avg_launch_ms"] * 1e-3) / 1e9
            kern[k]["fabric_frac"] = kern[k]["fabric_GBs"] / HBM_PEAK_GBS
    return src


INFINITY_CACHE_BYTES = 256 << 20


def hbm_streaming(kern, plan, pe):
    """The HBM-honest figure (round-4 review, item 3).  rocprofv3 on this image offers no counter behind the Infinity Cache
    (profiles/r05_rocprofv3_counter_list.txt: no DF / UMC / MALL block), so fabric bytes equal HBM bytes only where the cache
    cannot hold the working set: when one launch pair's T (batch x item, written once by the x-pass and read once by the
    y-pass, everything else is small) is several times the 256 MiB cache.  True for 4096^2 (67 MB x 60 items = 4 GB), false for
    the cache-sized batches of 2048^2 and below.  Then: (x-pass + y-pass PMC bytes per item) / (their time per item) against
    the 8 TB/s peak."""
    t_item = float(plan["box_rows"]) * pe * 8.0
    batch_bytes = t_item * plan["batch"] * max(1, plan["planes_in_flight"])
    streams = batch_bytes >= 4 * INFINITY_CACHE_BYTES
    out = {"hbm_streaming": streams, "T_bytes_per_launch_pair": batch_bytes, "infinity_cache_bytes": INFINITY_CACHE_BYTES}
    if not streams:
        out["note"] = ("one launch pair's T fits the Infinity Cache (by design): fabric bytes are NOT HBM bytes here, and no counter "
                       "behind the cache exists on this image (profiles/r05_rocprofv3_counter_list.txt)")
        return out
    if all("traffic" in kern[k] for k in ("xpass", "ypass")):
        per_item_bytes = sum(kern[k]["traffic"] / kern[k]["items_per_launch"] for k in ("xpass", "ypass"))
        per_item_s = sum(kern[k]["avg_launch_ms"] * 1e-3 / kern[k]["items_per_launch"] for k in ("xpass", "ypass"))
        out.update({"bytes_per_item": per_item_bytes, "us_per_item": per_item_s * 1e6,
                    "hbm_GBs": per_item_bytes / per_item_s / 1e9, "hbm_frac": per_item_bytes / per_item_s / 1e9 / HBM_PEAK_GBS,
                    "per_kernel_hbm_frac": {k: kern[k]["fabric_frac"] for k in ("xpass", "ypass")},
                    "note": "T streams through HBM (working set >> Infinity Cache): PMC fabric bytes of x-pass + y-pass per item over "
                            "their HIP-event time per item, against 8 TB/s -- the one honest HBM-roofline fraction of this engine"})
    else:
        out["note"] = "T streams through HBM, but profiles/traffic.json has no current counters for these kernels / this geometry"
    return out


def measured_ceilings(torch, dev):
    """Device-copy and device-fill rates of THIS box (1 GiB, beyond the 256 MiB Infinity Cache): what the memory
    system sustains for plain streams, to put next to the 8 TB/s spec the fractions are quoted against."""
    try:
        a = torch.empty(1 << 28, dtype=torch.float32, device=dev); b = torch.empty_like(a)
        b.copy_(a); a.zero_(); torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        for _ in range(5): b.copy_(a)
        e1.record()
        for _ in range(5): a.zero_()
        e2.record(); torch.cuda.synchronize()
        copy_gbs = 5 * 2 * a.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9      # read + write bytes
        fill_gbs = 5 * a.numel() * 4 / (e1.elapsed_time(e2) * 1e-3) / 1e9          # write bytes
        del a, b
        return copy_gbs, fill_gbs
    except Exception:
        return None, None


# What an N-GPU step should take, stated BEFORE any N > 1 run has ever executed (one GPU per lease in the build rounds; DESIGN.md
# section 5): per rank exactly its shard of the single-GPU step -- the per-point cost is shift-independent, planning and the
# once-per-image reconstruction do not shrink -- plus ONE all-reduce priced per xGMI link (ring: 2 (N-1)/N of the buffer through
# ~100 GB/s effective per direction).  single_gpu_ms: measured on one MI355X this round (profiles/r05_bench*.json; cfg4 = 8 x its
# measured shard); fixed_ms: plan read-back + coarse-grid reconstruction + post-process, which every rank repeats.
PREDICTION = {"cfg1": {"single_gpu_ms": 0.55, "fixed_ms": 0.25}, "cfg2": {"single_gpu_ms": 194.0, "fixed_ms": 0.6},
              "cfg3": {"single_gpu_ms": 1680.0, "fixed_ms": 1.5}, "cfg4": {"single_gpu_ms": 55600.0, "fixed_ms": 6.0},
              "cfg5": {"single_gpu_ms": 53900.0, "fixed_ms": 40.0}}
XGMI_EFFECTIVE_GBS = 100.0
PREDICTION_SOURCE = "literals in bench.py (profiles/r05_bench*.json)"


def _load_prediction_inputs():
    """single_gpu_ms from the round's committed bench line (profiles/prediction_inputs.json, written by scripts/collect_profiles.py
    from profiles/<round>_bench.json) instead of literals that drift without notice (round-5 advice); fixed_ms stays as stated."""
    global PREDICTION_SOURCE
    path = os.path.join(ROOT, "profiles", "prediction_inputs.json")
    try:
        data = json.load(open(path))
        for k, v in data.get("single_gpu_ms", {}).items():
            if k in PREDICTION and isinstance(v, (int, float)) and v > 0:
                PREDICTION[k] = dict(PREDICTION[k], single_gpu_ms=float(v))
        PREDICTION_SOURCE = f"profiles/prediction_inputs.json ({data.get('source')})"
    except Exception:
        pass


_load_prediction_inputs()


def predicted_step(workload, world, allreduce_bytes):
    p = PREDICTION.get(workload)
    if not p:
        return None
    ar_ms = 2.0 * (world - 1) / world * allreduce_bytes / (XGMI_EFFECTIVE_GBS * 1e9) * 1e3 if world > 1 else 0.0
    ms = (p["single_gpu_ms"] - p["fixed_ms"]) / world + p["fixed_ms"] + ar_ms
    return {"predicted_step_ms": ms, "predicted_speedup": p["single_gpu_ms"] / ms, "predicted_allreduce_ms": ar_ms,
            "single_gpu_ms_assumed": p["single_gpu_ms"], "single_gpu_ms_source": PREDICTION_SOURCE,
            "note": "stated before the first N > 1 run: (single_gpu_ms - fixed_ms) / N + fixed_ms + ring all-reduce at "
                    f"{XGMI_EFFECTIVE_GBS:.0f} GB/s per link direction (DESIGN.md section 7); compare with ms_per_step and ranks.*"}


CPU_SAMPLE_POINTS = {256: 64, 1024: 16, 2048: 8, 4096: 4}      # BASELINE.md / SURVEY 8d: K source points per grid size


def cpu_baseline_prepare(torch, nat, w, plan, full=False):
    """GPU half of the CPU-baseline leg, run while the workload is still resident: the K sample points through the GPU on
    the evaluation path the timed step ran (options, not the environment), and host copies of what the CPU half needs.
    The CPU half (cpu_baseline_run) is run AFTER every GPU timing of the bench (round-4 advice: the CPU legs used to sit
    between the extra workloads' GPU timings and left torch's thread setting changed behind them)."""
    import lithographysimulator_amd as L
    pn, N, planes, S_full, dev = w.pn, w.N, w.planes, w.S_full, w.dev
    shifts = L.sourceShifts(w.bitmap, pn)
    K = S_full if full else CPU_SAMPLE_POINTS.get(pn, 8)
    sel = shifts.cpu() if full else shifts[(torch.arange(K, device=dev) * S_full) // K].cpu()
    p_one = w.pupil if planes == 1 else w.pupil[planes // 2]
    # the parity sample runs the evaluation path of the TIMED step (a handful of points would otherwise fall below
    # the coarse-grid path's source-count threshold and check the direct kernels instead)
    gpu_raw = L.abbeIntensity(w.maskFT, p_one, sel.to(dev), N, options={"coarse": 2 if plan.get("coarse_grid") else 0}).cpu()
    parity_plan = nat.last_plan()
    assert parity_plan["coarse_grid"] == plan.get("coarse_grid"), (parity_plan, plan)
    return {"pn": pn, "N": N, "planes": planes, "S_full": S_full, "K": K, "full": full, "sel": sel, "m_cpu": w.maskFT.cpu(),
            "p_cpu": p_one.cpu(), "gpu_raw": gpu_raw, "parity_plan": parity_plan, "kernels": list(nat.last_kernels())}


def cpu_baseline_run(torch, st, reps=3):
    """The reference's CPU path beside the GPU number, in the same run on the GPU box's own host cores: the oracle's
    torch-CPU op chain (oracle/abbe_oracle.py abbe_raw: roll / mul / pad / fftshift / ifft2 / ifftshift / crop / abs^2 / add,
    a port of imageformation.py:62-67; the reference's Python itself does not travel to the GPU box) over K source points
    strided through the real list -- the loop is strictly linear in S -- or, `full`, over the WHOLE list once (config 1, as
    BASELINE.md asks), compared with the GPU image of the same points (cpu_baseline_prepare).  Reported, not optimised."""
    from oracle import abbe_oracle as O
    pn, N, planes, S_full, K, full, sel = (st[k] for k in ("pn", "N", "planes", "S_full", "K", "full", "sel"))
    m_cpu, p_cpu, gpu_raw, parity_plan = st["m_cpu"], st["p_cpu"], st["gpu_raw"], st["parity_plan"]
    # 32 threads is the fastest setting for this op chain on the GPU box's 2 x EPYC 9575F (256 hw threads:
    # 8 -> 2.1e7, 32 -> 2.6e7, 256 -> 1.6e6 pt*px/s; scripts/cpu_threads_probe.py), so that is the baseline.
    host_cpus = os.cpu_count() or 1
    threads_before = torch.get_num_threads()
    torch.set_num_threads(min(host_cpus, 32))
    try:
        cores = torch.get_num_threads()
        O.abbe_raw(m_cpu, p_cpu, sel[:1], N)                        # warm-up
        times = []
        for _ in range(1 if full else reps):
            c0 = time.perf_counter()
            ref_raw = O.abbe_raw(m_cpu, p_cpu, sel, N)
            times.append(time.perf_counter() - c0)
    finally:
        torch.set_num_threads(threads_before)
    tmed = statistics.median(times)
    parity = float((gpu_raw - ref_raw).abs().max() / ref_raw.max())
    how = (f"ALL {K} source points of the list, once, {tmed:.2f} s" if full else
           f"{K} source points strided through the {S_full}-point list, 1 warm-up + {reps} reps, median {tmed:.2f} s")
    return {"value": K * pn * pn / tmed, "unit": "source-pt*px/s", "cores": cores, "host_cpus": host_cpus,
            "kind": "port",
            "sample": how + f", full {pn}x{pn} grid" + (f", plane {planes // 2} of {planes}" if planes > 1 else "") +
                      "; oracle/abbe_oracle.py abbe_raw (torch-CPU roll/mul/pad/fftshift/ifft2/ifftshift/crop/abs2/add)",
            "seconds": tmed, "source_points": K,
            "gpu_vs_cpu_rel_to_max": parity,
            "parity_path": {"coarse_grid": parity_plan["coarse_grid"], "kernels": st["kernels"]}}


def extra_workload(torch, nat, dev, name, shard=None, steps=1, warm_points=0, warm_steps=1, profile_points=480, cpu=True):
    """One or two timed steps of another BASELINE configuration (same fences as the headline), plus a short profiled
    run for the x-pass / y-pass split."""
    import lithographysimulator_amd as L
    w = Workload(name, dev)
    lo, hi = 0, w.S_full
    note = None
    if shard:
        from lithographysimulator_amd.distributed import shard_bounds
        lo, hi = shard_bounds(w.S_full, shard[0], shard[1])
        note = f"shard {shard[0]}/{shard[1]} of the source list (per-rank work of the {shard[1]}-GPU run, no all-reduce)"
    if warm_points:                                              # allocate the workspace, warm the code objects
        w.step(lo, min(hi, lo + warm_points))
        short = False
    else:
        for i in range(max(1, warm_steps)):
            if i == max(1, warm_steps) - 1:                      # the last warm-up step is clocked: is a step short? (event_timed_steps)
                torch.cuda.synchronize()
                tw = time.perf_counter()
            w.step(lo, hi)
        torch.cuda.synchronize()
        short = (time.perf_counter() - tw) * 1e3 < SHORT_STEP_MS
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    for i in range(steps):
        if not short:
            marks[i].record()
        image = w.step(lo, hi)
    if not short:
        marks[steps].record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    step_ms = (event_timed_steps(torch, lambda: w.step(lo, hi), steps) if short
               else [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)])
    plan = nat.last_plan()
    S = hi - lo
    units = float(S) * w.pn * w.pn * w.planes
    nat.set_profiling(True)
    sh = L.sourceShifts(w.bitmap, w.pn)[lo:min(hi, lo + profile_points)]
    L.abbeIntensity(w.maskFT, w.pupil if w.planes == 1 else w.pupil[:2], sh, w.N)
    torch.cuda.synchronize()
    prof = nat.last_profile()
    kern, n_exec = kernel_profile(nat, prof, nat.last_plan(), w.pn, w.N, L.embeddedSize(w.pn, w.N))
    nat.set_profiling(False)
    attach_traffic(name, kern, nat.last_plan())
    both = kern["xpass"]["total_ms"] + kern["ypass"]["total_ms"]
    dom = "ypass" if kern["ypass"]["total_ms"] >= 0.95 * kern["xpass"]["total_ms"] else "xpass"   # as in the headline
    out = {"workload": (f"BASELINE {name}: " if name.startswith("cfg") else f"{name}: ") + w.desc + (f" [{note}]" if note else ""), "steps": steps,
           "ms_per_step": elapsed / steps * 1e3, "median_ms_per_step": statistics.median(step_ms), "step_ms": step_ms,
           "step_ms_events_inside_timed_region": not short,
           "value": units * steps / elapsed, "unit": "source-pt*px/s",
           "source_points": S, "source_points_full": w.S_full, "planes": w.planes, "pn": w.pn, "fft_n": w.N,
           "executed_fft_n": n_exec, "image_shape": list(image.shape), "plan": plan,
           "embedded_in": L.embeddedSize(w.pn, w.N) if L.embeddedSize(w.pn, w.N) != w.pn else None,
           "dominant_kernel": kern[dom]["kernel"], "dominant_kernel_time_frac": kern[dom]["total_ms"] / both if both else None,
           "dominant_kernel_valu_frac": kern[dom]["achieved_TFLOPs"] / VALU_PEAK_TFLOPS,
           "kernels": {k: {kk: v[kk] for kk in ("kernel", "avg_launch_ms", "items_per_launch", "traffic", "fabric_GBs", "fabric_frac",
                                                "traffic_stale") if kk in v}
                       for k, v in kern.items()},
           "hbm_honest": hbm_streaming(kern, nat.last_plan(), L.embeddedSize(w.pn, w.N)),
           "target_abs": {"per_gpu": TARGET_ABS_PER_GPU, "value_over_target": units * steps / elapsed / TARGET_ABS_PER_GPU},
           "profile_sample": f"first {sh.shape[0]} consecutive source points" + (" x 2 planes" if w.planes > 1 else "")}
    if name == "cfg1":
        # the same image as one of a SEQUENCE sharing pupil and source (PlanCache: no compaction, no planning launches, no
        # host wait from the second call on), 100 images back to back
        cache = L.PlanCache()
        for _ in range(3):
            w.step(plan_cache=cache)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(100):
            image = w.step(plan_cache=cache)
        torch.cuda.synchronize()
        t_seq = (time.perf_counter() - t0) / 100
        out["sequence_with_plan_cache"] = {"images": 100, "ms_per_image": t_seq * 1e3, "value": units / t_seq}
    if cpu:
        try:
            out["_cpu_state"] = cpu_baseline_prepare(torch, nat, w, plan, full=(name == "cfg1"))   # the CPU half runs after every GPU timing
        except Exception as exc:
            out["cpu_baseline"] = {"error": repr(exc)}
    del w, image
    torch.cuda.empty_cache()
    return out


def roofline_leg(torch, nat, L, step, dev, workload, pn, N):
    """--full: HIP-event time of each kernel class over one more (untimed) step of this rank's shard, the device's copy and fill
    rates, and the PMC traffic of profiles/traffic.json against them.  Returns (roofline, plan, executed FFT size)."""
    nat.set_profiling(True)
    step()
    torch.cuda.synchronize()
    prof = nat.last_profile()
    plan = nat.last_plan()
    nat.set_profiling(False)
    copy_gbs, fill_gbs = measured_ceilings(torch, dev)
    kern, n_exec = kernel_profile(nat, prof, plan, pn, N, L.embeddedSize(pn, N))
    # The two pass kernels share the time almost evenly (50.3 % / 49.1 % under rocprofv3) and trade places from run to
    # run; `roofline` describes the y-pass -- the VALU-bound one, for which a flop fraction means something -- unless the
    # x-pass leads by more than 5 %.  Both kernels carry their own figures (and their measured bound) under `kernels`.
    dom = "ypass" if kern["ypass"]["total_ms"] >= 0.95 * kern["xpass"]["total_ms"] else "xpass"
    traffic_src = attach_traffic(workload, kern, plan)
    traffic = kern[dom].get("traffic")
    kern["ypass"]["bound"] = "valu: fp32 issue + per-wave serial latency (load wait, LDS transposes); profiles/r03_ypass_lab.txt"
    kern["xpass"]["bound"] = ("fabric: the T stores (64-byte granules through the L2 to the Infinity Cache); without them the "
                              "kernel takes 0.6 of its time (profiles/r02_xpass_diag_variants.txt, r03_ypass_lab.txt)")
    for k in kern:
        kern[k]["valu_frac"] = kern[k]["achieved_TFLOPs"] / VALU_PEAK_TFLOPS
    both_ms = kern["xpass"]["total_ms"] + kern["ypass"]["total_ms"]
    both_flops = sum(kern[k]["nominal_flops_per_launch"] * kern[k]["launches"] for k in kern)
    eff40 = 40.0 * pn * pn * prof["ypass_points"] / (both_ms * 1e-3) / 1e9 if both_ms else 0.0
    dom_s = kern[dom]["avg_launch_ms"] * 1e-3
    fabric_gbs = traffic / dom_s / 1e9 if traffic and dom_s > 0 else None
    # "bound" takes the contract's two values ("hbm" | "mfma"): this is the flop side -- priced against the dense fp32 peak,
    # 157.3 TFLOP/s, which on gfx950 is the same figure for the matrix and the vector pipe; `bound_detail` says which pipe
    roofline = {"bound": "mfma", "bound_measured": "valu", "bound_detail": "VALU: fp32 vector issue, NOT the matrix pipe -- the path has no MFMA instruction; \"mfma\" is the "
                                                  "contract's name for the flop side, priced at the dense fp32 peak, which on gfx950 is "
                                                  "157.3 TFLOP/s for the vector and the matrix pipe alike", "kernel": kern[dom]["kernel"],
                "achieved": kern[dom]["achieved_TFLOPs"], "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": kern[dom]["achieved_TFLOPs"] / VALU_PEAK_TFLOPS, "traffic": traffic,
                "avg_launch_ms": kern[dom]["avg_launch_ms"],
                "nominal_flops_per_launch": kern[dom]["nominal_flops_per_launch"],
                "kernel_time_frac": kern[dom]["total_ms"] / both_ms if both_ms else None,
                "fabric_GBs": fabric_gbs, "fabric_frac": fabric_gbs / HBM_PEAK_GBS if fabric_gbs else None,
                "effective_40B_GBs": eff40, "effective_40B_over_peak": eff40 / HBM_PEAK_GBS,
                "copy_ceiling_GBs": copy_gbs, "fill_ceiling_GBs": fill_gbs, "hbm_peak_GBs": HBM_PEAK_GBS,
                "note": "kernel: the y-pass unless the x-pass leads it by more than 5 % (they share the time 50 / 50 and trade "
                        "places from run to run; both are under `kernels` with their own bound).  "
                        "bound: fp32 VALU issue (profiles/r03_*: the kernel's instruction stream issues at 1.9 ns per "
                        "instruction per SIMD against a measured 1.0-1.26 ns floor at two waves per SIMD; packed fp32 "
                        "gives no extra rate on gfx950).  achieved = nominal 5*N*log2(N) flops per transformed line "
                        "(pruned transforms execute fewer) / HIP-event launch time.  traffic / fabric_* = PMC bytes the "
                        "L2 exchanged with the fabric per launch of this workload, Infinity-Cache hits INCLUDED (T is kept "
                        "inside that cache on purpose): an upper bound on HBM traffic, not HBM traffic.  effective_40B_* "
                        "divide the SURVEY 8d byte MODEL by x-pass + y-pass kernel time: most of those bytes are never "
                        "moved, so it exceeds the peak and is not a roofline fraction.  avg_launch_ms comes from HIP events the "
                        "library records around every launch of ONE extra, untimed step: the marks themselves cost about 4 % "
                        "(launches x avg_launch_ms of both kernels exceeds ms_per_step by that much), so achieved / frac are "
                        "slightly conservative; rocprofv3 --kernel-trace of the same command (profiles/) has the unmarked durations",
                "traffic_source": traffic_src,
                "hbm_honest": hbm_streaming(kern, plan, L.embeddedSize(pn, N)),
                "pipeline": {"achieved": both_flops / (both_ms * 1e-3) / 1e12 if both_ms else 0.0,
                             "frac": both_flops / (both_ms * 1e-3) / 1e12 / VALU_PEAK_TFLOPS if both_ms else 0.0,
                             "note": "x-pass + y-pass nominal flops over their summed kernel time"},
                "kernels": kern}
    return roofline, plan, n_exec


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and (args.gpus or 1) > 1:
        spawn_ranks(args)

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus is not None and args.gpus != world:
        # a launcher that started another number of ranks than the command line NAMES would silently report the wrong n_gpus;
        # without --gpus the launcher's WORLD_SIZE is simply adopted (`torchrun --nproc-per-node N bench.py`)
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node equal to --gpus")
    args.gpus = world
    # Test hooks (tests/test_gpu_bench_contract.py): on a box with ONE GPU the multi-rank code path of this file is
    # exercised with every rank on cuda:0 and a gloo group (RCCL refuses two ranks on one device).
    backend = os.environ.get("LITHO_BENCH_BACKEND", "nccl")
    share_gpu = os.environ.get("LITHO_BENCH_SHARE_GPU") == "1"
    dev = torch.device("cuda", 0 if share_gpu else local_rank)
    torch.cuda.set_device(dev)
    group = None
    store = None
    backend_fallback = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # First contact with a multi-GPU node must end in minutes with the guilty rank named, not at the lease limit: the
        # rendezvous and every collective carry a timeout (RCCL: the process group's watchdog aborts a collective that does not
        # complete in time), and before the timed region every rank checks in through the rendezvous store (check_in).
        tmo = timedelta(seconds=RENDEZVOUS_TIMEOUT_S)
        try:
            if backend == "nccl":
                if os.environ.get("LITHO_BENCH_FORCE_RCCL_FAIL") == "1":     # test hook: the fallback below, on a one-GPU box
                    raise RuntimeError("LITHO_BENCH_FORCE_RCCL_FAIL=1")
                dist.init_process_group("nccl", device_id=dev, timeout=tmo)      # "nccl" is RCCL on ROCm
                probe = torch.ones(1, dtype=torch.float32, device=dev)           # first contact: one tiny collective, checked
                dist.all_reduce(probe)
                if float(probe.item()) != float(world):
                    raise RuntimeError(f"RCCL probe all-reduce returned {float(probe.item())}, expected {world}")
            else:
                dist.init_process_group(backend, timeout=tmo)
        except Exception as exc:
            if backend != "nccl" or os.environ.get("LITHO_BENCH_NO_FALLBACK") == "1":
                die(rank, f"rendezvous of {world} ranks at {os.environ.get('MASTER_ADDR')}:{os.environ.get('MASTER_PORT')} failed "
                          f"within {RENDEZVOUS_TIMEOUT_S} s", exc)
            # RCCL could not be brought up on this node: a record with the collective staged through the host (gloo: the 16.8 MB
            # image of config 3 costs tens of milliseconds that way) says more than no record -- LABELLED as such in `ranks`.
            sys.stderr.write(f"bench.py: rank {rank}: RCCL initialisation failed ({exc!r}); falling back to a gloo group "
                             "(all-reduce staged through the host)\n")
            backend_fallback = repr(exc)
            try:
                if dist.is_initialized():
                    dist.destroy_process_group()
            except Exception:
                pass
            os.environ["MASTER_PORT"] = str(int(os.environ.get("MASTER_PORT", "29500")) + 1)
            backend = "gloo"
            try:
                dist.init_process_group("gloo", timeout=tmo)
            except Exception as exc2:
                die(rank, f"gloo fallback rendezvous of {world} ranks failed as well", exc2)
        group = dist.group.WORLD
        assert dist.get_world_size() == world == args.gpus, (dist.get_world_size(), world, args.gpus)
        try:
            store = dist.distributed_c10d._get_default_store()
        except Exception:
            store = None
        check_in(store, rank, world, "initialised")

    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat

    w = Workload(args.workload, dev)
    pn, planes, N, S_full = w.pn, w.planes, w.N, w.S_full

    # ---- what one step processes
    lo, hi, shard_note = 0, S_full, None
    if args.shard:
        if world > 1:
            sys.exit("--shard is a single-GPU option")
        i, n = (int(v) for v in args.shard.split("/"))
        from lithographysimulator_amd.distributed import shard_bounds
        lo, hi = shard_bounds(S_full, i, n)
        shard_note = f"shard {i}/{n} of the source list (per-rank work of the {n}-GPU run, no all-reduce)"
    if args.points > 0:
        hi = min(hi, lo + args.points)
        shard_note = (shard_note + "; " if shard_note else "") + f"PARTIAL: first {hi - lo} consecutive source points only"
    S = hi - lo

    def step():
        return w.step(lo, hi, group=group)

    def fence(phase=None):
        torch.cuda.synchronize()
        if world > 1:
            if phase:
                check_in(store, rank, world, phase)               # host side, names the ranks that never arrived
            try:
                dist.barrier()
            except Exception as exc:                              # a peer died between its check-in and the barrier
                die(rank, f"barrier '{phase or 'end of timed region'}' failed", exc)
            torch.cuda.synchronize()

    short = False
    for i in range(args.warmup):
        if i == args.warmup - 1:                                  # the last warm-up step is clocked: is a step short?
            torch.cuda.synchronize()
            tw = time.perf_counter()
        step()
    if args.warmup > 0:
        torch.cuda.synchronize()
        short = (time.perf_counter() - tw) * 1e3 < SHORT_STEP_MS
    fence("warm-up done")
    # per-step HIP events on the launch stream beside the host clock (median of >= 5 event-timed calls): marks[i]
    # is recorded before step i, marks[K] after the last one.  Short steps (config 1) are event-timed in a pass of their own.
    if world > 1:                                                 # every rank takes the same branch
        flag = torch.tensor([1.0 if short else 0.0], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        short = bool(flag.item() > 0.5)
    fence()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    for i in range(args.steps):
        if not short:
            marks[i].record()
        image = step()
    if not short:
        marks[args.steps].record()
    fence()
    elapsed_own = time.perf_counter() - t0
    # short steps: their event pass is K more steps of its own (--full only)
    step_ms = (None if short and not args.full else event_timed_steps(torch, step, args.steps) if short
               else [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)])
    own_median = statistics.median(step_ms) if step_ms else None
    elapsed, median_ms = elapsed_own, own_median
    ranks = None
    if world > 1:
        cdev = dev if backend == "nccl" else "cpu"
        t = torch.tensor([elapsed_own, own_median or 0.0], dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t[0].item())
        median_ms = float(t[1].item()) if own_median is not None else None
    if world > 1 and args.full:
        # one more, instrumented step: this rank's compute (its shard of the Abbe sum) and the all-reduce, by events
        from lithographysimulator_amd.distributed import shard_bounds
        from lithographysimulator_amd.imageformation import _all_reduce_sum
        sh_all = L.sourceShifts(w.bitmap, pn)
        rlo, rhi = shard_bounds(sh_all.shape[0], rank, world)
        fence()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        h0 = time.perf_counter()
        e0.record()
        part = L.abbeIntensity(w.maskFT, w.pupil, sh_all[rlo:rhi], N)
        e1.record()
        torch.cuda.synchronize()
        h1 = time.perf_counter()
        _all_reduce_sum(part, group)
        e2.record()
        torch.cuda.synchronize()
        h2 = time.perf_counter()
        mine = torch.tensor([elapsed_own / args.steps * 1e3, e0.elapsed_time(e1), (h2 - h1) * 1e3, float(rhi - rlo),
                             own_median], dtype=torch.float64, device=cdev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        rows = [[float(v) for v in r.cpu()] for r in allr]
        # who the ranks are: device name + PCI address of every rank (two ranks on one device = a launch mistake on a real node)
        props = torch.cuda.get_device_properties(dev)
        ident = f"{props.name} pci {getattr(props, 'pci_domain_id', 0):04x}:{getattr(props, 'pci_bus_id', 0):02x}:{getattr(props, 'pci_device_id', 0):02x} cuda:{dev.index}"
        idents = [None] * world
        try:
            dist.all_gather_object(idents, ident)
        except Exception as exc:                                  # identities are a diagnostic: never cost the measurement
            idents = [f"unavailable: {exc!r}"] * world
        try:
            rccl = ".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else None
        except Exception:
            rccl = None
        ranks = {"step_ms": [r[0] for r in rows], "compute_ms": [r[1] for r in rows],
                 "allreduce_wait_ms": [r[2] for r in rows], "source_points": [int(r[3]) for r in rows],
                 "step_ms_max": max(r[0] for r in rows), "step_ms_min": min(r[0] for r in rows),
                 "median_step_ms": [r[4] for r in rows],
                 "compute_ms_max": max(r[1] for r in rows), "compute_ms_min": min(r[1] for r in rows),
                 "allreduce_wait_ms_max": max(r[2] for r in rows), "allreduce_wait_ms_min": min(r[2] for r in rows),
                 "allreduce_bytes": int(part.numel() * 4),
                 "world": dist.get_world_size(), "backend": backend + (" (RCCL)" if backend == "nccl" else ""), "rccl_version": rccl,
                 "backend_fallback": backend_fallback,          # not None: RCCL could not be initialised, the all-reduce went through the host
                 "devices": idents, "distinct_devices": len(set(idents)) if not str(idents[0]).startswith("unavailable") else None,
                 "note": "step_ms = each rank's own mean over the timed steps, median_step_ms = its median by HIP events; compute_ms (HIP events) and "
                         "allreduce_wait_ms (host clock from this rank's compute done to its all-reduce done: "
                         "collective + waiting for the slowest rank) from one extra instrumented step"}
        del part, sh_all
    ms_per_step = elapsed / args.steps * 1e3
    units = float(S) * pn * pn * planes                          # source-point*pixels per step, whole job
    value = units * args.steps / elapsed

    if rank == 0 and args.dump_outputs:
        dumped = dump_outputs(args.dump_outputs, {"image": image})
    plan = nat.last_plan()
    n_exec = L.embeddedSize(pn, N) if plan.get("coarse_grid") else N
    roofline = None
    if args.full:
        roofline, plan, n_exec = roofline_leg(torch, nat, L, step, dev, args.workload, pn, N)

    out = {"metric": "Abbe source-points x image-pixels per second", "value": value, "unit": "source-pt*px/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
           # SURVEY 8d asks for the median of >= 5 event-timed calls (the slowest rank's); `value` stays the mean over the fenced region
           "median_ms_per_step": median_ms, "value_at_median": units / (median_ms * 1e-3) if median_ms else None,
           "step_ms": step_ms, "step_ms_events_inside_timed_region": not short,
           "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32",
           "data": "synthetic",
           "config": {"workload": (f"BASELINE {args.workload}: " if args.workload.startswith("cfg") else f"{args.workload}: ") + w.desc
                                  + (f" [{shard_note}]" if shard_note else ""),
                      "pn": pn, "fft_n": N, "executed_fft_n": n_exec, "source_points": S, "source_points_full": S_full, "planes": planes,
                      "points_per_rank": math.ceil(S / world),
                      # how often this process ran the step's kernels (warm-up + timed, with --full + the event pass of short steps + the
                      # profiled one): scripts/pmc_traffic.py divides whole-process counters by it
                      "step_executions": args.warmup + args.steps + ((args.steps if short else 0) + 1 if args.full else 0),
                      "pixel_size": PS, "wavelength": WL, "NA": NA,
                      "parallelism": f"source-point shards x{world}, one all-reduce" if world > 1 else "single GPU",
                      "plan": plan, "image_shape": list(image.shape)},
           "target_abs": {"per_gpu": TARGET_ABS_PER_GPU, "n_gpus": world, "value_over_target": value / (TARGET_ABS_PER_GPU * world),
                          "source": "BASELINE.md: >= 60 % of the 8 TB/s HBM roofline under the SURVEY 8d 40-byte model at 2048^2 = 1.2e11 "
                                    "source-pt*px/s per GPU (an EFFECTIVE figure: most of those 40 bytes are never moved)"}}
    if roofline is not None:
        out["roofline"] = roofline
    if ranks is not None:
        out["ranks"] = ranks
    if rank == 0 and args.dump_outputs:
        out["outputs"] = dumped
    if args.full and not args.shard and args.points == 0:
        pred = predicted_step(args.workload, world, planes * pn * pn * 4)
        if pred:
            # the record explains itself whichever way it comes out: measured step over predicted step, and (N > 1) where the
            # difference sits -- the slowest rank's compute against the prediction's compute share, the all-reduce wait against its price
            pred["measured_over_predicted"] = ms_per_step / pred["predicted_step_ms"]
            if ranks is not None:
                pred["compute_ms_max_over_predicted_compute"] = ranks["compute_ms_max"] / max(1e-9, pred["predicted_step_ms"] - pred["predicted_allreduce_ms"])
                pred["allreduce_wait_ms_min_over_predicted_allreduce"] = (ranks["allreduce_wait_ms_min"] / pred["predicted_allreduce_ms"]
                                                                          if pred["predicted_allreduce_ms"] > 0 else None)
            out["prediction"] = pred

    # ---- CPU baseline leg: the oracle's op-chain port of the reference loop, rank 0, N = 1 only.  GPU half now (the workload is
    # resident), CPU half after every GPU timing of this run
    cpu_state = None
    if args.full and world == 1 and not args.no_cpu_baseline:
        cpu_state = cpu_baseline_prepare(torch, nat, w, plan, full=(args.workload == "cfg1"))

    # ---- every other BASELINE configuration, one or two timed steps each (single-GPU --full run of the default workload only)
    if args.full and world == 1 and not args.no_extra and args.workload == "cfg3" and not args.shard and args.points == 0:
        del w, image
        torch.cuda.empty_cache()
        extras = []
        # (cfg1: 0.46 ms steps -- 20 of them are 9 ms, inside the clock ramp after an idle gap: 200)
        for name, kw in (("cfg1", dict(steps=200, warm_steps=20, profile_points=1 << 30)), ("cfg2", dict(steps=2, profile_points=4800)),
                         ("cfg4", dict(shard=(0, 8), steps=2, warm_points=600, profile_points=2400)),
                         ("cfg5", dict(steps=2 if args.steps >= 5 else 1, warm_points=240, profile_points=240)),
                         ("odd2000", dict(steps=1, warm_points=480, profile_points=480))):
            try:
                extras.append(extra_workload(torch, nat, dev, name, cpu=not args.no_cpu_baseline, **kw))
            except Exception as exc:                              # an extra must never cost the headline line
                extras.append({"workload": name, "error": repr(exc)})
        out["extra_workloads"] = extras

    # ---- the CPU halves, after all GPU timings (torch's thread setting is restored behind each)
    if cpu_state is not None:
        out["cpu_baseline"] = cpu_baseline_run(torch, cpu_state)
        cpu_state = None
    for e in out.get("extra_workloads", []):
        st = e.pop("_cpu_state", None)
        if st is not None:
            try:
                e["cpu_baseline"] = cpu_baseline_run(torch, st)
            except Exception as exc:
                e["cpu_baseline"] = {"error": repr(exc)}

    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
