"""What a weighted source costs: same-box A/B of the Abbe accumulation for BASELINE configs 3, 1 and config 4's shard 0/8,
    (a) unweighted on the PARENT's library (a build of the commit before weights existed, loaded through LITHO_ABBE_LIB),
    (b) unweighted on this build,
    (c) weighted on this build, random w in (0, 1]:

    python scripts/weighted_ab.py --parent-lib /path/to/parent/liblitho_abbe.so [--configs cfg3,cfg1,cfg4] [--out FILE]

Every (configuration, case) leg is a fresh child process under `timeout`; the legs alternate a, b, c, a, b, c (two rounds of
half the steps each, so that drift of the box hits the three cases alike); the script stops at the first non-zero status.
One step = one litho_abbe_accumulate* call over the whole source list (shifts already compacted), timed with HIP events;
besides the step times every leg reports the per-kernel times of one profiled call (litho_abbe_set_profiling).  Prints
mean / min / max and the step-to-step spread per case and the ratios b/a, c/a."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO_AB = [0, 0, 0.01, 0, 100, 0.01, 0, 0.01, 0.01, 0.01]
# name: (pn, source, aberrations, shard, timed steps per round, warm-up steps, time limit of one leg in seconds)
CONFIGS = {"cfg3": (2048, "quasar", DEMO_AB, None, 5, 1, 240), "cfg1": (256, "circ", None, None, 100, 20, 120),
           "cfg4": (4096, "annular", [0, 0, 0, 0, 100], (0, 8), 5, 1, 420)}


def child(cfg, case):
    import torch
    sys.path.insert(0, ROOT)
    from lithographysimulator_amd import _native as nat
    if case == "a":                                        # the parent's library does not have the weighted entries
        for name in ("litho_abbe_accumulate_weighted", "litho_source_compact_weighted"):
            nat._SIGNATURES.pop(name)
    import lithographysimulator_amd as L
    from lithographysimulator_amd.distributed import shard_bounds
    from lithographysimulator_amd.synthetic import bernoulli_mask
    pn, skind, ab, shard, steps, warm, _ = CONFIGS[cfg]
    dev = torch.device("cuda", 0)
    mask = L.Mask(bernoulli_mask(pn), 25, dev)
    mft = mask.fraunhofer(193., True)
    eps, N = mask.calculateEpsilonN(mask.deltaK, 25, 193.)
    pf = L.Pupil(pn, 193., 0.7, torch.tensor(ab, dtype=torch.float16) if ab is not None else None, dev).generatePupilFunction()
    ls = L.LightSource(0.0, 0.5, pn, 0.7, device=dev) if skind == "circ" else L.LightSource(0.4, 0.8, pn, 0.7, device=dev)
    sh = L.sourceShifts(ls.generateQuasar(4, -math.pi / 8) if skind == "quasar" else ls.generateAnnular(), pn)
    if shard:
        lo, hi = shard_bounds(sh.shape[0], *shard)
        sh = sh[lo:hi].contiguous()
    kw = {}
    if case == "c":
        g = torch.Generator().manual_seed(11)
        kw["weights"] = (1.0 - torch.rand(sh.shape[0], generator=g)).to(dev)
    out = torch.zeros((pn, pn), dtype=torch.float32, device=dev)
    for _ in range(warm):
        L.abbeIntensity(mft, pf, sh, N, out=out, **kw)
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.abbeIntensity(mft, pf, sh, N, out=out, **kw)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    nat.set_profiling(True)
    L.abbeIntensity(mft, pf, sh, N, out=out, **kw)
    torch.cuda.synchronize()
    p = nat.last_profile()
    nat.set_profiling(False)
    print("LEG " + json.dumps({"cfg": cfg, "case": case, "S": int(sh.shape[0]), "ms": times, "lib": nat.LIB_PATH,
                               "x_us_per_item": p["xpass_ms"] / max(1, p["xpass_points"]) * 1e3,
                               "y_us_per_item": p["ypass_ms"] / max(1, p["ypass_points"]) * 1e3,
                               "xpass_kernel": p["xpass_kernel"], "ypass_kernel": p["ypass_kernel"],
                               "coarse": nat.last_plan()["coarse_grid"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--configs", default="cfg3,cfg1,cfg4")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None)
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if not os.path.exists(args.parent_lib):
        sys.exit(f"{args.parent_lib}: no such library (build the parent commit with `make` and pass its liblitho_abbe.so)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for cfg in args.configs.split(","):
        legs = {"a": [], "b": [], "c": []}
        info = {}
        for rnd in range(2):
            for case in "abc":
                env = dict(os.environ)
                env.pop("LITHO_ABBE_LIB", None)
                if case == "a":
                    env["LITHO_ABBE_LIB"] = os.path.abspath(args.parent_lib)
                limit = CONFIGS[cfg][6]
                r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--parent-lib",
                                    args.parent_lib, "--child", cfg, case], env=env, capture_output=True, text=True)
                if r.returncode != 0:
                    say(f"{cfg} case {case} round {rnd}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}")
                    if args.out:
                        open(args.out, "w").write("\n".join(lines) + "\n")
                    sys.exit(r.returncode)
                leg = json.loads([l for l in r.stdout.splitlines() if l.startswith("LEG ")][0][4:])
                legs[case] += leg["ms"]
                print(f"   ({cfg} case {case} round {rnd}: {sum(leg['ms']) / len(leg['ms']):.3f} ms per step)", flush=True)
                info[case] = leg
        S = info["a"]["S"]
        say(f"== {cfg}: {S} source points, {len(legs['a'])} steps per case (two alternating rounds), ms per step")
        mean = {}
        for case, what in (("a", "unweighted, parent library"), ("b", "unweighted, this build"), ("c", "weighted,   this build")):
            t = legs[case]
            mean[case] = sum(t) / len(t)
            sd = (sum((v - mean[case]) ** 2 for v in t) / (len(t) - 1)) ** 0.5
            i = info[case]
            say(f"  ({case}) {what}: mean {mean[case]:10.3f}  min {min(t):10.3f}  max {max(t):10.3f}  step-to-step sd {100 * sd / mean[case]:5.2f} %"
                f"  | x {i['x_us_per_item']:7.3f} y {i['y_us_per_item']:7.3f} us/item | {i['xpass_kernel']} + {i['ypass_kernel']}"
                f"{' (coarse grid)' if i['coarse'] else ''}")
        say(f"  b/a = {mean['b'] / mean['a']:.4f}   c/a = {mean['c'] / mean['a']:.4f}   c/b = {mean['c'] / mean['b']:.4f}")
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
