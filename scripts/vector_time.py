"""What polarisation costs: set-up time of socsKernels and of vectorSocsKernels, the operator X -> T X of each on the same batch,
and the time of one hopkinsImage through either kernel set, at the benchmark's 2048^2 geometry.

    python scripts/vector_time.py [--pn 2048] [--kernels 64] [--reps 10] [--batch 16] [--operator-only]

2048^2 Bernoulli mask, quasar(4, -pi/8) 0.4-0.8, the 10-term demo pupil, K = 64; the vector setting is TE light at NA 1.35 in water
(index 1.44).  Set-up = one call on the host clock around a device synchronise (it waits for the host-side eigenproblems anyway).
Operator = device events around `reps` back-to-back calls of litho_tcc_apply and of litho_tcc_apply_vector on `batch` vectors:
4 against 14 transforms per vector, so about 3.5 x is expected.  Per image = device events around `reps` hopkinsImage calls after
two warm-up calls; both kernel sets have K kernels and run the same launches.  --operator-only stops after the operator lines (a
short run for `rocprofv3 --kernel-trace --stats`, which gives the share of k_vec_fan_out / k_vec_mix / k_vec_fan_in)."""
import argparse
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEMO_AB = [0, 0, 0.01, 0, 100, 0.01, 0, 0.01, 0.01, 0.01]
WL, NA, PS = 193.0, 0.7, 25
VNA, INDEX = 1.35, 1.44


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
    ap.add_argument("--kernels", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--operator-only", action="store_true")
    args = ap.parse_args()
    import lithographysimulator_amd as L
    from lithographysimulator_amd import socs as S
    from lithographysimulator_amd import vector as V
    from lithographysimulator_amd.synthetic import bernoulli_mask

    dev = torch.device("cuda", 0)
    pn = args.pn
    mask = L.Mask(bernoulli_mask(pn), PS, dev)
    mft = mask.fraunhofer(WL, True)
    bitmap = L.LightSource(0.4, 0.8, pn, NA, device=dev).generateQuasar(4, -math.pi / 8)
    pupil = L.Pupil(pn, WL, NA, torch.tensor(DEMO_AB, dtype=torch.float16), dev).generatePupilFunction()

    # the two operators on the same vectors
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.view_as_complex(torch.randn((args.batch, pn, pn, 2), generator=g, dtype=torch.float32, device=dev))
    W = S._weight_map(bitmap, pn)
    scalar_op = S._DeviceOperator(pupil.to(torch.complex64), torch.fft.ifftshift(W).to(torch.float32).to(dev).contiguous())
    pol = L.sourcePolarization(bitmap, "te")
    vector_op = V._VectorOperator(L.vectorPupils(pupil, VNA, INDEX), torch.fft.ifftshift(pol, dim=(-2, -1)).to(dev).contiguous(),
                                  8 << 30)
    for op in (scalar_op, vector_op):
        op(X)
    torch.cuda.synchronize()
    s_ms, v_ms = per_call_ms(lambda: scalar_op(X), args.reps), per_call_ms(lambda: vector_op(X), args.reps)
    print(f"operator, {pn}^2, {args.batch} vectors: scalar {s_ms / args.batch:.3f} ms / vector, vector {v_ms / args.batch:.3f} ms / vector, "
          f"ratio {v_ms / s_ms:.2f} (14 / 4 transforms = 3.5)", flush=True)
    if args.operator_only:
        return
    del X
    torch.cuda.empty_cache()

    print("| kernels | K | captured | set-up s | hopkinsImage ms |")
    print("|---|---|---|---|---|")
    for name in ("scalar", "vector TE, NA 1.35 / 1.44"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "scalar":
            socs = L.socsKernels(pupil, bitmap, kernels=args.kernels)
        else:
            socs = L.vectorSocsKernels(pupil, bitmap, VNA, polarization="te", mediumIndex=INDEX, kernels=args.kernels)
        torch.cuda.synchronize()
        setup = time.perf_counter() - t0
        for _ in range(2):
            L.hopkinsImage(mask, mft, socs, PS, mask.deltaK, WL)
        torch.cuda.synchronize()
        ms = per_call_ms(lambda: L.hopkinsImage(mask, mft, socs, PS, mask.deltaK, WL), args.reps)
        print(f"| {name} | {socs.K} | {socs.captured:.4f} | {setup:.2f} | {ms:.3f} |", flush=True)
        del socs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
