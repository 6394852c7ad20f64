"""Times forward-mode Hopkins imaging on one MI355X, warm, in one process:

    timeout -k 10 600 python scripts/socs_tangent_time.py [--repeats 5] [--pn 2048] [--kernels 64]

hopkinsTangent at 2048^2 with K = 64 for P = 1, 4 and 16 directions, beside hopkinsIntensity and hopkinsGradient of the same run
(annular 0.4-0.8 source, ideal pupil, 25 nm pixels at 193 nm).  Before timing, the tangent is cross-checked against the central
difference of hopkinsIntensity along its first direction (the image is quadratic, so the difference is exact up to rounding).

Bytes: what litho_socs_jvp's launches move through global memory, counted from the shapes -- per kernel and cell (8-byte complex)
the fields cost 48 bytes once per call (row pass 8 + 8, transpose 8 + 8, row pass 8 + 8) and every direction 48 more (row pass
8 + 8, transpose 8 + 8, the folding pass reads the direction's line and the field's, 8 + 8); per direction and cell 20 bytes on top
(the direction plane, the real sums and their transpose).  The share of peak is those bytes over the measured time against
4.1 TB/s.  First measurements of an untuned path; the figures go into LABNOTES.md."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lithographysimulator_amd as L                                     # noqa: E402
from lithographysimulator_amd import socs as _socs                       # noqa: E402

PEAK = 4.1e12


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeats * 1e3


def jvp_bytes(pn, K, P, chunk):
    """Bytes of hopkinsTangent's launches: the fields once per native call (kernel chunk x direction chunk of 16)."""
    cells = pn * pn
    calls = -(-P // 16)
    return K * cells * 48 * (calls + P) + P * cells * 20 * -(-K // chunk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pn", type=int, default=2048)
    ap.add_argument("--kernels", type=int, default=64)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    wl, na, ps, pn, K = 193.0, 0.7, 25.0, a.pn, a.kernels
    source = L.LightSource(0.4, 0.8, pn, na, device=dev).generateAnnular()
    pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
    socs = L.socsKernels(pupil, source, kernels=K)
    geo = torch.zeros((pn, pn), dtype=torch.int16)
    for r in range(pn // 8, pn - pn // 8, pn // 8):
        geo[r:r + 6, pn // 8:pn - pn // 8] = 1
    mask = L.Mask(geo, ps, dev)
    eps, N = mask.calculateEpsilonN(mask.deltaK, ps, wl)
    M = mask.fraunhofer(wl, True)
    gen = torch.Generator(device=dev).manual_seed(1)
    G = torch.randn((pn, pn), generator=gen, dtype=torch.float32, device=dev)
    dM = torch.view_as_complex(torch.randn((16, pn, pn, 2), generator=gen, dtype=torch.float32, device=dev))
    dM *= 0.1 * float(torch.linalg.norm(M) / torch.linalg.norm(dM[0]))
    tan = L.hopkinsTangent(M, socs, N, dM[:1])[0].double()
    fd = (L.hopkinsIntensity(M + dM[0], socs, N).double() - L.hopkinsIntensity(M - dM[0], socs, N).double()) / 2
    scale = float(L.hopkinsIntensity(M, socs, N).max())
    print(f"pn {pn} N {N} K {socs.K} (captured {socs.captured:.4f}): tangent vs central difference of hopkinsIntensity "
          f"{float((tan - fd).abs().max()) / scale:.2e} of the image's maximum", flush=True)
    chunk = _socs._kernel_chunk("hopkinsTangent", None, socs, 16)
    t_fwd = timed(lambda: L.hopkinsIntensity(M, socs, N), a.repeats)
    t_grad = timed(lambda: L.hopkinsGradient(M, socs, N, G), a.repeats)
    print(f"hopkinsIntensity {t_fwd:.3f} ms, hopkinsGradient {t_grad:.3f} ms ({t_grad / t_fwd:.2f} forwards); kernel chunk of the "
          f"tangent {chunk}", flush=True)
    for P in (1, 4, 16):
        t = timed(lambda: L.hopkinsTangent(M, socs, N, dM[:P]), max(1, a.repeats // (1 if P < 16 else 2)))
        nbytes = jvp_bytes(pn, socs.K, P, chunk)
        print(f"hopkinsTangent P {P:2d}: {t:.3f} ms = {t / P:.3f} ms per direction = {t / P / t_fwd:.2f} forwards per direction "
              f"({t / t_fwd:.2f} in all); {nbytes / 1e9:.2f} GB moved, {nbytes / (t * 1e-3) / 1e12:.2f} TB/s = "
              f"{100 * nbytes / (t * 1e-3) / PEAK:.0f} % of 4.1 TB/s", flush=True)


if __name__ == "__main__":
    main()
