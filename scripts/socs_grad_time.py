"""Times the mask-gradient path on one MI355X, warm, in one process:

    timeout -k 10 600 python scripts/socs_grad_time.py [--repeats 10] [--root CHECKOUT] [--pn16]

hopkinsIntensity, hopkinsGradient and one optimizeMask iteration at 256^2 with K = 32 and at 2048^2 with K = 64 (annular 0.4-0.8
source, ideal pupil, 25 nm pixels at 193 nm).  Before timing, each size is cross-checked: sum_k |hopkinsFields|^2 against
hopkinsIntensity, and Re <g, dM> against the central difference of sum G . hopkinsIntensity along one direction.  The figures go
into LABNOTES.md beside the forward's.

--pn16 times instead the one size the runs above do not reach, the 16-point line (one thread per line, 64 lines per workgroup):
litho_socs_fields and litho_socs_vjp called directly on 8 groups of 2048 kernels of 16^2 at N = 16, 32 and 1024, device events
around 200 calls after 5.  --root times the package and library of another checkout with this script (an A/B against a parent
commit: alternate the two roots in one visit)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv[:-1]:                                            # before the import below, so ahead of argparse
    ROOT = sys.argv[sys.argv.index("--root") + 1]
sys.path.insert(0, ROOT)
import lithographysimulator_amd as L                                     # noqa: E402


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeats * 1e3


def pn16(dev, pn=16, groups=8, K=2048, reps=200):
    from lithographysimulator_amd import _native as nat
    lib, st = nat.lib(), nat.stream_ptr(dev)
    gen = torch.Generator().manual_seed(1)
    k = torch.view_as_complex(torch.randn((groups * K, pn, pn, 2), generator=gen)).to(dev).contiguous()
    m = torch.view_as_complex(torch.randn((pn, pn, 2), generator=gen)).to(dev).contiguous()
    G = torch.rand((groups, pn, pn), generator=gen).to(dev)
    fields, g = torch.empty_like(k), torch.empty((pn, pn), dtype=torch.complex64, device=dev)
    nbytes = int(lib.litho_socs_vjp_work_bytes(groups, K, pn))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def events(fn):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    with torch.cuda.device(dev):
        for N in (16, 32, 1024):
            t_f = events(lambda: nat.check(lib.litho_socs_fields(nat.ptr(k), nat.ptr(m), groups * K, pn, N, nat.ptr(fields), st),
                                           "litho_socs_fields"))
            t_v = events(lambda: nat.check(lib.litho_socs_vjp(nat.ptr(k), nat.ptr(m), nat.ptr(G), groups, K, pn, N, nat.ptr(g), 0,
                                                              nat.ptr(work), nbytes, st), "litho_socs_vjp"))
            print(f"pn {pn} N {N} batch {groups * K}: litho_socs_fields {t_f:.4f} ms, litho_socs_vjp {t_v:.4f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--root", default=ROOT, help="the checkout whose package and library are timed (default: this script's)")
    ap.add_argument("--pn16", action="store_true", help="time the 16-point line kernels only")
    a = ap.parse_args()
    if a.root != ROOT:
        ap.error("give the checkout as two arguments: --root DIR")
    dev = torch.device("cuda", 0)
    if a.pn16:
        return pn16(dev)
    wl, na, ps = 193.0, 0.7, 25.0
    for pn, K in ((256, 32), (2048, 64)):
        source = L.LightSource(0.4, 0.8, pn, na, device=dev).generateAnnular()
        pupil = L.Pupil(pn, wl, na, None, dev).generatePupilFunction()
        t0 = time.perf_counter()
        socs = L.socsKernels(pupil, source, kernels=K)
        torch.cuda.synchronize()
        setup = time.perf_counter() - t0
        geo = torch.zeros((pn, pn), dtype=torch.int16)
        for r in range(pn // 8, pn - pn // 8, pn // 8):
            geo[r:r + 6, pn // 8:pn - pn // 8] = 1
        mask = L.Mask(geo, ps, dev)
        eps, N = mask.calculateEpsilonN(mask.deltaK, ps, wl)
        M = mask.fraunhofer(wl, True)
        gen = torch.Generator(device=dev).manual_seed(1)
        G = torch.randn((pn, pn), generator=gen, dtype=torch.float32, device=dev)
        # cross-checks in float64 on the device
        image = L.hopkinsIntensity(M, socs, N)
        chunk = max(1, min(K, (1 << 30) // (pn * pn * 8)))
        mine = torch.zeros((pn, pn), dtype=torch.float64, device=dev)
        for c0 in range(0, K, chunk):
            part = L.SOCSKernels(socs.kernels[c0:c0 + chunk].contiguous(), socs.eigenvalues[c0:c0 + chunk], 1.0, 1.0, 1.0, K, [None])
            E = L.hopkinsFields(M, part, N)
            mine += (E.real.double() ** 2 + E.imag.double() ** 2).sum(dim=0)
            del E
        e_img = float((mine - image.double()).abs().max() / image.double().max())
        g = L.hopkinsGradient(M, socs, N, G)
        dM = torch.view_as_complex(torch.randn((pn, pn, 2), generator=gen, dtype=torch.float32, device=dev))
        h = 1e-2 * float(torch.linalg.norm(M) / torch.linalg.norm(dM))
        up = (G.double() * L.hopkinsIntensity(M + h * dM, socs, N).double()).sum()
        down = (G.double() * L.hopkinsIntensity(M - h * dM, socs, N).double()).sum()
        fd = float(up - down) / (2 * h)
        an = float((g.to(torch.complex128).conj() * dM.to(torch.complex128)).sum().real)
        print(f"pn {pn} N {N} K {socs.K} (captured {socs.captured:.4f}, set-up {setup:.2f} s): sum |fields|^2 vs hopkinsIntensity "
              f"{e_img:.2e} of the maximum; Re<g,dM> {an:.6e} vs central difference {fd:.6e} ({abs(an - fd) / abs(fd):.1e})")
        t_fwd = timed(lambda: L.hopkinsIntensity(M, socs, N), a.repeats)
        t_fld = timed(lambda: L.hopkinsFields(M, part, N), a.repeats) * K / part.K
        t_grad = timed(lambda: L.hopkinsGradient(M, socs, N, G), a.repeats)
        open_image = L.hopkinsImage(mask, L.Mask(torch.ones_like(geo), ps, dev).fraunhofer(wl, True), socs, ps, mask.deltaK, wl, True)
        n_out = open_image.shape[-1]
        threshold = 0.3 * float(open_image[n_out // 2, n_out // 2])
        target = torch.zeros((n_out, n_out), dtype=torch.float32, device=dev)
        k = min(pn, n_out)
        target[:k, :k] = geo[:k, :k].to(dev).float()
        one = timed(lambda: L.optimizeMask(target, socs, ps, mask.deltaK, wl, threshold, iterations=1), max(1, a.repeats // 2))
        five = timed(lambda: L.optimizeMask(target, socs, ps, mask.deltaK, wl, threshold, iterations=5), max(1, a.repeats // 2))
        print(f"pn {pn} N {N} K {socs.K}: hopkinsIntensity {t_fwd:.3f} ms, hopkinsFields {t_fld:.3f} ms (per {K} kernels), "
              f"hopkinsGradient {t_grad:.3f} ms = {t_grad / t_fld:.2f} field passes, {t_grad / t_fwd:.2f} forwards; one optimizeMask "
              f"iteration {(five - one) / 4:.3f} ms")


if __name__ == "__main__":
    main()
