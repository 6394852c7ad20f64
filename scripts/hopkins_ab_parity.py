"""Bit equality of the Hopkins path (csrc/socs.hip, csrc/socs_grad.hip, socs.py, vector.py, ilt.py) between two checkouts:

    python scripts/hopkins_ab_parity.py ROOT_A ROOT_B [--timeout 300]

Runs the same seeded workload in one fresh child process per root, each under its own `timeout` and with its root first on
sys.path, so the Python of the two trees is compared as well as their libraries (LITHO_ABBE_LIB is dropped from the children's
environment, and a child asserts that its package and its library come from its root and that every output is finite).  Every
output is saved and compared with numpy.array_equal: nothing in this path reorders a sum, so there is no tolerance, and a
differing bit is a bug to explain.  Stops at the first child that fails; exit status 1 on any difference.

Workload (seconds in all): litho_fft2_c2c both ways, batch 3, n = 16 / 32 / 512 / 1024; litho_tcc_apply and
litho_tcc_apply_vector, batch 3, n = 16 / 64; litho_socs_fields and litho_socs_vjp (accumulate 0 and 1) at (pn, N) = (16, 16),
(16, 32), (16, 1024), (64, 256), (1024, 1024); litho_socs_jvp (2 directions), litho_socs_image_batch (3 tiles),
litho_source_sensitivity and litho_pupil_vjp (8 source points in chunks of 3, with and without weights), accumulate 0 and 1, at
(16, 16), (16, 32), (16, 512), (64, 256), (1024, 1024) with 3 x 2 kernels (1 x 2 at 1024), the sensitivities at 2048 as well;
litho_pupil_project (pn 64, 2 planes, 17 terms); socsKernels (bitmap, grey map, two-plane stack) and vectorSocsKernels (TE, the
same three, and applyBytes = 1) at pn 64 with 8 kernels; hopkinsIntensity (kernelChunk None / 3, with and without out),
vectorAbbeIntensity("unpolarized") and hopkinsGradient (kernelChunk 3)."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np


def child(root, path):
    sys.path.insert(0, root)
    import torch
    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat
    from lithographysimulator_amd import socs as S
    from lithographysimulator_amd.synthetic import bernoulli_mask
    package = os.path.join(os.path.abspath(root), "lithographysimulator_amd")
    assert os.path.dirname(os.path.abspath(L.__file__)) == package, L.__file__
    assert os.path.abspath(nat.LIB_PATH) == os.path.join(package, "lib", "liblitho_abbe.so"), nat.LIB_PATH
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(20250)
    lib, st = nat.lib(), nat.stream_ptr(dev)
    res = {}

    def cplx(*shape):
        return torch.view_as_complex(torch.randn(shape + (2,), generator=gen, dtype=torch.float32)).to(dev).contiguous()

    def real(*shape):
        return torch.rand(shape, generator=gen, dtype=torch.float32).to(dev).contiguous()

    def keep(name, t):
        res[name] = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        assert res[name].size and np.isfinite(res[name]).all(), f"{name}: empty or not finite"          # no vacuous equality

    with torch.cuda.device(dev):
        for n in (16, 32, 512, 1024):                                                # a: the plain 2-D transform
            x = cplx(3, n, n)
            keep(f"fft2/{n}/forward", S._device_fft2(x.clone()))
            keep(f"fft2/{n}/inverse", S._device_fft2(x.clone(), inverse=True))
        for n in (16, 64):                                                           # b: T x, scalar and vector
            x, y = cplx(3, n, n), torch.empty((3, n, n), dtype=torch.complex64, device=dev)
            ph, w = cplx(n, n), real(n, n)
            nat.check(lib.litho_tcc_apply(nat.ptr(ph), nat.ptr(w), nat.ptr(x), nat.ptr(y), 3, n, st), "litho_tcc_apply")
            keep(f"tcc/{n}", y)
            qh, w3 = cplx(6, n, n), real(3, n, n)
            nbytes = int(lib.litho_tcc_apply_vector_work_bytes(3, n))
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            nat.check(lib.litho_tcc_apply_vector(nat.ptr(qh), nat.ptr(w3), nat.ptr(x), nat.ptr(y), 3, n, nat.ptr(work), nbytes, st),
                      "litho_tcc_apply_vector")
            keep(f"tcc_vector/{n}", y)
        for pn, N in ((16, 16), (16, 32), (16, 1024), (64, 256), (1024, 1024)):      # c: fields and their adjoint
            groups, K = (2, 3) if pn <= 64 else (1, 2)
            k, m, G = cplx(groups * K, pn, pn), cplx(pn, pn), real(groups, pn, pn)
            fields = torch.empty_like(k)
            nat.check(lib.litho_socs_fields(nat.ptr(k), nat.ptr(m), groups * K, pn, N, nat.ptr(fields), st), "litho_socs_fields")
            keep(f"fields/{pn}/{N}", fields)
            nbytes = int(lib.litho_socs_vjp_work_bytes(groups, K, pn))
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            start = cplx(pn, pn)
            for acc in (0, 1):
                g = start.clone()
                nat.check(lib.litho_socs_vjp(nat.ptr(k), nat.ptr(m), nat.ptr(G), groups, K, pn, N, nat.ptr(g), acc, nat.ptr(work), nbytes,
                                             st), "litho_socs_vjp")
                keep(f"vjp/{pn}/{N}/accumulate{acc}", g)

        def work_for(sizer, *args):
            nbytes = int(sizer(*args))
            assert nbytes > 0, (sizer.__name__, args)
            return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes

        def ints(*shape, span):
            return torch.randint(-span, span, shape, generator=gen, dtype=torch.int32).to(dev).contiguous()

        # c': the other ends of the row pass.  (16, 16) with 3 groups is 48 group lines under 64-line workgroups.
        for pn, N in ((16, 16), (16, 32), (16, 512), (64, 256), (1024, 1024), (2048, 2048)):
            groups, K = (3, 2) if pn <= 64 else (1, 2)
            points, batch = (8, 3) if pn < 2048 else (2, 1)                          # chunks of 3 + 3 + 2
            planes = groups * K
            k, m, G = cplx(planes, pn, pn), cplx(pn, pn), real(groups, pn, pn)
            shifts, weights = ints(points, 2, span=pn), real(points)
            work, nbytes = work_for(lib.litho_source_sensitivity_work_bytes, groups, K, batch, pn)
            sens = torch.empty(points, dtype=torch.float32, device=dev)
            nat.check(lib.litho_source_sensitivity(nat.ptr(k), nat.ptr(m), nat.ptr(G), groups, K, nat.ptr(shifts), points, pn, N,
                                                   nat.ptr(sens), batch, nat.ptr(work), nbytes, st), "litho_source_sensitivity")
            keep(f"sensitivity/{pn}/{N}", sens)
            if pn == 2048:                                                           # the reducing store alone goes there
                continue
            work, nbytes = work_for(lib.litho_pupil_vjp_work_bytes, groups, K, batch, pn)
            start = cplx(planes, pn, pn)
            for acc in (0, 1):
                for name, w in (("plain", None), ("weighted", nat.ptr(weights))):
                    g = start.clone()
                    nat.check(lib.litho_pupil_vjp(nat.ptr(k), nat.ptr(m), nat.ptr(G), groups, K, nat.ptr(shifts), w, points, pn, N,
                                                  nat.ptr(g), acc, batch, nat.ptr(work), nbytes, st), "litho_pupil_vjp")
                    keep(f"pupil_vjp/{pn}/{N}/{name}/accumulate{acc}", g)
            P, tiles = 2, 3
            dM, masks = cplx(P, pn, pn), cplx(tiles, pn, pn)
            work, nbytes = work_for(lib.litho_socs_jvp_work_bytes, groups, K, P, pn)
            start = real(P, groups, pn, pn)
            for acc in (0, 1):
                dI = start.clone()
                nat.check(lib.litho_socs_jvp(nat.ptr(k), nat.ptr(m), nat.ptr(dM), P, groups, K, pn, N, nat.ptr(dI), acc, nat.ptr(work),
                                             nbytes, st), "litho_socs_jvp")
                keep(f"jvp/{pn}/{N}/accumulate{acc}", dI)
            work, nbytes = work_for(lib.litho_socs_image_batch_work_bytes, tiles, groups, K, pn)
            start = real(tiles, groups, pn, pn)
            for acc in (0, 1):
                out = start.clone()
                nat.check(lib.litho_socs_image_batch(nat.ptr(k), nat.ptr(masks), tiles, groups, K, pn, N, nat.ptr(out), acc, nat.ptr(work),
                                                     nbytes, st), "litho_socs_image_batch")
                keep(f"image_batch/{pn}/{N}/accumulate{acc}", out)
        pn, planes, J = 64, 2, 17                                                    # one term more than a tile of 16
        g, pups, basis = cplx(planes, pn, pn), cplx(planes, pn, pn), real(J, pn, pn)
        work, nbytes = work_for(lib.litho_pupil_project_work_bytes, planes, J, pn)
        coeff = torch.empty(J, dtype=torch.float32, device=dev)
        nat.check(lib.litho_pupil_project(nat.ptr(g), nat.ptr(pups), planes, nat.ptr(basis), J, pn, nat.ptr(coeff), nat.ptr(work), nbytes,
                                          st), "litho_pupil_project")
        keep("pupil_project", coeff)

    pn, WL, NA, PS = 64, 193.0, 0.7, 25                                              # d, e: the factorisations
    mask = L.Mask(bernoulli_mask(pn), PS, dev)
    mft = mask.fraunhofer(WL, True)
    _, N = mask.calculateEpsilonN(mask.deltaK, PS, WL)
    ab = torch.tensor([0, 0, 0.01, 0, 100, 0.01, 0, 0.01, 0.01, 0.01], dtype=torch.float16)
    P = L.Pupil(pn, WL, NA, ab, dev).generatePupilFunction()
    P0 = L.Pupil(pn, WL, NA, torch.zeros(10, dtype=torch.float16), dev).generatePupilFunction()
    bitmap = L.LightSource(0.4, 0.8, pn, NA, device=dev).generateAnnular()
    grey = (bitmap != 0).to(torch.float32).cpu() * (0.25 + torch.rand((pn, pn), generator=gen, dtype=torch.float32))
    sets = {}
    for name, pupil, source in (("bitmap", P, bitmap), ("grey", P, grey), ("stack", torch.stack([P, P0]), bitmap)):
        sets[f"socs/{name}"] = L.socsKernels(pupil, source, kernels=8)
        sets[f"vector/{name}"] = L.vectorSocsKernels(pupil, source, NA, polarization="te", kernels=8)
    sets["vector/bitmap/applyBytes1"] = L.vectorSocsKernels(P, bitmap, NA, polarization="te", kernels=8, applyBytes=1)
    for name, k in sets.items():
        for field in ("kernels", "eigenvalues", "trace", "captured"):
            keep(f"{name}/{field}", getattr(k, field))
        keep(f"{name}/boxes", [list(b) if b is not None else [-1] * 4 for b in k.boxes])

    for name in ("socs/bitmap", "socs/stack", "vector/grey"):                        # f: the images and the gradient
        k = sets[name]
        want = (k.planes, pn, pn) if k.stacked else (pn, pn)
        for chunk in (None, 3):
            keep(f"image/{name}/chunk{chunk}", L.hopkinsIntensity(mft, k, N, kernelChunk=chunk))
            keep(f"image/{name}/chunk{chunk}/out", L.hopkinsIntensity(mft, k, N, out=real(*want), kernelChunk=chunk))
        G = real(*want)
        keep(f"gradient/{name}", L.hopkinsGradient(mft, k, N, G, kernelChunk=3))
        keep(f"gradient/{name}/out", L.hopkinsGradient(mft, k, N, G, out=cplx(pn, pn), kernelChunk=3))
    Q, shifts = L.vectorPupils(torch.stack([P, P0]), NA), L.sourceShifts(bitmap, pn)
    keep("vector_abbe", L.vectorAbbeIntensity(mft, Q, shifts, N, "unpolarized"))
    keep("vector_abbe/out", L.vectorAbbeIntensity(mft, Q, shifts, N, "unpolarized", out=real(2, pn, pn)))
    torch.cuda.synchronize()
    np.savez(path, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("roots", nargs=2)
    ap.add_argument("--timeout", type=int, default=300, help="seconds for each child")
    a = ap.parse_args()
    env = {k: v for k, v in os.environ.items() if k != "LITHO_ABBE_LIB"}
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, root in enumerate(a.roots):
            path = os.path.join(tmp, f"root{i}.npz")
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", root, path]
            rc = subprocess.run(cmd, env=env).returncode
            if rc != 0:
                print(f"hopkins_ab_parity: the child of {root} ended with status {rc}; nothing more is run")
                return rc
            with np.load(path) as z:
                outs.append({k: z[k] for k in z.files})
    A, B = outs
    differ = [k for k in sorted(set(A) | set(B))
              if k not in A or k not in B or A[k].dtype != B[k].dtype or not np.array_equal(A[k], B[k])]
    for k in differ:
        print("DIFFERS ", k)
    values = sum(v.size for v in A.values())
    print(f"hopkins_ab_parity: {len(A)} outputs, {values} values, {len(A) - len(differ)} bit-identical, {len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    sys.exit(main())
