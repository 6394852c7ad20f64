"""Bit equality of the resist chain (csrc/peb.hip, csrc/develop.hip, csrc/develop_grad.hip, develop.py, peb.py, calibrate.py,
tangent.py) between two checkouts:

    python scripts/resist_ab_parity.py ROOT_A ROOT_B [--timeout 300]

Runs the same seeded workload in one fresh child process per root, each under its own `timeout` and with its root first on
sys.path, so the Python of the two trees is compared as well as their libraries (LITHO_ABBE_LIB is dropped from the children's
environment, and a child asserts that its package and its library come from its root).  Every output is saved as its raw bits
(fp32 viewed as uint32 and float64 as uint64, so NaN cells compare) and compared with numpy.array_equal: nothing in these kernels reorders a sum, so
there is no tolerance, and a differing bit is a bug to find.  Stops at the first child that fails; exit status 1 on any
difference.

Workload (seconds in all): the eleven volume entries at the seven shapes (n, D, B) of tests/test_gpu_resist_memory.py -- the
smallest on each side of the 16-byte path, the tile edge and the two 64 KiB LDS thresholds.  Images and acid doses carry a
negative and a NaN cell (the rate law's explicit NaN), slowness volumes the four kinds of wall (NaN, 0, -1, +inf).  The rate law
runs with q integer and not, m_th 0 and > 0; the bake with stepsPerLaunch 0, 2 and 4 wherever the fused kernel's LDS fits
160 KiB, kQuench finite and infinite, and each species not diffusing; the bake adjoint with checkpointEvery 1, the default and
steps; both solvers keep their launch counts.  Every pointwise entry (and the development adjoint, whose link and scale
kernels are packed) runs once more through the raw C ABI with every buffer one float past a 16-byte boundary: the scalar twins.
The entries added since ride on the same shapes and variants: the three parameter gradients (the bake's at checkpointEvery 1, the
default and steps), the four forward-mode entries with P = 1 and P = 3 directions (the bake's with and without dacid_in and with
the primal outputs; the three packed ones once more shifted), and the four host chains, whose float64 outputs compare as raw
64-bit words."""
import argparse
import ctypes
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

SHAPES = [(1, 1, 1), (4, 2, 2), (15, 2, 3), (16, 5, 2), (17, 3, 2), (12, 14, 2), (20, 29, 1)]
THICK, H, BAKE, STEPS = 100.0, 25.0, 60.0, 7
DOSES = (0.6, 1.0, 1.7)
LAWS = [(5.0, 0.4), (5.0, 0.0), (3.7, 0.4), (3.7, 0.0)]                              # (q, m_th)
DIFFUSIONS = {"lateral": (1.2, 0.0), "vertical": (0.0, 0.45), "both": (1.2, 0.45), "neither": (0.0, 0.0)}


def fused_fits(D, s):
    """include/litho_abbe.h: the fused bake kernel's LDS at s steps per launch against a workgroup's 160 KiB."""
    return s <= 1 or D * (4 * (16 + 2 * s) ** 2 + 256) * 4 <= 160 * 1024


def child(root, path):
    sys.path.insert(0, root)
    import torch
    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat
    from lithographysimulator_amd import calibrate as cal
    from lithographysimulator_amd import peb
    from lithographysimulator_amd import tangent as tan
    package = os.path.join(os.path.abspath(root), "lithographysimulator_amd")
    assert os.path.dirname(os.path.abspath(L.__file__)) == package, L.__file__
    assert os.path.abspath(nat.LIB_PATH) == os.path.join(package, "lib", "liblitho_abbe.so"), nat.LIB_PATH
    dev = torch.device("cuda", 0)
    lib, res = nat.lib(), {}

    def keep(name, t):
        a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        assert name not in res and a.size, name                                      # no vacuous equality
        res[name] = a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a

    def put(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

    def shifted(t):
        """A copy of t (or, for a shape, an uninitialised volume) whose first element lies 4 bytes past a 16-byte boundary."""
        shape = tuple(t.shape) if isinstance(t, torch.Tensor) else tuple(t)
        v = torch.full((math.prod(shape) + 1,), float("nan"), dtype=torch.float32, device=dev)[1:].view(shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        if isinstance(t, torch.Tensor):
            v.copy_(t)
        return v

    def mack(q, m_th):
        return L.MackResist(C=0.9, rMax=120.0, rMin=0.05, q=q, mTh=m_th, surfaceRate=0.25, surfaceDepth=30.0)

    def car(D, k_quench=2.0, acid=1.0, quencher=0.4, law=LAWS[0]):
        """The smallest stable step count on the (H, THICK / D) grid is 5 when the acid diffuses."""
        sigma = math.sqrt(4.5 / (2.0 / (H * H) + 0.25 / ((THICK / D) ** 2)))
        return L.ChemicallyAmplifiedResist(C=1.0, quencher=0.3, kAmp=0.05, kQuench=k_quench, kLoss=0.02, acidDiffusionLength=acid * sigma,
                                           quencherDiffusionLength=quencher * sigma, verticalScale=0.5, bakeTime=BAKE, mack=mack(*law))

    g3 = (ctypes.c_float * len(DOSES))(*DOSES)
    with torch.cuda.device(dev):
        st = nat.stream_ptr(dev)
        for n, D, B in SHAPES:
            tag = f"{n}-{D}-{B}"
            rng = np.random.default_rng(1000 * n + 10 * D + B)
            V, dose = rng.uniform(0.0, 3.0, (B, D, n, n)), rng.uniform(0.0, 80.0, (B, D, n, n))
            s = 10.0 ** rng.uniform(-3.0, 0.0, (B, D, n, n))
            if n > 1:
                V[0, 0, 0, 1], V[B - 1, D - 1, n - 1, n - 2] = -0.5, np.nan
                dose[0, 0, 0, 1], dose[B - 1, D - 1, n - 1, n - 2] = -0.5, np.nan
                s[0, 0, 0, 1], s[0, D - 1, n - 1, n - 2], s[B - 1, 0, 1, 0], s[B - 1, D - 1, n // 2, n // 2] = np.nan, 0.0, -1.0, np.inf
            V, dose, s = put(V), put(dose), put(s)
            uniform = lambda *shape, lo=-1.0, hi=1.0: put(rng.uniform(lo, hi, shape))       # noqa: E731
            nd, vol, gained = len(DOSES), (B, D, n, n), (len(DOSES) * B, D, n, n)

            # litho_latent_diffuse
            for name, (cxy, cz) in DIFFUSIONS.items():
                keep(f"{tag}/latent_diffuse/{name}", L.latentDiffusion(V, THICK, H, cxy * H, cz * (THICK / D)))
                sxy, sz = float(cxy * H) / H, float(cz * (THICK / D)) / (THICK / D)
                out, work = shifted(vol), shifted(vol)
                nat.check(lib.litho_latent_diffuse(nat.ptr(shifted(V)), B, D, n, sxy, sz, nat.ptr(out), nat.ptr(work), V.numel() * 4, st),
                          "litho_latent_diffuse")
                keep(f"{tag}/latent_diffuse/{name}/shifted", out)

            # litho_develop_rate, litho_develop_rate_vjp, litho_peb_rate: the rate law forwards and backwards
            gs = uniform(*gained)
            for q, m_th in LAWS:
                r, law = mack(q, m_th), f"q{q}-mth{m_th}"
                args = (r.rMax, r.rMin, r.q, r.mTh, r.surfaceRate, r.surfaceDepth, THICK)
                slow = L.developmentRate(V, r, THICK, H, DOSES)
                keep(f"{tag}/develop_rate/{law}", slow)
                out = shifted(gained)
                nat.check(lib.litho_develop_rate(nat.ptr(shifted(V)), B, D, n, g3, nd, r.C, *args, nat.ptr(out), st), "litho_develop_rate")
                keep(f"{tag}/develop_rate/{law}/shifted", out)
                g = gs.clone()
                g[torch.isnan(slow)] = float("nan")                                   # NaN on the walls
                keep(f"{tag}/develop_rate_vjp/{law}", L.developmentRateGradient(V, r, THICK, H, DOSES, g))
                out = shifted(vol)
                nat.check(lib.litho_develop_rate_vjp(nat.ptr(shifted(V)), B, D, n, g3, nd, r.C, *args, nat.ptr(shifted(g)), nat.ptr(out), st),
                          "litho_develop_rate_vjp")
                keep(f"{tag}/develop_rate_vjp/{law}/shifted", out)
                c = car(D, law=(q, m_th))
                m, slow = peb.amplifiedRate(dose, c, THICK)
                keep(f"{tag}/peb_rate/{law}/inhibitor", m)
                keep(f"{tag}/peb_rate/{law}/slowness", slow)
                keep(f"{tag}/peb_rate_vjp/{law}", peb.amplifiedRateGradient(dose, c, THICK, uniform(*vol)))
                out, out_m = shifted(vol), shifted(vol)
                nat.check(lib.litho_peb_rate(nat.ptr(shifted(dose)), B, D, n, c.kAmp, *args, nat.ptr(out), nat.ptr(out_m), st), "litho_peb_rate")
                keep(f"{tag}/peb_rate/{law}/shifted/slowness", out)
                keep(f"{tag}/peb_rate/{law}/shifted/inhibitor", out_m)
                nat.check(lib.litho_peb_rate(nat.ptr(shifted(dose)), B, D, n, c.kAmp, *args, nat.ptr(out), None, st), "litho_peb_rate")
                keep(f"{tag}/peb_rate/{law}/shifted/slowness only", out)

            # litho_develop_time, litho_developed_depth, litho_develop_time_vjp
            T, launches = L.developmentTime(s, THICK, H, returnLaunches=True)
            keep(f"{tag}/develop_time/T", T)
            keep(f"{tag}/develop_time/launches", [launches])
            t = float(T[torch.isfinite(T)].median())
            keep(f"{tag}/developed_depth", L.developedDepth(T, THICK, t))
            out = shifted((B, n, n))
            nat.check(lib.litho_developed_depth(nat.ptr(shifted(T)), B, D, n, THICK, t, nat.ptr(out), st), "litho_developed_depth")
            keep(f"{tag}/developed_depth/shifted", out)
            gT = uniform(*vol)
            gT[~(torch.isfinite(s) & (s > 0))] = float("nan")
            grad, launches = L.developmentTimeGradient(s, T, gT, THICK, H, returnLaunches=True)
            keep(f"{tag}/develop_time_vjp/grad", grad)
            keep(f"{tag}/develop_time_vjp/launches", [launches])
            nbytes = int(lib.litho_develop_vjp_work_bytes(B, D, n, 1024))
            work, out, count = torch.empty(nbytes, dtype=torch.uint8, device=dev), shifted(vol), ctypes.c_int(-1)
            nat.check(lib.litho_develop_time_vjp(nat.ptr(shifted(s)), nat.ptr(shifted(T)), nat.ptr(shifted(gT)), B, D, n, THICK, H, 1024,
                                                 nat.ptr(out), nat.ptr(work), nbytes, ctypes.byref(count), st), "litho_develop_time_vjp")
            keep(f"{tag}/develop_time_vjp/shifted/grad", out)
            keep(f"{tag}/develop_time_vjp/shifted/launches", [count.value])

            # litho_peb_expose, litho_peb_expose_vjp
            h0 = peb.exposeAcid(V, 0.9, DOSES)
            keep(f"{tag}/peb_expose", h0)
            out = shifted(gained)
            nat.check(lib.litho_peb_expose(nat.ptr(shifted(V)), B, D, n, g3, nd, 0.9, nat.ptr(out), st), "litho_peb_expose")
            keep(f"{tag}/peb_expose/shifted", out)
            ga = uniform(*gained)
            ga[torch.isnan(h0)] = float("nan")
            keep(f"{tag}/peb_expose_vjp", peb.exposeAcidGradient(V, 0.9, DOSES, ga))
            out = shifted(vol)
            nat.check(lib.litho_peb_expose_vjp(nat.ptr(shifted(V)), B, D, n, g3, nd, 0.9, nat.ptr(shifted(ga)), nat.ptr(out), st),
                      "litho_peb_expose_vjp")
            keep(f"{tag}/peb_expose_vjp/shifted", out)

            # litho_peb_bake, litho_peb_bake_vjp
            resists = {"finite": car(D), "instantaneous": car(D, k_quench=float("inf")), "acid still": car(D, acid=0.0),
                       "quencher still": car(D, quencher=0.0)}
            acid = uniform(*vol, lo=0.0, hi=1.0)
            acid_nan = acid.clone()
            if n > 1:
                acid_nan[B - 1, D // 2, n // 2, 1] = float("nan")                     # it spreads; the comparison is of bit patterns
            cot = [uniform(*vol) for _ in range(3)]
            for name, r in resists.items():
                for spl in (0, 2, 4):
                    if fused_fits(D, spl):
                        for what, v in zip(("acid", "quencher", "acid_dose"), peb.bakeAcid(acid_nan, r, THICK, H, steps=STEPS, stepsPerLaunch=spl)):
                            keep(f"{tag}/peb_bake/{name}/spl{spl}/{what}", v)
                for c in (1, None, STEPS):                                            # the adjoint takes finite volumes
                    gh, gq = peb.bakeGradient(acid, r, THICK, H, cot[0], cot[1], cot[2], steps=STEPS, checkpointEvery=c)
                    keep(f"{tag}/peb_bake_vjp/{name}/checkpoint{c}/grad_acid_in", gh)
                    keep(f"{tag}/peb_bake_vjp/{name}/checkpoint{c}/grad_quencher_in", gq)
            keep(f"{tag}/peb_bake_vjp/dose only/grad_acid_in", peb.bakeGradient(acid, resists["finite"], THICK, H, gradAcidDose=cot[2], steps=STEPS)[0])

            # the parameter gradients: litho_peb_expose_vjp_params, litho_peb_bake_vjp_params, litho_develop_rate_vjp_params and the
            # two host chains litho_peb_param_chain, litho_develop_rate_param_chain
            keep(f"{tag}/peb_expose_vjp_params", cal.exposureParameterGradient(V, 0.9, DOSES, ga))
            for name, r in resists.items():
                for c in (1, None, STEPS):
                    gh, gq, gstep = cal.bakeStepGradient(acid, r, THICK, H, cot[0], cot[1], cot[2], steps=STEPS, checkpointEvery=c)
                    keep(f"{tag}/peb_bake_vjp_params/{name}/checkpoint{c}/grad_acid_in", gh)
                    keep(f"{tag}/peb_bake_vjp_params/{name}/checkpoint{c}/grad_quencher_in", gq)
                    keep(f"{tag}/peb_bake_vjp_params/{name}/checkpoint{c}/grad_step", gstep)
                keep(f"{tag}/peb_param_chain/{name}", cal.bakeParameterChain(gstep, r, THICK, H, D, STEPS))
            for q, m_th in LAWS:
                r, law = mack(q, m_th), f"q{q}-mth{m_th}"
                g = gs.clone()
                g[torch.isnan(L.developmentRate(V, r, THICK, H, DOSES))] = float("nan")
                sums = cal._rate_sums("parity", V, DOSES, r.C, r, THICK, g)
                keep(f"{tag}/develop_rate_vjp_params/{law}", sums)
                keep(f"{tag}/develop_rate_param_chain/{law}", cal.rateParameterChain(sums, r, THICK))

            # forward mode: litho_peb_expose_jvp, litho_peb_bake_jvp, litho_develop_rate_jvp, litho_develop_time_jvp and the two host
            # chains litho_peb_param_tangent, litho_develop_rate_param_tangent; P = 1 and P = 3
            for P in (1, 3):
                dC = rng.uniform(-1.0, 1.0, P)
                dI, dh = uniform(P, *vol), uniform(P, *vol)
                keep(f"{tag}/peb_expose_jvp/P{P}", tan.exposeAcidTangent(V, 0.9, DOSES, dC, dI))
                keep(f"{tag}/peb_expose_jvp/P{P}/no dImage", tan.exposeAcidTangent(V, 0.9, DOSES, dC))
                out, dCc = shifted((P,) + gained), (ctypes.c_double * P)(*dC)
                nat.check(lib.litho_peb_expose_jvp(nat.ptr(shifted(V)), B, D, n, g3, nd, 0.9, P, dCc, nat.ptr(shifted(dI)), nat.ptr(out), st),
                          "litho_peb_expose_jvp")
                keep(f"{tag}/peb_expose_jvp/P{P}/shifted", out)
                dq, dpar = rng.uniform(-1.0, 1.0, P), rng.uniform(-1.0, 1.0, (P, 5))
                for name, r in resists.items():
                    dstep = tan.bakeParameterTangent(dpar, r, THICK, H, D, STEPS)
                    keep(f"{tag}/peb_param_tangent/{name}/P{P}", dstep)
                    outs = tan.bakeTangent(acid_nan, r, THICK, H, dAcid=dh, dQuencher=dq, dStep=dstep, steps=STEPS, returnPrimal=True)
                    for what, v in zip(("dacid", "dquencher", "dacid_dose", "acid", "quencher", "acid_dose"), outs):
                        keep(f"{tag}/peb_bake_jvp/{name}/P{P}/primal/{what}", v)
                    outs = tan.bakeTangent(acid, r, THICK, H, dQuencher=dq, dStep=dstep, steps=STEPS)
                    for what, v in zip(("dacid", "dquencher", "dacid_dose"), outs):
                        keep(f"{tag}/peb_bake_jvp/{name}/P{P}/no dacid_in/{what}", v)
                dpar7 = rng.uniform(-1.0, 1.0, (P, 7))
                for q, m_th in LAWS:
                    r, law = mack(q, m_th), f"q{q}-mth{m_th}"
                    dphi = tan.rateParameterTangent(dpar7, r, THICK, D)
                    keep(f"{tag}/develop_rate_param_tangent/{law}/P{P}", dphi)
                    keep(f"{tag}/develop_rate_jvp/{law}/P{P}", tan.developmentRateTangent(V, r, THICK, DOSES, dX=dI, dPhi=dphi))
                    keep(f"{tag}/develop_rate_jvp/{law}/P{P}/no dX", tan.developmentRateTangent(V, r, THICK, DOSES, dPhi=dphi))
                    out, phi = shifted((P,) + gained), dphi.contiguous().to(dev)
                    nat.check(lib.litho_develop_rate_jvp(nat.ptr(shifted(V)), B, D, n, g3, nd, r.C, r.rMax, r.rMin, r.q, r.mTh, r.surfaceRate,
                                                         r.surfaceDepth, THICK, P, nat.ptr(shifted(dI)), nat.ptr(phi), nat.ptr(out), st),
                              "litho_develop_rate_jvp")
                    keep(f"{tag}/develop_rate_jvp/{law}/P{P}/shifted", out)
                ds = uniform(P, *vol)
                ds[:, ~(torch.isfinite(s) & (s > 0))] = float("nan")                     # ignored on the walls
                dT, launches = tan.developmentTimeTangent(s, T, ds, THICK, H, returnLaunches=True)
                keep(f"{tag}/develop_time_jvp/P{P}/dT", dT)
                keep(f"{tag}/develop_time_jvp/P{P}/launches", [launches])
                nbytes = int(lib.litho_develop_jvp_work_bytes(B, D, n, P, 1024))
                work, out, count = torch.empty(nbytes, dtype=torch.uint8, device=dev), shifted((P,) + vol), ctypes.c_int(-1)
                nat.check(lib.litho_develop_time_jvp(nat.ptr(shifted(s)), nat.ptr(shifted(T)), nat.ptr(shifted(ds)), B, D, n, P, THICK, H, 1024,
                                                     nat.ptr(out), nat.ptr(work), nbytes, ctypes.byref(count), st), "litho_develop_time_jvp")
                keep(f"{tag}/develop_time_jvp/P{P}/shifted/dT", out)
                keep(f"{tag}/develop_time_jvp/P{P}/shifted/launches", [count.value])
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
                print(f"resist_ab_parity: the child of {root} ended with status {rc}; nothing more is run")
                return rc
            with np.load(path) as z:
                outs.append({k: z[k] for k in z.files})
    A, B = outs
    differ = [k for k in sorted(set(A) | set(B))
              if k not in A or k not in B or A[k].dtype != B[k].dtype or not np.array_equal(A[k], B[k])]
    for k in differ:
        print("DIFFERS ", k)
    values = sum(v.size for v in A.values())
    nans = sum(int(np.isnan(v.view(np.float32)).sum()) for v in A.values() if v.dtype == np.uint32)
    print(f"resist_ab_parity: {len(A)} outputs, {values} values ({nans} of them NaN), {len(A) - len(differ)} bit-identical, "
          f"{len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    sys.exit(main())
