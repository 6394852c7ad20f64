"""Pupil gradients on the GPU: litho_pupil_vjp and litho_pupil_project (csrc/socs_grad.hip), pupilGradient, wavefrontGradient,
zernikeBasis, aberrationGradient and fitAberrations, against the float64 definitions of tests/pupil_grad_oracle.py and against the
weighted Abbe sum the project already pins.

Regimes of the row kernel k_centred_rows (rolled load with the stored field, then the adjoint with the plane's G) and the case that
reaches each (PG.ORACLE_CASES, held against the oracle; the sizes above 1024 against the engine):
  * lines per workgroup (plane_fft.hpp, LineShape): pn 16, the one-thread line, 64 lines per workgroup; pn 32 ... 512, 64 / T lines per
    workgroup; pn 1024, one workgroup of one wave per line; pn 2048 and 4096, a line of 2 and 4 waves (the engine tie below);
  * transforms per line: m = N / pn = 1 -- (16,16), (64,64), (256,256), (1024,1024); 1 < m <= pn -- (16,64), (32,64), (64,128),
    (128,256); m > pn -- (16,512);
  * planes and K: the G of plane (item mod groups K) / K -- (16,16,2,1), (32,64,3,1), (64,128,2,3), (256,256,3,1).

Bounds: PG.TOL_PGRAD_* and PG.TOL_PROJECT_* (the project's image tolerances: the complex64 floors of the formulas are under a
quarter of them); the loop by four times its own complex64 floor (PG.TOL_FIT_*).  Every test prints what it observed (-s)."""
import ctypes
import math

import pytest
import torch

import pupil_grad_oracle as PG
import socs_grad_oracle as GO
from helpers import NA, PS, TOL_IMAGE_MAX, WL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat
    assert nat.lib().litho_target_arch() == b"gfx950"
    return L


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    return _native


def _on(dev, *tensors):
    return [t.to(dev) for t in tensors]


def _bits(a, b):
    return torch.equal(torch.view_as_real(a), torch.view_as_real(b))


# ---- 1: against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("pn,N,groups,K,points", PG.ORACLE_CASES)
def test_gradient_against_the_oracle(L, dev, pn, N, groups, K, points, weighted):
    P, M, G, sh, w = PG.case(pn, N, groups, K, points)
    listed = sh.tolist()
    if points == 8:
        assert [0, 0] in listed and any(abs(a) > pn or abs(b) > pn for a, b in listed) and len({tuple(s) for s in listed}) < points
        assert any(a < 0 for a, _ in listed) and [pn // 2, -pn // 2] in listed
    assert float(w[1]) == 0.0 and float(w.max()) > 0.25
    want = PG.reference((pn, N, groups, K, points), weighted)
    Pd, Md, Gd, shd, wd = _on(dev, P, M, G, sh, w)
    got = L.pupilGradient(Md, Pd, shd, N, Gd, weights=wd if weighted else None, pupilsPerPlane=K)
    assert got.dtype == torch.complex64 and tuple(got.shape) == tuple(P.shape)
    e_max, e_l2 = GO.rel_max(got, want), GO.rel_l2(got, want)
    print(f"pn {pn} N {N} groups {groups} K {K} weighted {weighted}: max {e_max:.2e} (bound {PG.TOL_PGRAD_MAX:.1e}), l2 {e_l2:.2e} "
          f"({PG.TOL_PGRAD_L2:.1e})")
    assert e_max < PG.TOL_PGRAD_MAX and e_l2 < PG.TOL_PGRAD_L2


# ---- 2: the bits do not depend on how the list is cut --------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,N,groups,K", [(16, 64, 1, 1), (16, 16, 2, 1), (64, 128, 2, 3), (256, 256, 1, 1)])
def test_the_bits_do_not_depend_on_the_call(L, dev, pn, N, groups, K):
    P, M, G, sh, w = _on(dev, *PG.case(pn, N, groups, K, 8))
    count = sh.shape[0]

    def grad(rows, **kw):
        return L.pupilGradient(M, P, sh[rows].contiguous(), N, G, weights=w[rows].contiguous(), pupilsPerPlane=K, **kw)

    every = slice(0, count)
    base = grad(every, batch=count)
    for batch in (1, 3, count, count + 5, None):
        assert _bits(grad(every, batch=batch), base), batch
    assert _bits(grad(every), grad(every)), "two calls"
    # a list split over two calls, the second one adding to the first: the same sequence of additions into every cell.  The heads
    # of 1, 2, 3, 5 and 7 points also leave inactive lines in the last workgroup at pn 16 (64 lines = 4 items of one plane)
    for n in (1, 2, 3, 5, 7):
        head = grad(slice(0, n))
        assert _bits(head, grad(slice(0, n), batch=1)) and bool(torch.isfinite(torch.view_as_real(head)).all()), n
        assert _bits(grad(slice(n, count), out=head), base), n
    # another ORDER of the list is another rounding: within tolerance only
    perm = torch.tensor([5, 0, 7, 2, 6, 1, 4, 3], device=dev)
    other = grad(perm)
    e_max = GO.rel_max(other, base.cpu())
    print(f"pn {pn} N {N} groups {groups} K {K}: permuted list, max {e_max:.2e} of max|g| (bound {PG.TOL_PGRAD_MAX:.1e}), equal bits: "
          f"{_bits(other, base)}")
    assert e_max < PG.TOL_PGRAD_MAX


# ---- 3: against the weighted Abbe sum ----------------------------------------------------------------------------------------------
def _engine_setting(L, dev, pn, points):
    """test_gpu_source_grad._engine_setting, restated."""
    from lithographysimulator_amd.synthetic import bernoulli_mask
    g = torch.Generator().manual_seed(pn)
    pf = L.Pupil(pn, WL, NA, torch.tensor([0, 0, 0, 0, 30], dtype=torch.float16), dev).generatePupilFunction()
    if pn <= 2048:
        mask = L.Mask(bernoulli_mask(pn), PS, dev)
        mft = mask.fraunhofer(WL, True)
        _, N = mask.calculateEpsilonN(mask.deltaK, PS, WL)
    else:
        # beyond the mask spectrum's own sizes at this pixel: any spectrum ties the two paths; N = pn
        mft = torch.view_as_complex(torch.randn((pn, pn, 2), generator=g, dtype=torch.float32)).to(dev)
        N = pn
    sh = L.sourceShifts(L.LightSource(0.4, 0.8, pn, NA, device=dev).generateAnnular(), pn)
    sel = sh[(torch.arange(points, device=dev) * sh.shape[0]) // points].contiguous()
    w = (0.25 + torch.rand(points, generator=g, dtype=torch.float32)).to(dev)
    G = torch.randn((pn, pn), generator=g, dtype=torch.float32).to(dev)
    return mft, pf, sel, int(N), w, G


@pytest.mark.parametrize("pn,points", [(64, 40), (256, 64), (2048, 4), (4096, 2)])
def test_gradient_against_the_weighted_abbe_sum(L, dev, nat, pn, points):
    """Re <g, P> = 2 <G, abbeIntensity(weights=w)>: the image is a Hermitian quadratic form in the pupil, with the engine's default
    plan.  No oracle here: 2048^2 and 4096^2 are the lines of two and four waves."""
    mft, pf, sel, N, w, G = _engine_setting(L, dev, pn, points)
    I = L.abbeIntensity(mft, pf, sel, N, weights=w)
    plan = nat.last_plan()
    g = L.pupilGradient(mft, pf, sel, N, G, weights=w)
    lhs = float((g.real.double() * pf.real.double() + g.imag.double() * pf.imag.double()).sum())
    rhs = 2.0 * float((G.double() * I.double()).sum())
    bound = (2.0 * TOL_IMAGE_MAX * float(I.max()) * float(G.double().abs().sum())
             + PG.TOL_PGRAD_MAX * float(g.abs().max()) * float(pf.abs().double().sum()))
    print(f"pn {pn} N {N} {points} points (coarse grid {plan['coarse_grid']}): Re<g, P> {lhs:.6e}, 2<G, I_w> {rhs:.6e}, difference "
          f"{abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert math.isfinite(lhs) and abs(lhs - rhs) <= bound


# ---- 4: nothing else is written --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,N,groups,K,batch", [(16, 64, 2, 3, 3), (64, 64, 1, 1, 8), (1024, 1024, 1, 1, 1)])
def test_inputs_and_canaries_are_intact(L, dev, nat, pn, N, groups, K, batch):
    points = 8 if pn < 1024 else 2
    P, M, G, sh, w = _on(dev, *PG.case(pn, N, groups, K, points))
    lib = nat.lib()
    nbytes = int(lib.litho_pupil_vjp_work_bytes(groups, K, batch, pn))
    assert nbytes == batch * groups * K * pn * pn * 8
    pad = 64                                                                   # canary words of 4 bytes on either side
    canary = 0x5A5AA5A5
    nwords = groups * K * pn * pn * 2
    work = torch.full((nbytes // 4 + 2 * pad,), canary, dtype=torch.int32, device=dev)
    grad = torch.full((nwords + 2 * pad,), canary, dtype=torch.int32, device=dev)
    before = [t.clone() for t in (P, M, G, sh, w)]
    with torch.cuda.device(dev):
        rc = lib.litho_pupil_vjp(nat.ptr(P), nat.ptr(M), nat.ptr(G), groups, K, nat.ptr(sh), nat.ptr(w), points, pn, N,
                                 ctypes.c_void_p(grad.data_ptr() + 4 * pad), 0, batch, ctypes.c_void_p(work.data_ptr() + 4 * pad),
                                 nbytes, nat.stream_ptr(dev))
    assert rc == nat.LITHO_OK
    torch.cuda.synchronize(dev)
    for name, a, b in zip(("pupils", "maskFT", "gradI", "shifts", "weights"), (P, M, G, sh, w), before):
        assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b), name
    for name, t, n in (("work", work, nbytes // 4), ("grad", grad, nwords)):
        assert bool((t[:pad] == canary).all()) and bool((t[pad + n:] == canary).all()), name
    got = torch.view_as_complex(grad[pad:pad + nwords].view(torch.float32).reshape(groups * K, pn, pn, 2))
    assert _bits(got, L.pupilGradient(M, P, sh, N, G, weights=w, pupilsPerPlane=K)), "the raw call and the Python layer"
    # an empty list: zeros when it starts the sum, nothing when it adds to it
    with torch.cuda.device(dev):
        args = (nat.ptr(P), nat.ptr(M), nat.ptr(G), groups, K, nat.ptr(sh), None, 0, pn, N, ctypes.c_void_p(grad.data_ptr() + 4 * pad))
        tail = (batch, ctypes.c_void_p(work.data_ptr() + 4 * pad), nbytes, nat.stream_ptr(dev))
        assert lib.litho_pupil_vjp(*args, 1, *tail) == nat.LITHO_OK
        assert torch.equal(grad[pad:pad + nwords].view(torch.float32), torch.view_as_real(got).reshape(-1))
        assert lib.litho_pupil_vjp(*args, 0, *tail) == nat.LITHO_OK
    assert int(grad[pad:pad + nwords].abs().max()) == 0 and bool((grad[:pad] == canary).all()) and bool((grad[pad + nwords:] == canary).all())


# ---- 5: the projection -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,J,planes", PG.PROJECT_CASES)
def test_projection_against_the_oracle(L, dev, pn, J, planes):
    g, P, basis, want = PG.project_case(pn, J, planes)
    gd, Pd, bd = _on(dev, g, P, basis)
    if planes == 1:
        gd, Pd = gd[0], Pd[0]
    got = L.aberrationGradient(gd, Pd, bd)
    assert got.dtype == torch.float32 and tuple(got.shape) == (J,)
    e_max, e_l2 = GO.rel_max(got, want), GO.rel_l2(got, want)
    assert torch.equal(L.aberrationGradient(gd, Pd, bd), got), "two calls"
    dW = L.wavefrontGradient(gd, Pd)
    assert dW.dtype == torch.float32 and tuple(dW.shape) == tuple(Pd.shape)
    e_w = GO.rel_max(dW, PG.wavefront_gradient(g.to(torch.complex128), P.to(torch.complex128)).reshape(dW.shape))
    by_map = (dW.double().reshape(planes, 1, pn, pn) * bd.double()[None]).sum(dim=(0, 2, 3)).cpu()
    e_map = GO.rel_max(by_map, want)
    print(f"pn {pn} J {J} planes {planes}: max {e_max:.2e} (bound {PG.TOL_PROJECT_MAX:.1e}), l2 {e_l2:.2e} ({PG.TOL_PROJECT_L2:.1e}); "
          f"wavefrontGradient {e_w:.2e}, its float64 pairing with the basis {e_map:.2e}")
    assert e_max < PG.TOL_PROJECT_MAX and e_l2 < PG.TOL_PROJECT_L2
    assert e_w < PG.TOL_PROJECT_MAX and e_map < PG.TOL_PROJECT_MAX


def test_zernike_basis_is_the_pupils_own_terms(L, dev):
    pn, indices = 64, (0, 4, 7, 8, 12, 65)
    got = L.zernikeBasis(indices, pn, dev)
    want = PG.zernike_basis(indices, pn)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(indices), pn, pn)
    d = (got.cpu() - want).abs()
    print(f"zernikeBasis {indices} at pn {pn}: {int((d != 0).sum())} cells differ from the oracle, max {float(d.max()):.2e}")
    # fp16 values: one unit in the last place of the largest term (|Z| < 16: 2^-7) where the device's pow or trig rounds otherwise
    assert float(d.max()) <= 2.0 ** -7 and float(got[:, 0, 0].abs().max()) == 0.0


# ---- 6: the Python layer ---------------------------------------------------------------------------------------------------------
def test_python_layer_errors(L, dev):
    from lithographysimulator_amd.imageformation import ShapeError
    z = torch.zeros((48, 48), dtype=torch.complex64, device=dev)
    sh = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="pupilGradient.*power of two"):
        L.pupilGradient(z, z, sh, 64, z.real)
    P, M, G, s8, w = _on(dev, *PG.case(32, 64))
    with pytest.raises(ValueError, match="pupilGradient.*power of two"):
        L.pupilGradient(M, P, s8, 96, G)
    with pytest.raises(RuntimeError, match="smaller than the mask"):
        L.pupilGradient(M, P, s8, 16, G)
    with pytest.raises(ShapeError, match="pupilGradient"):
        L.pupilGradient(M, P[0, :16], s8, 64, G)
    with pytest.raises(ShapeError, match="pupilGradient"):
        L.pupilGradient(M, P, s8.reshape(4, 4), 64, G)
    with pytest.raises(ShapeError, match="pupilGradient"):
        L.pupilGradient(M, P, s8, 64, G[0, :16])
    with pytest.raises(ShapeError, match="pupilGradient"):
        L.pupilGradient(M, torch.cat([P, P]), s8, 64, G, pupilsPerPlane=3)
    with pytest.raises(ShapeError, match="weights"):
        L.pupilGradient(M, P, s8, 64, G, weights=w[:3])
    with pytest.raises(ShapeError, match="out"):
        L.pupilGradient(M, P, s8, 64, G, out=torch.zeros((32, 32), dtype=torch.complex64, device=dev))
    with pytest.raises(ValueError, match="batch"):
        L.pupilGradient(M, P, s8, 64, G, batch=0)
    empty = L.pupilGradient(M, P, s8[:0], 64, G)
    assert tuple(empty.shape) == tuple(P.shape) and float(empty.abs().max()) == 0.0
    with pytest.raises(ShapeError, match="aberrationGradient"):
        L.aberrationGradient(P, P[:, :16], torch.zeros((2, 32, 32), device=dev))
    with pytest.raises(ShapeError, match="aberrationGradient"):
        L.aberrationGradient(P, P, torch.zeros((2, 16, 16), device=dev))
    with pytest.raises(ValueError, match="zernikeBasis"):
        L.zernikeBasis((), 32, dev)
    measured = torch.zeros((40, 40), device=dev)
    with pytest.raises(ValueError, match="together"):
        L.fitAberrations(measured, M.real, M.real, torch.zeros((2, 32, 32), device=dev), PS, 4 / 32, WL, imager=lambda c: measured)
    with pytest.raises(ValueError, match="together"):
        L.fitAberrations(measured, M.real, M.real, torch.zeros((2, 32, 32), device=dev), PS, 4 / 32, WL, gradient=lambda c, g: c)
    with pytest.raises(ShapeError, match="transmission"):
        L.fitAberrations(measured, M.real[:16], M.real, torch.zeros((2, 32, 32), device=dev), PS, 4 / 32, WL)
    with pytest.raises(ValueError, match="measured must be"):
        L.fitAberrations(torch.zeros((7, 7), device=dev), M.real, M.real, torch.zeros((2, 32, 32), device=dev), PS, 4 / 32, WL)


# ---- 7: the device model of fitAberrations against the CPU chain ---------------------------------------------------------------------
@pytest.mark.parametrize("pn,planes,normalize", PG.FIT_LOOP_CASES)
def test_one_iteration_of_the_device_loop_against_the_cpu_chain(L, dev, pn, planes, normalize):
    c = PG.fit_case(pn, planes, normalize)
    ref, got = c.reference(), c.loop(dev=dev)
    e_loss = max(abs(a - b) / b for a, b in zip(got.losses, ref.losses))
    e_update = float((PG.update_of(c, got) - PG.update_of(c, ref)).abs().max())
    print(f"pn {pn} planes {planes} normalize {normalize}: losses {got.losses} (oracle {ref.losses}), relative {e_loss:.2e} (bound "
          f"{PG.TOL_FIT_LOSS:.1e}); update {e_update:.2e} (bound {PG.TOL_FIT_UPDATE:.1e})")
    assert len(got.losses) == 2 and e_loss < PG.TOL_FIT_LOSS and e_update < PG.TOL_FIT_UPDATE


# ---- 8: end to end -----------------------------------------------------------------------------------------------------------------
def test_fit_aberrations_end_to_end(L, dev):
    """PG.end_to_end_case through the public calls only: an annular source thinned to about 40 points, three defocus planes, coma
    and spherical; `measured` is the device model at the truth, the start is zero.  That the coefficient error shrinks holds on
    the float64 chain (test_pupil_grad_cpu.py::test_end_to_end_retrieval_on_the_oracle_model), so it is asserted here."""
    c = PG.end_to_end_case()
    pn = c.pn
    bitmap = L.LightSource(0.4, 0.8, pn, NA, device=dev).generateAnnular()
    source = c.source.to(dev)
    assert bool(((source != 0) <= (bitmap != 0)).all()) and 30 <= int((source != 0).sum()) <= 40
    basis = L.zernikeBasis((8, 12), pn, dev)
    base = torch.tensor([-0.15, 0.0, 0.15], device=dev)[:, None, None] * L.zernikeBasis((4,), pn, dev)
    t = c.t.to(dev)
    mask = L.Mask(transmission=t, pixelSize=c.ps, device=dev)
    eps, N = mask.calculateEpsilonN(mask.deltaK, c.ps, 193.0)
    M = mask.fraunhofer(193.0, True)
    sh, w = L.sourceShifts(source != 0, pn), source[source != 0].contiguous()

    def image_of(coefficients):
        W = base + torch.tensordot(coefficients.to(dev), basis, dims=1)
        P = torch.stack([L.generatePhi(Wp, pn, dev) for Wp in W])
        return L.postProcess(L.abbeIntensity(M, P, sh, N, weights=w) / float(w.double().sum()), eps)

    truth = c.truth.to(dev)
    measured = image_of(truth)
    res = L.fitAberrations(measured, t, source, basis, c.ps, 4 / pn, 193.0, baseWavefront=base, iterations=12, step=0.02)
    err0, err = float(truth.abs().max()), float((res.coefficients - truth).abs().max())
    print(f"pn {pn}, {sh.shape[0]} points, 3 planes: losses {['%.3e' % v for v in res.losses]}, best {res.best}, steps {res.steps}\n"
          f"coefficients {res.coefficients.tolist()} (truth {truth.tolist()}), error {err:.2e} from {err0:.2e}")
    assert len(res.losses) == 13 and len(res.steps) == 13 and res.losses[res.best] == min(res.losses)
    assert res.losses[res.best] < res.losses[0] and all(math.isfinite(v) for v in res.losses)
    assert res.coefficients.dtype == torch.float32 and tuple(res.coefficients.shape) == (2,) and bool(torch.isfinite(res.coefficients).all())
    # the returned coefficients give the recorded best loss through the public calls (the same kernels on the same inputs; 1e-4
    # covers a plan chosen differently without the loop's PlanCache: an image difference of 3e-7 of its peak against a residual
    # that the oracle loop leaves at 5e-4 of it)
    d = image_of(res.coefficients) - measured
    loss = float((d * d).mean())
    assert abs(loss - res.losses[res.best]) <= 1e-4 * res.losses[res.best], (loss, res.losses[res.best])
    assert err < err0
