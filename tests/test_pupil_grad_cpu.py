"""Pupil gradients without a GPU: the oracle against torch.autograd on the complex128 chain, dl/dc against central differences,
the Euler identity of a quadratic form, the fp32 floors the device bounds are derived from, fitAberrations' update and
backtracking on CPU hooks, the retrieval of the end-to-end case on the oracle model, and the C ABI's argument checks (made before
any launch, so the codes come back without a device)."""
import math

import pytest
import torch

import pupil_grad_oracle as PG
import socs_grad_oracle as GO
from helpers import TOL_IMAGE_L2, TOL_IMAGE_MAX
from oracle import abbe_oracle as O


def _within(measured, recorded):
    """As in test_socs_grad_cpu.py: the recorded floor is what one machine printed when the bound was chosen; another host BLAS
    sums in another order, so the re-check allows a factor 2 and still catches a floor that has really moved."""
    return measured <= 2.0 * recorded


@pytest.mark.parametrize("key", [(16, 16, 1, 1, 8), (16, 64, 2, 1, 8), (32, 64, 1, 3, 8), (64, 128, 2, 3, 8)])
@pytest.mark.parametrize("weighted", [False, True])
def test_oracle_against_autograd(key, weighted):
    """g from the formula against torch.autograd through the complex128 chain written with torch operations only: the loss is
    <G, I>, whose dl/dI is G, and torch's gradient of a complex leaf is dl/dRe + i dl/dIm."""
    pn, N, groups, K, _ = key
    P, M, G, sh, w = PG.case(*key)
    w = w if weighted else None
    leaf = P.to(torch.complex128).requires_grad_(True)
    F = O.centred_dft_matrix(pn, N)
    loss = torch.zeros((), dtype=torch.float64)
    for i, (dy, dx) in enumerate(sh.tolist()):
        E = F @ (torch.roll(leaf, shifts=(dy, dx), dims=(-2, -1)) * M.to(torch.complex128)) @ F.T
        I = (E.real ** 2 + E.imag ** 2).reshape(groups, K, pn, pn).sum(dim=1)
        loss = loss + (1.0 if w is None else float(w[i])) * (G.double() * I).sum()
    loss.backward()
    g = PG.gradient(P, M, sh, N, G, weights=w, K=K)
    err = float((g - leaf.grad).abs().max() / leaf.grad.abs().max())
    print(f"{key} weighted {weighted}: max |g - autograd| / max |g| = {err:.2e}")
    assert tuple(g.shape) == tuple(P.shape) and err <= 1e-12
    if weighted:
        assert float(w[1]) == 0.0 and float(w.min()) == 0.0


def test_euler_identity():
    """I is a Hermitian quadratic form in P, so Re <g, P> = 2 <G, I> for K = groups = 1, to float64 round-off."""
    for pn, N in ((16, 16), (16, 64), (32, 64), (64, 64)):
        P, M, G, sh, w = PG.case(pn, N)
        g = PG.gradient(P, M, sh, N, G, weights=w)
        I = PG.intensity(P, M, sh, N, weights=w)
        lhs, rhs = GO.inner(g, P), 2.0 * float((G.double() * I).sum())
        scale = 2.0 * float((G.double().abs() * I).sum())
        print(f"pn {pn} N {N}: |Re<g, P> - 2<G, I>| / 2 sum |G| I = {abs(lhs - rhs) / scale:.2e}")
        assert abs(lhs - rhs) <= 1e-12 * scale


@pytest.mark.parametrize("pn,planes,normalize", [(32, 1, True), (32, 1, False), (32, 2, True), (32, 2, False)])
def test_coefficient_gradient_against_central_differences(pn, planes, normalize):
    """dl/dc of the loop's model (gradient, wavefront gradient and projection chained) against central differences of its own
    float64 loss, along every coefficient and along a random direction; the points include a wrapping shift."""
    c = PG.fit_case(pn, planes, normalize)
    assert any(abs(dy) + pn // 4 >= pn // 2 for dy, _ in c.shifts.tolist())
    imager, grad = c.model()
    measured = c.measured.double()

    def loss_of(v):
        d = imager(v) - measured
        return float((d * d).mean())

    c0 = c.c0.double()
    diff = imager(c0) - measured
    g = grad(c0, 2.0 * diff / diff.numel())
    gen = torch.Generator().manual_seed(6)
    dirs = list(torch.eye(c0.numel(), dtype=torch.float64)) + [torch.randn(c0.numel(), generator=gen, dtype=torch.float64)]
    h = 1e-5
    for d in dirs:
        fd = (loss_of(c0 + h * d) - loss_of(c0 - h * d)) / (2 * h)
        an = float((g * d).sum())
        print(f"pn {pn} planes {planes} normalize {normalize}: fd {fd:.8e}  analytic {an:.8e}")
        # truncation h^2 |l'''| / 6 with derivatives of order (2 pi)^k l, and rounding eps64 l / h: both under 1e-6 of the gradient
        assert abs(fd - an) <= 1e-6 * float(g.abs().max())


def test_fp32_floor_of_the_gradient_formula():
    """The fp32 floor the device bound is derived from (pupil_grad_oracle.py, "Tolerance"): the same formula in torch's CPU
    complex64 against float64 on exactly the GPU tests' cases, with and without weights."""
    worst_max = worst_l2 = 0.0
    for key in PG.ORACLE_CASES:
        P, M, G, sh, w = PG.case(*key)
        for weighted in (False, True):
            ww = w if weighted else None
            g64 = PG.reference(key, weighted)
            g32 = PG.gradient(P, M, sh, key[1], G, weights=ww, K=key[3], dtype=torch.complex64).to(torch.complex128)
            d = (g32 - g64).abs()
            e_max, e_l2 = float(d.max() / g64.abs().max()), float(torch.linalg.norm(g32 - g64) / torch.linalg.norm(g64))
            print(f"{key} weighted {weighted}: max {e_max:.2e}  l2 {e_l2:.2e}")
            worst_max, worst_l2 = max(worst_max, e_max), max(worst_l2, e_l2)
    print(f"complex64 formula vs float64: max {worst_max:.2e} (recorded {PG.FP32_FLOOR_MAX:.1e}), l2 {worst_l2:.2e} (recorded "
          f"{PG.FP32_FLOOR_L2:.1e})")
    assert _within(worst_max, PG.FP32_FLOOR_MAX) and _within(worst_l2, PG.FP32_FLOOR_L2)
    assert worst_max < TOL_IMAGE_MAX / 4 and worst_l2 < TOL_IMAGE_L2 / 4
    # the rule: the image tolerances where the floor is under a quarter of them, four times the floor otherwise
    assert PG.TOL_PGRAD_MAX == (TOL_IMAGE_MAX if PG.FP32_FLOOR_MAX < TOL_IMAGE_MAX / 4 else 4 * PG.FP32_FLOOR_MAX)
    assert PG.TOL_PGRAD_L2 == (TOL_IMAGE_L2 if PG.FP32_FLOOR_L2 < TOL_IMAGE_L2 / 4 else 4 * PG.FP32_FLOOR_L2)


def test_fp32_floor_of_the_projection():
    worst_max = worst_l2 = 0.0
    for key in PG.PROJECT_CASES:
        g, P, basis, want = PG.project_case(*key)
        got = PG.coefficient_gradient(g, P, basis, dtype=torch.complex64).double()
        e_max, e_l2 = float((got - want).abs().max() / want.abs().max()), float(torch.linalg.norm(got - want) / torch.linalg.norm(want))
        print(f"{key}: max {e_max:.2e}  l2 {e_l2:.2e}")
        worst_max, worst_l2 = max(worst_max, e_max), max(worst_l2, e_l2)
        # the wavefront gradient and the projection are one formula
        dW = PG.wavefront_gradient(g.to(torch.complex128), P.to(torch.complex128))
        assert float(((dW[:, None] * basis.double()[None]).sum(dim=(0, 2, 3)) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    print(f"projection floor: max {worst_max:.2e} (recorded {PG.PROJECT_FLOOR_MAX:.1e}), l2 {worst_l2:.2e} (recorded "
          f"{PG.PROJECT_FLOOR_L2:.1e})")
    assert _within(worst_max, PG.PROJECT_FLOOR_MAX) and _within(worst_l2, PG.PROJECT_FLOOR_L2)
    assert PG.TOL_PROJECT_MAX == (TOL_IMAGE_MAX if PG.PROJECT_FLOOR_MAX < TOL_IMAGE_MAX / 4 else 4 * PG.PROJECT_FLOOR_MAX)
    assert PG.TOL_PROJECT_L2 == (TOL_IMAGE_L2 if PG.PROJECT_FLOOR_L2 < TOL_IMAGE_L2 / 4 else 4 * PG.PROJECT_FLOOR_L2)


def test_fp32_floor_of_the_fit_loop():
    """The floor behind TOL_FIT_LOSS / TOL_FIT_UPDATE: the one-iteration loop on the complex64 chain against the float64 chain, on
    the device tests' cases."""
    worst_loss = worst_update = 0.0
    for key in PG.FIT_LOOP_CASES:
        c = PG.fit_case(*key)
        ref, got = c.reference(), c.loop(*c.model(dtype=torch.complex64))
        e_loss = max(abs(a - b) / b for a, b in zip(got.losses, ref.losses))
        e_update = float((PG.update_of(c, got) - PG.update_of(c, ref)).abs().max())
        print(f"{key}: losses {ref.losses}, relative {e_loss:.2e}; update {e_update:.2e}")
        worst_loss, worst_update = max(worst_loss, e_loss), max(worst_update, e_update)
    print(f"loop floor: loss {worst_loss:.2e} (recorded {PG.FIT_FLOOR_LOSS:.1e}), update {worst_update:.2e} (recorded "
          f"{PG.FIT_FLOOR_UPDATE:.1e})")
    assert _within(worst_loss, PG.FIT_FLOOR_LOSS) and _within(worst_update, PG.FIT_FLOOR_UPDATE)
    assert (PG.TOL_FIT_LOSS, PG.TOL_FIT_UPDATE) == (4 * PG.FIT_FLOOR_LOSS, 4 * PG.FIT_FLOOR_UPDATE)


def test_update_best_iterate_and_backtracking():
    import lithographysimulator_amd as L
    c = PG.fit_case(32, 1, True)
    imager, grad = c.model()
    # the first update is c0 - step . grad / max|grad| of the oracle's gradient
    first = c.reference()
    diff = imager(c.c0.double()) - c.measured.double()
    g0 = grad(c.c0.double(), 2.0 * diff / diff.numel())
    assert abs(first.losses[0] - float((diff * diff).mean())) <= 1e-12 * first.losses[0]
    assert float((first.coefficients.double() - (c.c0.double() - PG.FIT_STEP * g0 / g0.abs().max())).abs().max()) <= 1e-7
    assert first.coefficients.dtype == torch.float32 and first.steps == [0.0, PG.FIT_STEP] and first.best == 1

    # a quadratic bowl whose first step overshoots: the loop returns to the best iterate and halves the step until it improves
    # (every number is dyadic, so the comparisons are exact): image = diag(c - centre), measured = 0, loss = |c - centre|^2 / 4
    centre = torch.tensor([0.25, -0.5])
    calls = []

    def bowl(v):
        calls.append(v.clone())
        return torch.diag(v - centre)

    res = L.fitAberrations(torch.zeros((2, 2)), None, None, torch.zeros((2, 4, 4)), 1.0, 1.0, 193.0, initial=torch.tensor([0.375, -0.5]),
                           iterations=4, step=0.5, imager=bowl, gradient=lambda v, g: torch.diag(g))
    # c0 = (0.375, -0.5): distance 0.125; step 0.5 lands at (-0.125, -0.5): distance 0.375, rejected; 0.25 -> (0.125, -0.5):
    # distance 0.125, equal and so not below; 0.125 -> (0.25, -0.5): loss 0, accepted; there the gradient is zero and the iterate stays
    assert res.steps == [0.0, 0.5, 0.25, 0.125, 0.125] and res.best == 3, (res.steps, res.best, res.losses)
    assert res.losses == [0.125 ** 2 / 4, 0.375 ** 2 / 4, 0.125 ** 2 / 4, 0.0, 0.0] and len(calls) == 5
    assert torch.equal(calls[2], torch.tensor([0.125, -0.5])) and torch.equal(res.coefficients, centre)

    # a non-finite loss ends the loop with the best iterate so far
    res = L.fitAberrations(torch.zeros((2, 2)), None, None, torch.zeros((2, 4, 4)), 1.0, 1.0, 193.0, iterations=3, step=1.0,
                           imager=lambda v: torch.diag(1.0 / (1.0 - v)), gradient=lambda v, g: -torch.ones(2))
    assert len(res.losses) == 2 and math.isinf(res.losses[1]) and res.best == 0 and float(res.coefficients.abs().max()) == 0.0


def test_end_to_end_retrieval_on_the_oracle_model():
    """The end-to-end case of the device test on the float64 chain: the loss falls and the coefficient error ends smaller than
    at the start -- what entitles the device test to assert the same."""
    c = PG.end_to_end_case()
    assert c.planes == 3 and 30 <= c.shifts.shape[0] <= 40 and c.basis.shape[0] == 2
    res = c.loop(*c.model(), iterations=12, step=0.02)
    err0 = float((c.c0.double() - c.truth.double()).abs().max())
    err = float((res.coefficients.double() - c.truth.double()).abs().max())
    print(f"losses {['%.3e' % v for v in res.losses]}, best {res.best}, steps {res.steps}\ncoefficients {res.coefficients.tolist()} "
          f"(truth {c.truth.tolist()}), error {err:.2e} from {err0:.2e}")
    assert res.losses[res.best] < res.losses[0] and err < err0
    d = c.model()[0](res.coefficients) - c.measured.double()
    assert abs(float((d * d).mean()) - res.losses[res.best]) <= 1e-9 * res.losses[0]


def test_argument_errors():
    import lithographysimulator_amd as L
    m, b = torch.zeros((8, 8)), torch.zeros((3, 16, 16))
    with pytest.raises(ValueError, match="together"):
        L.fitAberrations(m, None, None, b, 1.0, 1.0, 193.0, imager=lambda c: m)
    with pytest.raises(ValueError, match="together"):
        L.fitAberrations(m, None, None, b, 1.0, 1.0, 193.0, gradient=lambda c, g: c)
    with pytest.raises(ValueError, match="iterations"):
        L.fitAberrations(m, None, None, b, 1.0, 1.0, 193.0, iterations=0, imager=lambda c: m, gradient=lambda c, g: c)
    with pytest.raises(ValueError, match="step"):
        L.fitAberrations(m, None, None, b, 1.0, 1.0, 193.0, step=0.0, imager=lambda c: m, gradient=lambda c, g: c)
    with pytest.raises(ValueError, match="basis"):
        L.fitAberrations(m, None, None, b[0], 1.0, 1.0, 193.0, imager=lambda c: m, gradient=lambda c, g: c)
    with pytest.raises(ValueError, match="initial"):
        L.fitAberrations(m, None, None, b, 1.0, 1.0, 193.0, initial=torch.zeros(4), imager=lambda c: m, gradient=lambda c, g: c)
    g = torch.zeros((4, 4), dtype=torch.complex64)
    assert float(L.wavefrontGradient(g + 1j, g + 1.0)[0, 0]) == pytest.approx(2 * math.pi)
    with pytest.raises(ValueError, match="wavefrontGradient"):
        L.wavefrontGradient(g, g[:2])
    for name in ("pupilGradient", "wavefrontGradient", "zernikeBasis", "aberrationGradient", "fitAberrations", "AberrationResult"):
        assert name in L.__all__ and hasattr(L, name)


def test_the_abi_refuses_bad_arguments_without_a_device():
    """Every check of litho_pupil_vjp and litho_pupil_project is made before any launch: codes, not crashes, on a machine without
    a GPU (the pointers are never dereferenced on the host)."""
    from lithographysimulator_amd import _native as nat
    lib = nat.lib()
    assert {"litho_pupil_vjp", "litho_pupil_vjp_work_bytes", "litho_pupil_project", "litho_pupil_project_work_bytes"} <= set(nat.exported_symbols())
    buf = torch.zeros(64, dtype=torch.complex64)
    p = nat.ptr(buf)
    wb = lib.litho_pupil_vjp_work_bytes
    assert wb(2, 3, 5, 32) == 5 * 2 * 3 * 32 * 32 * 8                        # one chunk of fields and nothing else
    for bad in ((0, 3, 5, 32), (2, 0, 5, 32), (2, 3, 0, 32), (2, 3, 5, 24), (2, 3, 5, 8), (2, 3, 5, 8192), (1, 1, 1 << 20, 4096),
                (1 << 16, 1 << 16, 1, 16)):
        assert wb(*bad) == 0, bad
    big = 1 << 40

    def call(pupils=p, maskFT=p, gradI=p, groups=1, K=1, shifts=p, weights=p, count=4, pn=32, N=64, grad=p, accumulate=0, batch=2,
             work=p, work_bytes=big):
        return lib.litho_pupil_vjp(pupils, maskFT, gradI, groups, K, shifts, weights, count, pn, N, grad, accumulate, batch, work,
                                   work_bytes, None)

    for name in ("pupils", "maskFT", "gradI", "shifts", "grad", "work"):
        assert call(**{name: None}) == nat.E_ARG, name
    for pn, N, rc in ((24, 64, nat.E_ARG), (48, 64, nat.E_ARG), (8, 64, nat.E_ARG), (8192, 8192, nat.E_ARG), (32, 48, nat.E_ARG),
                      (32, 8192, nat.E_ARG), (64, 32, nat.E_NSMALL), (4096, 2048, nat.E_NSMALL)):
        assert call(pn=pn, N=N) == rc, (pn, N)
    assert call(count=-1) == nat.E_ARG
    assert call(batch=0) == nat.E_ARG and call(batch=-3) == nat.E_ARG
    assert call(groups=0) == nat.E_ARG and call(K=0) == nat.E_ARG
    assert call(pn=4096, N=4096, batch=1 << 20) == nat.E_ARG                  # more than INT_MAX lines in a chunk
    need = wb(1, 1, 2, 32)
    assert call(work_bytes=need - 1) == nat.E_WORKSPACE and call(work_bytes=0) == nat.E_WORKSPACE
    # an empty list added to what grad holds: nothing to do and nothing launched
    assert call(count=0, accumulate=1, work_bytes=need) == nat.LITHO_OK

    pwb = lib.litho_pupil_project_work_bytes
    assert pwb(1, 5, 16) == 1 * 5 * 4 and pwb(3, 66, 256) == 384 * 66 * 4 and pwb(1, 1, 4096) == 1024 * 4
    for bad in ((0, 5, 32), (1, 0, 32), (1, 1025, 32), (1, 5, 24), (1, 5, 8), (1, 5, 8192)):
        assert pwb(*bad) == 0, bad

    def project(grad=p, pupils=p, planes=1, basis=p, J=5, pn=32, out=p, work=p, work_bytes=big):
        return lib.litho_pupil_project(grad, pupils, planes, basis, J, pn, out, work, work_bytes, None)

    for name in ("grad", "pupils", "basis", "out", "work"):
        assert project(**{name: None}) == nat.E_ARG, name
    assert project(planes=0) == nat.E_ARG and project(J=0) == nat.E_ARG and project(J=1025) == nat.E_ARG and project(pn=48) == nat.E_ARG
    assert project(work_bytes=pwb(1, 5, 32) - 1) == nat.E_WORKSPACE
