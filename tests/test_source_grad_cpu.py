"""Source gradients without a GPU: the oracle's linearity identity, optimizeSource on CPU hooks (its gradient against central
differences of its own float64 loss, the projection, the best iterate, the all-zero stop), the fp32 floors the device bounds are
derived from, and the C ABI's argument checks (made before any launch, so the codes come back without a device)."""
import pytest
import torch

import socs_grad_oracle as GO
import source_grad_oracle as SG
from helpers import TOL_IMAGE_L2, TOL_IMAGE_MAX


def _within(measured, recorded):
    """As in test_socs_grad_cpu.py: the recorded floor is what one machine printed when the bound was chosen; another host BLAS
    sums in another order, so the re-check allows a factor 2 and still catches a floor that has really moved."""
    return measured <= 2.0 * recorded


def test_linearity_identity_on_the_oracle_alone():
    """sum_s w_s sens_s = <G, I_w> to float64 round-off, I_w the weighted Abbe sum built from oracle.abbe_oracle's single-point
    field (the restatement of the reference's calculateFFTAerial): ties the restated sensitivities to the yardstick's field."""
    for pn, N in ((16, 16), (16, 64), (32, 64), (64, 64)):
        P, M, G, sh = SG.case(pn, N)
        g = torch.Generator().manual_seed(pn + N)
        w = torch.rand(sh.shape[0], generator=g, dtype=torch.float64)
        assert float(G.min()) < 0 < float(G.max())
        sens = SG.sensitivities(P, M, sh, N, G)
        lhs = float((w * sens).sum())
        Iw = SG.weighted_image(P[0], M, sh, w, N)
        rhs = float((G.double() * Iw).sum())
        scale = float((G.double().abs() * Iw).sum())
        print(f"pn {pn} N {N}: |lhs - rhs| / sum |G| I_w = {abs(lhs - rhs) / scale:.2e}")
        assert abs(lhs - rhs) <= 1e-12 * scale


def test_fp32_floor_of_the_sensitivity_formula():
    """The fp32 floor the device bound is derived from (source_grad_oracle.py, "Tolerance"): the same formula in torch's CPU
    complex64 against float64 on exactly the GPU tests' cases, measured against the oracle and never against the device."""
    worst_max = worst_l2 = worst_abs = 0.0
    for key in SG.ORACLE_CASES:
        P, M, G, sh = SG.case(*key)
        s64 = SG.reference(*key)
        s32 = SG.sensitivities(P, M, sh, key[1], G, K=key[3], dtype=torch.complex64).double()
        sabs = SG.sensitivities(P, M, sh, key[1], G, K=key[3], absolute=True)
        d = s32 - s64
        e_max, e_l2 = float(d.abs().max() / s64.abs().max()), float(torch.linalg.norm(d) / torch.linalg.norm(s64))
        e_abs = float((d.abs() / sabs).max())
        print(f"{key}: max {e_max:.2e}  l2 {e_l2:.2e}  relative to sum |G| |E|^2 {e_abs:.2e}")
        worst_max, worst_l2, worst_abs = max(worst_max, e_max), max(worst_l2, e_l2), max(worst_abs, e_abs)
    print(f"complex64 formula vs float64 over {len(SG.ORACLE_CASES)} cases: max {worst_max:.2e} (recorded {SG.FP32_FLOOR_MAX:.1e}), "
          f"l2 {worst_l2:.2e} (recorded {SG.FP32_FLOOR_L2:.1e}), relative to the sum without cancellation {worst_abs:.2e} "
          f"(recorded {SG.FP32_FLOOR_ABS:.1e})")
    assert _within(worst_max, SG.FP32_FLOOR_MAX) and _within(worst_l2, SG.FP32_FLOOR_L2) and _within(worst_abs, SG.FP32_FLOOR_ABS)
    assert worst_max < TOL_IMAGE_MAX / 4 and worst_l2 < TOL_IMAGE_L2 / 4
    # the rule: the image tolerances where the floor is under a quarter of them, four times the floor otherwise
    assert SG.TOL_SENS_MAX == (TOL_IMAGE_MAX if SG.FP32_FLOOR_MAX < TOL_IMAGE_MAX / 4 else 4 * SG.FP32_FLOOR_MAX)
    assert SG.TOL_SENS_L2 == (TOL_IMAGE_L2 if SG.FP32_FLOOR_L2 < TOL_IMAGE_L2 / 4 else 4 * SG.FP32_FLOOR_L2)


def test_fp32_floor_of_the_source_loop():
    """The floor behind TOL_SMO_LOSS / TOL_SMO_UPDATE: the one-iteration loop on the complex64 chain against the float64 chain, on
    the device tests' cases."""
    worst_loss = worst_update = 0.0
    for key in SG.SMO_LOOP_CASES:
        c = SG.smo_case(*key)
        ref, got = c.reference(), c.loop(*c.model(dtype=torch.complex64))
        e_loss = max(abs(a - b) / b for a, b in zip(got.losses, ref.losses))
        e_update = float((SG.update_of(c, got) - SG.update_of(c, ref)).abs().max())
        print(f"{key}: losses {ref.losses}, relative {e_loss:.2e}; update {e_update:.2e}")
        worst_loss, worst_update = max(worst_loss, e_loss), max(worst_update, e_update)
    print(f"loop floor: loss {worst_loss:.2e} (recorded {SG.SMO_FLOOR_LOSS:.1e}), update {worst_update:.2e} (recorded "
          f"{SG.SMO_FLOOR_UPDATE:.1e})")
    assert _within(worst_loss, SG.SMO_FLOOR_LOSS) and _within(worst_update, SG.SMO_FLOOR_UPDATE)
    assert (SG.TOL_SMO_LOSS, SG.TOL_SMO_UPDATE) == (4 * SG.SMO_FLOOR_LOSS, 4 * SG.SMO_FLOOR_UPDATE)


@pytest.mark.parametrize("pn,planes,normalize", [(32, 1, True), (32, 1, False), (32, 2, True), (32, 2, False)])
def test_loop_gradient_is_the_derivative_of_its_loss(pn, planes, normalize):
    """sourceLossGradient's gradient against central differences of its own float64 loss, along every weight and along a random
    direction; the points include a wrapping shift (dy = -pn/2 against a disc of radius pn/4).  The loss and the closed forms are
    also the oracle file's."""
    import lithographysimulator_amd as L
    c = SG.smo_case(pn, planes, normalize)
    assert any(abs(dy) + pn // 4 >= pn // 2 for dy, _ in c.shifts.tolist())
    imager, sensitivity = c.model()
    w = c.w0.double()
    target = c.target.double()

    def loss_of(v):
        return float(L.sourceLossGradient(v, target, imager, sensitivity, c.threshold, SG.SMO_DOSE, c.a_r, normalize)[0])

    loss, grad = L.sourceLossGradient(w, target, imager, sensitivity, c.threshold, SG.SMO_DOSE, c.a_r, normalize)
    image = imager(w) / (float(w.sum()) if normalize else 1.0)
    assert abs(float(loss) - SG.smo_loss(image, target, c.threshold, SG.SMO_DOSE, c.a_r)) <= 1e-14 * float(loss)
    G = SG.smo_grad_image(image, target, c.threshold, SG.SMO_DOSE, c.a_r)
    g = sensitivity(G)
    want = SG.normalised_gradient(g, G, image, w.sum()) if normalize else g
    assert float((grad - want).abs().max()) <= 1e-12 * float(want.abs().max())
    gen = torch.Generator().manual_seed(5)
    dirs = list(torch.eye(w.numel(), dtype=torch.float64)) + [torch.randn(w.numel(), generator=gen, dtype=torch.float64)]
    h = 1e-6
    for d in dirs:
        fd = (loss_of(w + h * d) - loss_of(w - h * d)) / (2 * h)
        an = float((grad * d).sum())
        print(f"pn {pn} planes {planes} normalize {normalize}: fd {fd:.6e}  analytic {an:.6e}")
        # h^2 truncation (third derivative ~ a_r^2 larger than the first) and eps64 |l| / h rounding both lie under 1e-6 of the
        # gradient's scale; a wrong term shows at order 0.1 ... 1
        assert abs(fd - an) <= 1e-6 * float(grad.abs().max())


def test_projection_best_iterate_and_the_all_zero_stop():
    import lithographysimulator_amd as L
    c = SG.smo_case(32, 1, True)
    res = L.optimizeSource(c.target, None, None, c.candidates, c.ps, 4 / c.pn, 193.0, c.threshold, dose=SG.SMO_DOSE, iterations=12,
                           step=1.5, imager=c.model()[0], sensitivity=c.model()[1])
    # a step of 1.5 max(w) sends weights through zero: the projection holds them there
    assert float(res.weights.min()) >= 0.0 and bool((res.weights == 0).any()) and bool(torch.isfinite(res.weights).all())
    assert res.best == min(range(len(res.losses)), key=res.losses.__getitem__)
    assert tuple(res.source.shape) == (c.pn, c.pn) and res.source.dtype == torch.float32
    assert torch.equal(res.source[c.candidates != 0], res.weights) and float(res.source[c.candidates == 0].abs().max()) == 0.0
    # the returned weights give the recorded best loss
    image = c.model()[0](res.weights.double()) / float(res.weights.double().sum())
    assert abs(SG.smo_loss(image, c.target, c.threshold, SG.SMO_DOSE, c.a_r) - res.losses[res.best]) <= 1e-6 * res.losses[res.best]
    # the first update is the oracle's projected update of the oracle's gradient
    first = c.reference()
    w0 = c.w0.double()
    image0 = c.model()[0](w0) / float(w0.sum())
    G0 = SG.smo_grad_image(image0, c.target, c.threshold, SG.SMO_DOSE, c.a_r)
    grad0 = SG.normalised_gradient(c.model()[1](G0), G0, image0, w0.sum())
    assert float((first.weights.double() - SG.projected_update(w0, grad0, SG.SMO_STEP)).abs().max()) <= 1e-6

    # a gradient that is positive and equal everywhere with step >= 1 zeroes every weight at once: the loop ends there and
    # returns the best iterate so far, the start
    calls = []

    def imager(w):
        calls.append(w.clone())
        return w.sum() / 512 * torch.ones((4, 4))                               # the threshold: the resist is on its slope

    res = L.optimizeSource(torch.zeros((4, 4)), None, None, torch.ones((16, 16)), 1.0, 1.0, 193.0, 0.5, iterations=5, step=1.0,
                           normalize=False, imager=imager, sensitivity=lambda g: g.sum() * torch.ones(256))
    assert len(calls) == 1 and len(res.losses) == 1 and res.best == 0 and torch.equal(res.weights, torch.ones(256))


def test_argument_errors():
    import lithographysimulator_amd as L
    t = torch.zeros((8, 8))
    cand = torch.ones((16, 16))
    with pytest.raises(ValueError, match="together"):
        L.optimizeSource(t, None, None, cand, 1.0, 1.0, 193.0, 0.5, imager=lambda w: t)
    with pytest.raises(ValueError, match="iterations"):
        L.optimizeSource(t, None, None, cand, 1.0, 1.0, 193.0, 0.5, iterations=0, imager=lambda w: t, sensitivity=lambda g: g)
    with pytest.raises(ValueError, match="no lit point"):
        L.optimizeSource(t, None, None, torch.zeros((16, 16)), 1.0, 1.0, 193.0, 0.5, imager=lambda w: t, sensitivity=lambda g: g)
    with pytest.raises(ValueError, match="non-negative"):
        L.optimizeSource(t, None, None, -cand, 1.0, 1.0, 193.0, 0.5, imager=lambda w: t, sensitivity=lambda g: g)
    with pytest.raises(ValueError, match="rounds"):
        L.optimizeSourceMask(t, torch.zeros((16, 16)), cand, 1.0, 1.0, 193.0, 0.5, rounds=0)
    for name in ("sourceSensitivities", "sourceGradient", "optimizeSource", "optimizeSourceMask", "SourceResult"):
        assert name in L.__all__ and hasattr(L, name)


def test_the_abi_refuses_bad_arguments_without_a_device():
    """Every check of litho_source_sensitivity is made before any launch: codes, not crashes, on a machine without a GPU (the
    pointers are never dereferenced on the host)."""
    from lithographysimulator_amd import _native as nat
    lib = nat.lib()
    assert {"litho_source_sensitivity", "litho_source_sensitivity_work_bytes"} <= set(nat.exported_symbols())
    buf = torch.zeros(64, dtype=torch.complex64)
    p = nat.ptr(buf)
    wb = lib.litho_source_sensitivity_work_bytes
    # batch groups K field planes, one transposed copy of gradI, one partial per line
    assert wb(2, 3, 5, 32) == 5 * 2 * 3 * 32 * 32 * 8 + 2 * 32 * 32 * 4 + 5 * 2 * 3 * 32 * 4
    for bad in ((0, 3, 5, 32), (2, 0, 5, 32), (2, 3, 0, 32), (2, 3, 5, 24), (2, 3, 5, 8), (2, 3, 5, 8192), (1, 1, 1 << 20, 4096),
                (1 << 16, 1 << 16, 1, 16)):
        assert wb(*bad) == 0, bad
    big = 1 << 40

    def call(pupils=p, maskFT=p, gradI=p, groups=1, K=1, shifts=p, count=4, pn=32, N=64, sens=p, batch=2, work=p, work_bytes=big):
        return lib.litho_source_sensitivity(pupils, maskFT, gradI, groups, K, shifts, count, pn, N, sens, batch, work, work_bytes, None)

    for name in ("pupils", "maskFT", "gradI", "shifts", "sens", "work"):
        assert call(**{name: None}) == nat.E_ARG, name
    for pn, N, rc in ((24, 64, nat.E_ARG), (48, 64, nat.E_ARG), (8, 64, nat.E_ARG), (8192, 8192, nat.E_ARG), (32, 48, nat.E_ARG),
                      (32, 8192, nat.E_ARG), (64, 32, nat.E_NSMALL), (4096, 2048, nat.E_NSMALL)):
        assert call(pn=pn, N=N) == rc, (pn, N)
    assert call(count=-1) == nat.E_ARG
    assert call(batch=0) == nat.E_ARG and call(batch=-3) == nat.E_ARG
    assert call(groups=0) == nat.E_ARG and call(K=0) == nat.E_ARG
    assert call(pn=4096, N=4096, batch=1 << 20) == nat.E_ARG                  # more than INT_MAX lines in a chunk
    need = wb(1, 1, 2, 32)
    assert call(work_bytes=need - 1) == nat.E_WORKSPACE
    assert call(work_bytes=0) == nat.E_WORKSPACE
    # count = 0: nothing to do and nothing launched, so this returns LITHO_OK without a device too
    assert call(count=0, work_bytes=need) == nat.LITHO_OK
