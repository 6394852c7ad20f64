"""The inverse-lithography loop on the GPU: optimizeMask's device model (lithographysimulator_amd/ilt.py `_device_model`: Mask
spectrum, hopkinsIntensity, gain, postProcess and back through postProcessAdjoint, gain, hopkinsGradient, maskSpectrumAdjoint)
and the loop on it, against the float64 chain of tests/socs_grad_oracle.py.

Settings (GO.IltCase): K = 3 band-limited kernels of GO.sized_case around a SOCSKernels with weight_sum 2.7, so that `normalize`
is not the identity; pixel sizes of GO.epsilon_regimes (shrink / crop / copy of both resizes, pad and crop), deltaK = 4 / pn,
193 nm; pn 32 and 64, one plane and a stack of two -- the smallest sizes at which both resizes, the pad / crop and the stacked
adjoint all act.  dose 1.1, a seeded theta0 and target, the threshold at the median of the oracle image.

Bounds (socs_grad_oracle.py, "Loop tolerances"): the complex64 CPU chain against the float64 one on exactly these cases lies
under a quarter of helpers.TOL_IMAGE_MAX / TOL_IMAGE_L2 for the image and for the adjoint, so those are their bounds; through the
loop the resist sigmoid amplifies an image error about 25-fold, and the bounds are four times the complex64 loop's own floor.
Every test prints what it observed (-s)."""
import pytest
import torch

import socs_grad_oracle as GO

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


def _device_hooks(case, normalize, dev):
    """(socs, imager, adjoint): the SOCSKernels of the case and optimizeMask's own device model around it."""
    from lithographysimulator_amd.ilt import _device_model
    socs = GO.socs_around(case.kernels, dev, weight_sum=GO.ILT_WEIGHT_SUM)
    return (socs,) + tuple(_device_model(socs, case.pn, case.ps, 4 / case.pn, 193.0, normalize, dev))


# ---- the device model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,regime,planes,normalize", GO.ILT_DEVICE_CASES)
def test_device_image_against_the_oracle(L, dev, pn, regime, planes, normalize):
    """imager(t) for a complex transmission (background 0.1 + 0.2j, feature 1, sigmoid of theta0: both parts vary)."""
    case = GO.device_case(pn, regime, planes, normalize)
    _, imager, _ = _device_hooks(case, normalize, dev)
    got = imager(case.t0.to(torch.complex64).to(dev))
    assert got.dtype == torch.float32 and got.device == dev
    assert tuple(got.shape) == tuple(case.image0.shape) == ((planes, case.n_out, case.n_out) if planes > 1 else (case.n_out, case.n_out))
    e_max, e_l2 = GO.rel_max(got, case.image0), GO.rel_l2(got, case.image0)
    print(f"image pn {pn} {regime} planes {planes} normalize {normalize}: max {e_max:.2e} ({e_max / GO.TOL_ILT_IMAGE_MAX:.3f} of the "
          f"bound {GO.TOL_ILT_IMAGE_MAX:.0e}), l2 {e_l2:.2e} ({e_l2 / GO.TOL_ILT_IMAGE_L2:.3f} of {GO.TOL_ILT_IMAGE_L2:.0e})")
    assert e_max < GO.TOL_ILT_IMAGE_MAX and e_l2 < GO.TOL_ILT_IMAGE_L2


@pytest.mark.parametrize("pn,regime,planes,normalize", GO.ILT_DEVICE_CASES)
def test_device_adjoint_against_the_oracle(L, dev, pn, regime, planes, normalize):
    """The same gradient on the image for both sides -- the float64 closed form of the loss at the oracle image, cast to fp32,
    both signs -- so that the sigmoid's amplification of an image error stays out of the comparison.  For a stack the result
    must also lie further than the bound from the adjoint of either plane alone: a plane silently dropped is caught."""
    case = GO.device_case(pn, regime, planes, normalize)
    _, imager, adjoint = _device_hooks(case, normalize, dev)
    t = case.t0.to(torch.complex64)
    G = case.grad_image0.to(torch.float32)
    assert bool((G < 0).any()) and bool((G > 0).any())
    imager64, adjoint64 = case.model()
    imager64(t)
    want = adjoint64(G)
    imager(t.to(dev))
    got = adjoint(G.to(dev))
    assert got.dtype == torch.complex64 and tuple(got.shape) == (pn, pn) and got.device == dev
    e_max, e_l2 = GO.rel_max(got, want), GO.rel_l2(got, want)
    print(f"adjoint pn {pn} {regime} planes {planes} normalize {normalize}: max {e_max:.2e} ({e_max / GO.TOL_ILT_ADJOINT_MAX:.3f} of "
          f"the bound {GO.TOL_ILT_ADJOINT_MAX:.0e}), l2 {e_l2:.2e} ({e_l2 / GO.TOL_ILT_ADJOINT_L2:.3f} of {GO.TOL_ILT_ADJOINT_L2:.0e})")
    assert e_max < GO.TOL_ILT_ADJOINT_MAX and e_l2 < GO.TOL_ILT_ADJOINT_L2
    for p in range(planes if planes > 1 else 0):
        im_p, ad_p = GO.model(case.kernels[p], pn, case.eps, case.N, case.gain)
        im_p(t)
        alone = ad_p(G[p])
        away = GO.rel_max(got, alone)
        print(f"    from plane {p} alone: {away:.2e} of its maximum")
        assert away > 1e3 * GO.TOL_ILT_ADJOINT_MAX


# ---- the loop, default device path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,regime,kind,normalize", GO.ILT_LOOP_CASES)
def test_one_iteration_on_the_device(L, dev, pn, regime, kind, normalize):
    """optimizeMask(initial=theta0, iterations=1) with no hooks, for a binary mask, an attenuated one (background -sqrt(0.06)), a
    complex background (0.1 + 0.2j) and that background on a two-plane stack: both losses and the update (theta0 - theta1) /
    step against the same loop on the float64 chain, which descends in its first step (asserted), so theta1 is what both return.
    The same call through imager= / adjoint= taken from _device_model, and the call repeated, give the same bits: nothing in the
    chain uses atomics."""
    case = GO.loop_case(pn, regime, kind, normalize)
    ref = case.reference()
    assert ref.best == 1 and ref.losses[1] < ref.losses[0]
    socs, imager, adjoint = _device_hooks(case, normalize, dev)

    def run(kernels=socs, **kw):
        return L.optimizeMask(case.target.to(dev), kernels, case.ps, 4 / pn, 193.0, case.threshold, dose=GO.ILT_DOSE,
                              initial=case.theta0.to(dev), iterations=1, step=GO.ILT_STEP, background=case.background,
                              normalize=normalize, **kw)

    got = run()
    assert got.best == 1 and len(got.losses) == 2
    e_loss = [abs(got.losses[i] - ref.losses[i]) / ref.losses[i] for i in (0, 1)]
    e_up = float((GO.update_of(case, got) - GO.update_of(case, ref)).abs().max())
    print(f"loop pn {pn} {regime} {kind} normalize {normalize}: losses {got.losses[0]:.8f} -> {got.losses[1]:.8f} (oracle "
          f"{ref.losses[0]:.8f} -> {ref.losses[1]:.8f}), relative {e_loss[0]:.2e}, {e_loss[1]:.2e} ({max(e_loss) / GO.TOL_ILT_LOSS:.3f} of "
          f"the bound {GO.TOL_ILT_LOSS:.1e}); update {e_up:.2e} ({e_up / GO.TOL_ILT_UPDATE:.3f} of {GO.TOL_ILT_UPDATE:.1e})")
    assert max(e_loss) < GO.TOL_ILT_LOSS and e_up < GO.TOL_ILT_UPDATE
    hooked = run(GO.Grid(pn), imager=imager, adjoint=adjoint)
    again = run()
    for other in (hooked, again):
        assert other.losses == got.losses and other.best == got.best
        assert torch.equal(other.theta, got.theta) and torch.equal(torch.view_as_real(other.transmission), torch.view_as_real(got.transmission))


# ---- the arguments the device branch handles --------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["shrink", "crop", "copy"])
@pytest.mark.parametrize("pn", [32, 64])
def test_device_branch_arguments(L, dev, pn, regime):
    """A target of another size than the post-processed grid is refused by name of the right size; `initial` and `target` on the
    CPU are moved to the device; what comes back lives there, in the documented types."""
    case = GO.loop_case(pn, regime, "binary", True)
    socs = GO.socs_around(case.kernels, dev, weight_sum=GO.ILT_WEIGHT_SUM)
    n = case.n_out
    for bad in (n - 1, n + 1):
        with pytest.raises(ValueError, match=rf"\[{n},{n}\]"):
            L.optimizeMask(torch.zeros((bad, bad), device=dev), socs, case.ps, 4 / pn, 193.0, case.threshold)
    args = dict(dose=GO.ILT_DOSE, iterations=1, step=GO.ILT_STEP)
    on_dev = L.optimizeMask(case.target.to(dev), socs, case.ps, 4 / pn, 193.0, case.threshold, initial=case.theta0.to(dev), **args)
    res = L.optimizeMask(case.target, socs, case.ps, 4 / pn, 193.0, case.threshold, initial=case.theta0, **args)
    assert res.losses == on_dev.losses and torch.equal(res.theta, on_dev.theta)
    assert res.theta.device == dev and res.mask.device == dev and res.transmission.device == dev
    assert res.theta.dtype == torch.float32 and res.mask.dtype == torch.bool and res.transmission.dtype == torch.complex64
    assert tuple(res.theta.shape) == tuple(res.mask.shape) == tuple(res.transmission.shape) == (pn, pn)
    assert torch.equal(res.mask, res.theta > 0)
    print(f"pn {pn} {regime}: n_out {n}, losses {res.losses}")
