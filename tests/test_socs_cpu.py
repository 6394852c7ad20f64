"""Hopkins imaging on the CPU: the identities behind the SOCS factorisation (tests/socs_oracle.py, float64) and the host algebra of
socsKernels -- subspace iteration, J clamp, masking box, captured fraction -- run with `applier=` set to the oracle's dense
operator, so no GPU is involved.  Image truth: the float64 weighted Abbe sum (oracle.field_closed_form); tolerances: the
project's TOL_IMAGE_MAX / TOL_IMAGE_L2.  Every test prints what it observed (-s)."""
import numpy as np
import pytest
import torch

import socs_oracle as SO
from helpers import DEMO_AB, NA, TOL_IMAGE_L2, TOL_IMAGE_MAX, WL, f16, rel_l2, rel_max
from oracle import abbe_oracle as O

case, truth = SO.problem, SO.truth


def socs(name, **kw):
    import lithographysimulator_amd as L
    P, W, M, N = case(name)
    return L.socsKernels(P, W, applier=SO.apply_as_applier(P.numpy(), W.numpy()), **kw)


def test_operator_trace_and_gram_identities():
    P, W, M, N = case("wrap32")
    pn = 32
    d, w = SO.source_points(W.numpy())
    assert d.shape[0] == 92 and 0 < w.min() and w.max() <= 2.0
    nz = np.argwhere(P.numpy() != 0)
    assert nz[:, 0].max() + d[:, 0].max() > pn - 1 or nz[:, 0].min() + d[:, 0].min() < 0       # the source wraps the pupil
    A = SO.explicit_A(P.numpy(), W.numpy())
    T = SO.tcc(A)
    assert np.abs(T - T.conj().T).max() <= 1e-12 * np.abs(T).max()
    rng = np.random.default_rng(0)
    X = rng.standard_normal((3, pn, pn)) + 1j * rng.standard_normal((3, pn, pn))
    want = (T @ X.reshape(3, -1).T).T.reshape(3, pn, pn)
    got = SO.dense_apply(P.numpy(), W.numpy(), X)
    e_op = np.abs(got - want).max() / np.abs(want).max()
    tr = float(W.double().sum()) * float((np.abs(P.numpy().astype(np.complex128)) ** 2).sum())
    e_tr = abs(np.trace(T).real - tr) / tr
    G = SO.gram(P.numpy(), W.numpy())
    e_g = np.abs(G - A @ A.conj().T).max() / np.abs(G).max()
    phi, lam = SO.exact_kernels(P.numpy(), W.numpy())
    e_fact = np.abs(np.einsum("kf,kg->fg", phi.reshape(92, -1), phi.reshape(92, -1).conj()) - T).max() / np.abs(T).max()
    e_img = rel_max(SO.kernel_image(torch.from_numpy(phi), M, N), truth("wrap32"))
    print(f"dense operator {e_op:.1e}, trace {e_tr:.1e}, Gram {e_g:.1e}, sum phi phi^H = T {e_fact:.1e}, full-rank image {e_img:.1e}")
    assert e_op < 1e-12 and e_tr < 1e-12 and e_g < 1e-12 and e_fact < 1e-12 and e_img < 1e-12
    assert abs(lam.sum() - tr) < 1e-12 * tr and lam.min() > 0


@pytest.mark.parametrize("name,S", [("wrap32", 92), ("focus64", 40)])
def test_full_rank_kernels_reproduce_the_abbe_image(name, S):
    P, W, M, N = case(name)
    k = socs(name, kernels=S, oversample=0)
    assert k.K == S and k.lit_points == S and tuple(k.kernels.shape) == (S,) + tuple(P.shape) and k.kernels.dtype == torch.complex64
    img = SO.kernel_image(k.kernels, M, N)
    e_max, e_l2 = rel_max(img, truth(name)), rel_l2(img, truth(name))
    print(f"{name}: full rank K = {S}: max {e_max:.2e} (bound {TOL_IMAGE_MAX:.0e}), l2 {e_l2:.2e} (bound {TOL_IMAGE_L2:.0e}), "
          f"captured {k.captured:.8f}")
    assert e_max < TOL_IMAGE_MAX and e_l2 < TOL_IMAGE_L2
    assert abs(k.captured - 1.0) < 1e-5
    lam = k.eigenvalues.numpy()
    assert k.eigenvalues.dtype == torch.float64 and (np.diff(lam) <= 0).all()
    want = SO.exact_kernels(P.numpy(), W.numpy())[1]
    assert np.abs(lam - want).max() < 1e-5 * want[0]


def test_more_vectors_than_lit_points_are_clamped():
    k = socs("focus64", kernels=64, oversample=16)
    assert k.K == 40 and k.kernels.shape[0] == 40
    P, W, M, N = case("focus64")
    img = SO.kernel_image(k.kernels, M, N)
    assert rel_max(img, truth("focus64")) < TOL_IMAGE_MAX and rel_l2(img, truth("focus64")) < TOL_IMAGE_L2


def test_kernel_energy_is_the_eigenvalue_sum_and_captured_is_reported():
    P, W, M, N = case("wrap32")
    k = socs("wrap32", kernels=24, oversample=8)
    energy = float((k.kernels.abs().double() ** 2).sum())
    lam_sum = float(k.eigenvalues.sum())
    tr = float(W.double().sum()) * float((np.abs(P.numpy().astype(np.complex128)) ** 2).sum())
    print(f"K 24: sum |phi|^2 {energy:.6f}, sum lambda {lam_sum:.6f}, trace {tr:.6f}, captured {k.captured:.4f}")
    assert abs(energy - lam_sum) < 1e-5 * lam_sum and lam_sum <= tr * (1 + 1e-6)
    assert abs(k.trace - tr) < 1e-12 * tr and abs(k.captured - lam_sum / tr) < 1e-12 and 0.5 < k.captured < 1.0
    per_kernel = (k.kernels.abs().double() ** 2).sum(dim=(1, 2)).numpy()
    assert np.abs(per_kernel - k.eigenvalues.numpy()).max() < 1e-5 * per_kernel[0]


def test_truncated_kernels_stay_near_the_exact_truncation():
    """K = 24 of 92 at pn 32: image error <= 1.5 x the error of the exact rank-24 truncation + TOL_IMAGE_MAX."""
    P, W, M, N = case("wrap32")
    phi, lam = SO.exact_kernels(P.numpy(), W.numpy())
    floor = rel_max(SO.kernel_image(torch.from_numpy(phi[:24]), M, N), truth("wrap32"))
    k = socs("wrap32", kernels=24, oversample=8)
    err = rel_max(SO.kernel_image(k.kernels, M, N), truth("wrap32"))
    print(f"K 24: image error {err:.3e}, exact rank-24 truncation {floor:.3e}, ratio {err / floor:.3f}")
    assert err <= 1.5 * floor + TOL_IMAGE_MAX


def test_the_masking_box_holds_exact_zeros():
    P, W, M, N = case("focus64")
    k = socs("focus64", kernels=16, oversample=8)
    (box,) = k.boxes
    assert box is not None
    r_lo, r_hi, c_lo, c_hi = box
    nz, (d, _) = np.argwhere(P.numpy() != 0), SO.source_points(W.numpy())
    assert (r_lo, r_hi) == (nz[:, 0].min() + d[:, 0].min(), nz[:, 0].max() + d[:, 0].max())
    assert (c_lo, c_hi) == (nz[:, 1].min() + d[:, 1].min(), nz[:, 1].max() + d[:, 1].max())
    assert 0 < r_lo and r_hi < 63 and 0 < c_lo and c_hi < 63                    # a real restriction of the grid
    outside = torch.ones((64, 64), dtype=torch.bool)
    outside[r_lo:r_hi + 1, c_lo:c_hi + 1] = False
    assert int((k.kernels[:, outside] != 0).sum()) == 0 and int((k.kernels[:, ~outside] != 0).sum()) > 0
    exact = SO.exact_kernels(P.numpy(), W.numpy())[0]                          # the range of T lies inside the box
    assert np.abs(exact[:, outside.numpy()]).max() == 0.0
    assert socs("wrap32", kernels=8, oversample=4).boxes == [None]             # a wrapping source: no masking


def test_a_pupil_stack_is_factored_plane_by_plane():
    import lithographysimulator_amd as L
    P, W, M, N = case("focus64")
    P2 = O.pupil_function(f16(DEMO_AB), 64, NA, WL)
    ap = [SO.apply_as_applier(p.numpy(), W.numpy()) for p in (P, P2)]
    k = L.socsKernels(torch.stack([P, P2]), W, kernels=40, oversample=0, applier=ap)
    assert tuple(k.kernels.shape) == (2, 40, 64, 64) and tuple(k.eigenvalues.shape) == (2, 40) and k.planes == 2 and k.stacked
    assert tuple(k.captured.shape) == (2,) and float((k.captured - 1).abs().max()) < 1e-5
    for p, pupil in enumerate((P, P2)):
        want = truth("focus64") if p == 0 else SO.abbe_truth(pupil, M, W, N)
        img = SO.kernel_image(k.kernels[p], M, N)
        assert rel_max(img, want) < TOL_IMAGE_MAX and rel_l2(img, want) < TOL_IMAGE_L2
    with pytest.raises(ValueError):
        L.socsKernels(torch.stack([P, P2]), W, applier=ap[:1])


def test_refusals():
    import lithographysimulator_amd as L
    from lithographysimulator_amd import _native as nat
    P, W, M, N = case("wrap32")
    ap = SO.apply_as_applier(P.numpy(), W.numpy())
    for bad in (-0.5, float("nan"), float("inf")):
        Wb = W.clone()
        Wb[3, 4] = bad
        with pytest.raises(ValueError, match="negative or not finite"):
            L.socsKernels(P, Wb, applier=ap)
    for pn in (8, 48, 30, 8192):
        with pytest.raises(ValueError, match="power of two, 16 ... 4096"):
            L.socsKernels(torch.empty((pn, pn), dtype=torch.complex64), W, applier=ap)
    with pytest.raises(ValueError):
        L.socsKernels(P, torch.zeros_like(W), applier=ap)                      # nothing lit
    with pytest.raises(ValueError):
        L.socsKernels(P, W[:16], applier=ap)                                   # another grid
    with pytest.raises(ValueError):
        L.socsKernels(P, W, kernels=0, applier=ap)
    with pytest.raises(RuntimeError):
        L.socsKernels(P, W)                                                    # no applier: the device operator, and P is on the CPU
    for name in ("litho_fft2_c2c", "litho_tcc_apply", "litho_socs_fold"):
        assert name in nat.exported_symbols()
    with pytest.raises(ValueError, match="model"):
        L.correctLayout([np.array([[0.0, 0.0], [100.0, 0.0], [100.0, 100.0], [0.0, 100.0]])], 32, 25.0, (0.0, 0.0), WL, None, None,
                        0.3, spacing=50.0, maxBias=10.0, imager=lambda p: None, epe=lambda i: None, model="hopkins")


def test_an_integer_bitmap_means_weight_one():
    P, W, M, N = case("focus64")
    bitmap = (W > 0).to(torch.int64) * 3                                       # non-zero = lit, whatever the value
    import lithographysimulator_amd as L
    ones = (W > 0).to(torch.float32)
    k = L.socsKernels(P, bitmap, kernels=40, oversample=0, applier=SO.apply_as_applier(P.numpy(), ones.numpy()))
    assert k.weight_sum == 40.0
    want = SO.abbe_truth(P, M, ones, N)
    img = SO.kernel_image(k.kernels, M, N)
    assert rel_max(img, want) < TOL_IMAGE_MAX and rel_l2(img, want) < TOL_IMAGE_L2


# ---- the oracle's spectrum and residual norm, and the host algebra on truncated sets (pn 64) ----------------------------------
def test_exact_spectrum_and_top_k_kernels():
    P, W, M, N = case("wrap32")
    phi, lam = SO.exact_kernels(P.numpy(), W.numpy())
    spec = SO.exact_spectrum(P.numpy(), W.numpy())
    top, lam_top = SO.exact_kernels(P.numpy(), W.numpy(), K=24)
    assert spec.shape == (92,) and spec.dtype == np.float64 and (np.diff(spec) <= 0).all()
    assert np.abs(spec - lam).max() <= 1e-12 * lam[0] and np.array_equal(lam_top, lam)
    assert top.shape == (24, 32, 32) and np.array_equal(top, phi[:24])


@pytest.mark.parametrize("name", ["wrap32", "focus64"])
def test_residual_norm_against_eckart_young(name):
    """The exact top-K kernels leave exactly lambda_{K+1}; no kernels at all leave lambda_1; all S leave nothing."""
    P, W, M, N = case(name)
    A = SO.explicit_A(P.numpy(), W.numpy())
    phi, lam = SO.exact_kernels(P.numpy(), W.numpy())
    S, F = A.shape
    for K in (1, 8, 24, S - 1):
        r = SO.residual_norm(A, phi[:K])
        print(f"{name} K {K}: residual {r:.12e}, lambda_K+1 {lam[K]:.12e}, relative difference {abs(r - lam[K]) / lam[K]:.1e}")
        assert abs(r - lam[K]) <= 1e-10 * lam[K]
    r0 = SO.residual_norm(A, np.zeros((5, F)))
    rS = SO.residual_norm(A, phi)
    print(f"{name}: zero rows {r0:.12e} (lambda_1 {lam[0]:.12e}), all {S} kernels {rS / lam[0]:.1e} lambda_1")
    assert abs(r0 - lam[0]) <= 1e-10 * lam[0]
    assert rS <= 1e-12 * lam[0]
    if name == "wrap32":                                                        # and it is the norm of the explicit residual
        K = 24
        E = SO.tcc(A) - np.einsum("kf,kg->fg", phi[:K].reshape(K, -1), phi[:K].reshape(K, -1).conj())
        assert abs(np.linalg.norm(E, 2) - SO.residual_norm(A, phi[:K])) <= 1e-10 * lam[K]


def test_the_pn64_settings_are_what_the_tests_say():
    sizes = {n: int((SO.truncated_setting(n)[1] > 0).sum()) for n in "abcd"}
    assert sizes == {"a": 380, "b": 293, "c": 380, "d": 380}
    w = SO.truncated_setting("d")[1]
    assert float(w[w > 0].min()) < 2e-4 and float(w.max()) > 0.5                # four decades
    for n in "cd":                                                              # the shifted source is not symmetric
        W = SO.truncated_setting(n)[1]
        assert not torch.equal(W, W.T)


@pytest.mark.parametrize("name,K,oversample", SO.TRUNC_RUNS)
def test_truncated_host_algebra_at_64(name, K, oversample):
    """socsKernels with the float64 dense operator as `applier`: what tests/test_gpu_socs_truncated.py asserts on the device,
    minus the image."""
    import lithographysimulator_amd as L
    P, W = SO.truncated_setting(name)
    k = L.socsKernels(P, W, kernels=K, oversample=oversample, applier=SO.apply_as_applier(P.numpy(), W.numpy()))
    seen = SO.check_truncated(f"cpu {name}", name, K, k.kernels, k.eigenvalues, k.captured, k.boxes[0])
    assert seen["wraps"] == (name in "cd") and k.K == K and abs(k.trace - SO.truncated_exact(name)[2]) <= 1e-12 * k.trace


def test_truncated_host_algebra_on_a_stack():
    import lithographysimulator_amd as L
    names = ("a_demo", "a_f120")
    Ps = [SO.truncated_setting(n)[0] for n in names]
    W = SO.truncated_setting("a")[1]
    k = L.socsKernels(torch.stack(Ps), W, applier=[SO.apply_as_applier(p.numpy(), W.numpy()) for p in Ps])
    assert tuple(k.kernels.shape) == (2, 64, 64, 64)
    for p, n in enumerate(names):
        SO.check_truncated(f"cpu stack plane {p} ({n})", n, 64, k.kernels[p], k.eigenvalues[p], float(k.captured[p]), k.boxes[p])
    assert rel_max(k.kernels[1].abs(), k.kernels[0].abs()) > 1e-2               # the planes' kernels differ
