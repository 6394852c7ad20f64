"""Truncated SOCS kernels on the device: socsKernels with litho_tcc_apply as the operator, at the defaults (kernels 64,
oversample 16, iterations 2), K = 16 and (K 24, oversample 8), pn 64, N 128 -- the regime Hopkins imaging is used in, which the
full-rank parity tests of test_gpu_socs.py cannot see.

Four optical settings from tests/socs_oracle.py (truncated_setting): (a) ideal pupil, annular 0.4-0.8, weight 1, S = 380;
(b) demo aberrations, disc 0-0.6, S = 293; (c) demo aberrations, the shifted annular source that wraps the pupil around the grid,
grey weights, S = 380; (d) as (c) with weights over four decades.  One two-plane stack (demo aberrations, 120 nm defocus) over
source (a).  Truth is float64 on the CPU: the exact spectrum lambda of T from the S x S Gram matrix, the operator norm of
T - sum_k phi_k phi_k^H (socs_oracle.residual_norm), the weighted Abbe sum for the image.  Per kernel set (check_truncated):

  theta descending, >= 0, theta_k <= lambda_k + 1e-5 lambda_1            (Rayleigh-Ritz values never exceed the exact ones)
  |captured - sum theta / trace| <= 1e-12;  |sum |phi_k|^2 - theta_k| <= 1e-5 theta_1
  exact - 1e-3 <= captured <= exact + 1e-5,  exact = sum_{k<=K} lambda_k / trace
  (1 - 1e-3) lambda_{K+1} <= residual norm <= 1.5 lambda_{K+1}            (Eckart-Young below, the truncation rule above)
  exact zeros outside the masking box, a strict restriction of the grid, where the source does not wrap ((a), (b), the stack)

and for (a), (c) at K = 16, 64 the image: error against the float64 Abbe sum <= 1.5 x the exact top-K kernels' + TOL_IMAGE_MAX.

Measured with the float64 operator on the CPU (tests/test_socs_cpu.py, the same assertions): theta - lambda <= 4.8e-8 lambda_1,
energy identity <= 4.9e-8 theta_1, captured deficit 3.5e-5 ... 7.0e-4 (worst: (b), K 64), residual / lambda_{K+1} <= 1.0003 at
K 16, 1.12 ... 1.29 at K 64, 1.19 at (K 24, oversample 8); image ratio for (a) 1.03 at K 16 and 1.01 at K 64.
Measured on an MI355X (litho_tcc_apply as the operator), the thirteen sets of kernels, stack planes included: theta - lambda
between -3.9e-8 and -1.9e-9 lambda_1 (never above the exact value); energy identity <= 1.3e-7 theta_1; captured deficit 3.1e-5
... 7.3e-4 (worst: (b), K 64); residual / lambda_{K+1} 1.0001 ... 1.0013 at K 16, 1.11 ... 1.31 at K 64 ((a) 1.31, (b) 1.24,
(c) 1.26, (d) 1.11, stack 1.21 and 1.19), 1.12 at (K 24, oversample 8); image ratio (a) 0.995 at K 16 and 1.005 at K 64, (c) 0.989
and 1.091; the stack's planes differ by 0.40 of the largest kernel sample and 4.1e-2 lambda_1 in their spectra.  On the CPU
the ratio at K 64 spreads over 1.20 ... 1.29 with the seed of the random start alone ((a) and (b), six seeds each); the device
draws its start from its own generator."""
import numpy as np
import pytest
import torch

import socs_oracle as SO
from helpers import TOL_IMAGE_MAX, rel_max

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


_sets, _truths = {}, {}


def _kernels(L, dev, name, K, oversample):
    """socsKernels of one run on the device, made once (the image test takes the sets of the kernel test)."""
    key = (name, K, oversample)
    if key not in _sets:
        P, W = SO.truncated_setting(name)
        if (K, oversample) == (64, 16):
            _sets[key] = L.socsKernels(P.to(dev), W.to(dev))                    # the defaults, as a caller gets them
        else:
            _sets[key] = L.socsKernels(P.to(dev), W.to(dev), kernels=K, oversample=oversample)
    return _sets[key]


def _truth(name):
    if name not in _truths:
        P, W = SO.truncated_setting(name)
        _truths[name] = SO.abbe_truth(P, SO.truncated_mask(), W.numpy(), SO.TRUNC_N)
    return _truths[name]


@pytest.mark.parametrize("name,K,oversample", SO.TRUNC_RUNS)
def test_truncated_kernels_against_the_exact_spectrum(L, dev, name, K, oversample):
    k = _kernels(L, dev, name, K, oversample)
    assert k.K == K and not k.stacked and k.kernels.dtype == torch.complex64 and k.eigenvalues.dtype == torch.float64
    assert (k.boxes == [None]) == (name in "cd")                                # (c) and (d) wrap, (a) and (b) are masked
    assert abs(k.trace - SO.truncated_exact(name)[2]) <= 1e-12 * k.trace
    SO.check_truncated(f"device {name}", name, K, k.kernels, k.eigenvalues, k.captured, k.boxes[0])


@pytest.mark.parametrize("K", [16, 64])
@pytest.mark.parametrize("name", ["a", "c"])
def test_truncated_image_against_the_exact_truncation(L, dev, name, K):
    P, W = SO.truncated_setting(name)
    M, N, truth = SO.truncated_mask(), SO.TRUNC_N, _truth(name)
    exact = SO.exact_kernels(P.numpy(), W.numpy(), K=K)[0]
    floor = rel_max(SO.kernel_image(torch.from_numpy(exact), M, N), truth)
    k = _kernels(L, dev, name, K, 16)
    err = rel_max(L.hopkinsIntensity(M.to(dev), k, N).cpu(), truth)
    print(f"device {name} K {K}: image error {err:.3e}, exact top-{K} kernels {floor:.3e}, ratio {err / floor:.3f} (bound 1.5 x + "
          f"{TOL_IMAGE_MAX:.0e})")
    assert err <= 1.5 * floor + TOL_IMAGE_MAX


@pytest.mark.parametrize("K", [16, 64])
def test_truncated_stack_plane_by_plane(L, dev, K):
    """Demo aberrations and 120 nm defocus over source (a): each plane against its own exact spectrum."""
    names = ("a_demo", "a_f120")
    W = SO.truncated_setting("a")[1]
    pupils = torch.stack([SO.truncated_setting(n)[0] for n in names]).to(dev)
    k = L.socsKernels(pupils, W.to(dev), kernels=K)
    assert k.stacked and k.planes == 2 and tuple(k.kernels.shape) == (2, K, 64, 64) and tuple(k.eigenvalues.shape) == (2, K)
    for p, n in enumerate(names):
        assert k.boxes[p] is not None
        assert abs(float(k.trace[p]) - SO.truncated_exact(n)[2]) <= 1e-12 * float(k.trace[p])
        SO.check_truncated(f"device stack plane {p} ({n})", n, K, k.kernels[p], k.eigenvalues[p], float(k.captured[p]), k.boxes[p])
    apart = rel_max(k.kernels[1].abs().cpu(), k.kernels[0].abs().cpu())
    spectra = float((k.eigenvalues[1] - k.eigenvalues[0]).abs().max() / k.eigenvalues[0, 0])
    print(f"stack K {K}: |kernels| of the planes differ by {apart:.3f} of the maximum, eigenvalues by {spectra:.2e} lambda_1")
    assert apart > 1e-2
