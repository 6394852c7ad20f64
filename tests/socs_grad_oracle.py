"""CPU restatement of the mask-gradient definitions (include/litho_abbe.h "Mask gradients", lithographysimulator_amd/ilt.py) in
float64, written from the formulas and not from the kernels.  TEST INFRASTRUCTURE ONLY.

    F = O.centred_dft_matrix(pn, N),  L(X) = F X F^T,  E_k = L(phi_k . M),  I = sum_k |E_k|^2  (per plane of a stack)
    g = dl/dRe M + i dl/dIm M = 2 sum_p sum_k conj(phi_pk) . L^H(G_p . E_pk),   L^H(Y) = conj(F) Y conj(F)^T

The two linear bookends are restated through explicit dense matrices: the mask-spectrum chain of O.mask_spectrum (for a complex
transmission) is S(t) = B t B^T with B = crop . centred forward DFT . pad-or-crop . R, and O.post_process on a non-negative image is
Pp raw Pp^T with Pp = pad . R'; their adjoints are B^H y conj(B) and Pp^T g Pp.  R comes from O.bilinear_resize itself, applied
to probe images (`resize_matrix`), so nothing here re-derives torch's coordinate rule.

Gradient tolerance.  The device's line transforms and a float64 reference differ by fp32 rounding, so the bound comes from the
fp32 floor of the formula itself: the same formula is evaluated in torch's CPU complex64 and compared with this file on the cases
of the GPU tests (test_socs_grad_cpu.py::test_fp32_floor_of_the_gradient_formula prints and re-checks it).  Where that error is
below a quarter of helpers.TOL_IMAGE_MAX / TOL_IMAGE_L2 the project's image tolerances are the bound, otherwise four times the
measured error (the factor covers the different summation order).  Measured:
    max|dg| / max|g| <= 7.9e-7 and ||dg||_2 / ||g||_2 <= 7.5e-7 over all of them (the largest at pn 1024 and at (16, 512)),
both below a quarter of helpers.TOL_IMAGE_MAX (2e-5 / 4 = 5e-6) and TOL_IMAGE_L2 (5e-6 / 4 = 1.25e-6), so the gradient is held
to the project's image tolerances themselves."""
import math

import numpy as np
import torch

from helpers import TOL_IMAGE_L2, TOL_IMAGE_MAX
from oracle import abbe_oracle as O

C128 = torch.complex128
# the measured complex64 floor of the gradient formula (see the head of the file) and the bounds chosen from it
FP32_FLOOR_MAX, FP32_FLOOR_L2 = 7.9e-7, 7.5e-7
TOL_GRAD_MAX, TOL_GRAD_L2 = TOL_IMAGE_MAX, TOL_IMAGE_L2
# |<A x, y> - <x, A^H y>| <= TOL_ADJOINT ||A x|| ||y|| for the fp32 forwards: fp32 unit round-off 6e-8 times the 14 ... 24 butterfly
# stages of these sizes is about 1.5e-6, which leaves a seven-fold margin; a structural error (a missing shift, a transposed R, a
# wrong pad side) shows at order 1
TOL_ADJOINT = 1e-5


def _k4(kernels):
    k = torch.as_tensor(kernels)
    return (k if k.dim() == 4 else k[None]), k.dim() == 4


def fields(kernels, M, N, dtype=C128):
    """E[.., k] = F (phi_k . M) F^T: [K,pn,pn] or [planes,K,pn,pn] like `kernels`."""
    k4, stacked = _k4(kernels)
    pn = k4.shape[-1]
    F = O.centred_dft_matrix(pn, N, dtype=dtype)
    E = F @ (k4.to(dtype) * torch.as_tensor(M).to(dtype)) @ F.T
    return E if stacked else E[0]


def intensity(kernels, M, N):
    """float64 sum_k |E_k|^2: [pn,pn] or [planes,pn,pn]."""
    E = fields(kernels, M, N)
    return (E.real ** 2 + E.imag ** 2).sum(dim=-3)


def gradient(kernels, M, N, G, dtype=C128):
    """g of the head of the file for G = dl/dI ([pn,pn] or [planes,pn,pn]); `dtype` complex64 evaluates the same formula in torch's
    CPU single precision (the floor the device's bound is derived from)."""
    k4, _ = _k4(kernels)
    pn = k4.shape[-1]
    real = torch.float64 if dtype == C128 else torch.float32
    F = O.centred_dft_matrix(pn, N, dtype=dtype)
    G3 = torch.as_tensor(G).to(real).reshape(k4.shape[0], 1, pn, pn)
    phi = k4.to(dtype)
    E = F @ (phi * torch.as_tensor(M).to(dtype)) @ F.T
    A = F.conj() @ (G3 * E) @ F.conj().T
    return 2.0 * (phi.conj() * A).sum(dim=(0, 1))


def inner(a, b):
    """Re <a, b> = Re sum conj(a) b in float64 (the pairing of dl = Re <g, dM>)."""
    a, b = torch.as_tensor(a).to(C128), torch.as_tensor(b).to(C128)
    return float((a.conj() * b).sum().real)


# ---- the bookends as dense matrices ------------------------------------------------------------------------------------------
def resize_matrix(n_in, scale):
    """float64 [n_out, n_in] holding O.bilinear_resize's fp32 weights along one axis.  Probe j is the image whose row j is all
    ones: the resize along x of a constant row is the constant (l0 + l1 rounds to 1 in fp32 for l0 = fl(1 - l1)), so any column
    of the result is column j of R."""
    cols = []
    for j in range(n_in):
        probe = torch.zeros((n_in, n_in), dtype=torch.float32)
        probe[j, :] = 1.0
        cols.append(O.bilinear_resize(probe, scale)[:, 0])
    return torch.stack(cols, dim=1).double()


def pad_matrix(n_out, n_in, lead):
    """[n_out, n_in] 0/1: F.pad with `lead` samples in front (negative: a crop) -- output index s + lead holds input s."""
    P = torch.zeros((n_out, n_in), dtype=torch.float64)
    for s in range(n_in):
        if 0 <= s + lead < n_out:
            P[s + lead, s] = 1.0
    return P


def spectrum_matrix(pn, epsilon, N):
    """B complex128 [pn, pn] with O.mask_spectrum's chain = B t B^T (mask.py:74-90): resize by epsilon, pad or crop to N
    (pW = (N - ns) // 2 in front), ifftshift . fft . fftshift, centre pn."""
    R = resize_matrix(pn, epsilon)
    ns = R.shape[0]
    Pd = pad_matrix(N, ns, (N - ns) // 2)
    k = torch.arange(N, dtype=torch.float64) - N // 2
    ang = -2 * math.pi * torch.outer(k, k) / N
    Fc = torch.complex(torch.cos(ang), torch.sin(ang))
    trim = (N - pn) // 2
    return Fc[trim:trim + pn] @ (Pd @ R).to(C128)


def spectrum_complex(t, epsilon, N):
    """O.mask_spectrum's chain op for op on a complex transmission, float64 arithmetic on O.bilinear_resize's fp32 weights: the
    resize of the real and of the imaginary part, F.pad, the shifted fft2, the crop."""
    t = torch.as_tensor(t).to(C128)
    pn = t.shape[0]
    scaled = torch.complex(O.bilinear_resize(t.real, epsilon), O.bilinear_resize(t.imag, epsilon))
    ns = scaled.shape[0]
    pW, corr = (N - ns) // 2, ns % 2
    pr = torch.nn.functional.pad(scaled.real, (pW, pW + corr, pW, pW + corr))
    pi = torch.nn.functional.pad(scaled.imag, (pW, pW + corr, pW, pW + corr))
    spec = torch.fft.ifftshift(torch.fft.fft2(torch.fft.fftshift(torch.complex(pr, pi))))
    trim = (N - pn) // 2
    return spec[trim:trim + pn, trim:trim + pn]


def spectrum_adjoint(y, pn, epsilon, N):
    B = spectrum_matrix(pn, epsilon, N)
    return B.conj().T @ torch.as_tensor(y).to(C128) @ B.conj()


def postprocess_matrix(pn, epsilon):
    """Pp float64 [n_out, pn] with O.post_process(raw >= 0) = Pp raw Pp^T (imageformation.py:69-77)."""
    R = resize_matrix(pn, 1.0 / epsilon)
    n2 = R.shape[0]
    pW = (pn - round(pn / epsilon)) // 2
    return pad_matrix(n2 + 2 * pW + n2 % 2, n2, pW) @ R


def postprocess_adjoint(g, pn, epsilon):
    Pp = postprocess_matrix(pn, epsilon)
    return Pp.T @ torch.as_tensor(g).double() @ Pp


def epsilon_regimes(pn):
    """{name: (pixelSize, epsilon, N)} at 193 nm for the three regimes of the resize: "shrink" epsilon < 1; "crop" epsilon > 1 with
    floor(pn epsilon) > N, so that the pad is negative; "copy" floor(pn epsilon) == pn.  beta = 193 pn / (4 pixelSize)."""
    out = {}
    for name, ps in (("shrink", 20.0), ("crop", 60.0), ("copy", 193.0 * pn / (4.0 * (2 * pn - 0.1)))):
        eps, N = O.calculate_epsilon_n(4 / pn, ps, 193.0)
        out[name] = (ps, eps, N)
    return out


def model(kernels, pn, epsilon, N, gain=1.0):
    """(imager, adjoint) for optimizeMask on this file's float64 chain: transmission -> B t B^T -> gain . intensity -> Pp . Pp^T."""
    B, Pp = spectrum_matrix(pn, epsilon, N), postprocess_matrix(pn, epsilon)
    state = {}

    def imager(t):
        state["M"] = B @ torch.as_tensor(t).to(C128) @ B.T
        return Pp @ (gain * intensity(kernels, state["M"], N)) @ Pp.T

    def adjoint(g):
        graw = gain * (Pp.T @ torch.as_tensor(g).double() @ Pp)
        return B.conj().T @ gradient(kernels, state["M"], N, graw) @ B.conj()

    return imager, adjoint


# ---- the cases the CPU floor measurement and the GPU tests share --------------------------------------------------------------
GRAD_SIZES = [(16, 16), (16, 32), (32, 64), (32, 128), (64, 64), (64, 128), (128, 256)]
# further regimes of the line kernel: the two-pass line transform, and m = N / pn > pn (most values of r own no output)
EXTRA_SIZES = [(256, 512), (16, 512), (16, 4096)]
# one line per workgroup, K = 2, one plane: the dense float64 gradient is still a fraction of a second here
LARGE_GRAD_SIZES = [(1024, 1024), (1024, 2048)]
_cases = {}


def random_G(shape, seed):
    """A real dl/dI with both signs and a block of exact zeros."""
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(shape, generator=g, dtype=torch.float64)
    G[..., : shape[-2] // 4, :] = 0.0
    return G.to(torch.float32)


def sized_case(pn, N, K=5, planes=1):
    """(kernels complex64 [K,pn,pn] or [planes,K,pn,pn], M complex64 [pn,pn], G fp32) at any size: band-limited random kernels (the
    inner (pn/2)^2 box, as SOCS kernels of a box-limited pupil are) of decaying norm, the spectrum of an attenuated phase-shift
    Bernoulli mask -- a complex transmission -- through O.mask_spectrum's chain."""
    key = (pn, N, K, planes)
    if key not in _cases:
        from lithographysimulator_amd.mask import attenuatedPSM
        from lithographysimulator_amd.synthetic import bernoulli_mask
        g = torch.Generator().manual_seed(1000 * pn + N + K + planes)
        k = torch.view_as_complex(torch.randn((planes, K, pn, pn, 2), generator=g, dtype=torch.float32))
        box = torch.zeros((pn, pn))
        box[pn // 4:3 * pn // 4, pn // 4:3 * pn // 4] = 1.0
        k = k * box * (0.7 ** torch.arange(K, dtype=torch.float32))[None, :, None, None]
        t = attenuatedPSM(bernoulli_mask(pn))
        # a spectrum as the device's chain would give it, whatever N: the resize is the copy here (epsilon 1)
        M = spectrum_complex(t, 1.0, N).to(torch.complex64)
        G = random_G((planes, pn, pn), pn + N)
        _cases[key] = ((k if planes > 1 else k[0]).contiguous(), M.contiguous(), G if planes > 1 else G[0])
    return _cases[key]
