"""CPU restatement (torch, float64 / complex128) of the two centred transforms every image is built from, written from the
definitions in include/litho_abbe.h and oracle/abbe_oracle.py -- not from the kernels:

  * the mask spectrum (Mask._ffFraunhofer, mask.py:74-90): the mask is scaled bilinearly by epsilon in fp32, put into an
    N x N frame (zero-padded, or cropped when it is larger), and
        S[q, p] = sum_{j,k} frame[j, k] exp(-2 pi i ((q - c)(j - N/2) + (p - c)(k - N/2)) / N),  c = pn / 2,  q, p in [0, pn);
  * the single-point field (calculateFFTAerial, imageformation.py:32-45):
        E[q, p] = sum_{i,j} A[i, j] exp(+2 pi i ((q - c)(i - c) + (p - c)(j - c)) / N),  A = pupil * mask spectrum.

oracle.abbe_oracle states the same in the reference's fp32 op chain: the parity target.  This file is the instrument for
"is the kernel as accurate as fp32 allows": everything after the fp32 scaled image (which golden g3 pins to the reference) is
float64, and FP32_CHAIN_FLOOR records how far the reference's own fp32 chain is from it.  tests/test_spectrum_cpu.py pins this
file; tests/test_gpu_spectrum.py holds the HIP kernels to 4 x that floor."""
import math

import numpy as np
import torch

from oracle import abbe_oracle as O

C128 = torch.complex128

# max |fp32 chain - float64| / ||scaled image||_F of the reference's chain (fp32_chain below: torch's CPU FFT in complex64) on
# the seeded +-1 mask (pm1_mask(pn, SEED_FLOOR)), the larger of the two product ratios (pn = N / 2 at epsilon 1.0363, pn = N at
# epsilon 0.9948); measure_floor() measures one entry.  N <= 4096 over the whole pn x pn array, N = 8192 and 16384 on the 24
# sampled rows and 24 sampled columns.  The reference chain measuring itself: no kernel of this project ran for these numbers.
# tests/test_spectrum_cpu.py re-measures N <= 2048 and fails if an entry is off by more than a factor 2.
FP32_CHAIN_FLOOR = {
    16: 2.01e-7, 32: 3.04e-7, 64: 4.20e-7, 128: 5.84e-7, 256: 5.82e-7, 512: 8.40e-7, 1024: 7.88e-7, 2048: 1.12e-6,
    4096: 1.10e-6, 8192: 9.17e-7, 16384: 9.94e-7,
}
# The same measurement on `lines_mask(N / 2) - 0.5` at 25 nm pixels (measure_floor_product).  That input is NOT zero-mean (18 % of
# the four-bar pattern is clear: mean -0.32), its DC order is 0.64 ns times ||x||_F, and the fp32 rounding of that one number
# alone is 100 times the zero-mean floor: no fp32 result can meet the table above on it, the reference's own chain included.
# Its floor is therefore its own.  (`bernoulli_mask - 0.5` is zero-mean -- 1.05e-6 and 8.7e-7 by the same measurement -- and uses the table above.)
FP32_CHAIN_FLOOR_LINES = {4096: 9.62e-5, 8192: 1.99e-4}
BOUND_FACTOR = 4                               # a kernel may be this many times further from float64 than the reference's chain
EPS_HALF, EPS_FULL = 1.0363, 0.9948            # the product's ratios: pn = N / 2 (25 nm pixels at 193 nm) and pn = N
SEED_FLOOR = 20240

# (pn, N, epsilon): the smallest sizes at which each awkward shape of the mask-spectrum chain can happen
AWKWARD = [
    (30, 32, 0.9),           # pn no multiple of 4 (the last 4-column tile is ragged), down-scaled, ns = 27 odd
    (34, 64, 0.92),          # the same with padding on both sides, ns = 31
    (64, 64, 1.3264),        # the scaled image is cropped: ns = 84, ns - N even
    (64, 64, 1.30),          # ... ns = 83, ns - N odd: the floor division of a negative pad differs by one
    (64, 64, 1.0),           # ns = pn = N: the copy branch, no padding
    (64, 128, 1.0),          # the copy branch, padded
    (64, 128, 2.0),          # ns = N exactly
    (64, 256, 0.829),        # N = 4 pn, ns = 53
    (16, 16, 0.07),          # ns = 1: a single sample
    (96, 256, 1.0363),       # pn no power of two
    (100, 128, 1.0363),
    (1000, 2048, 1.0363),    # a window of 1036 samples, frame offset 506
    (1000, 2048, 1.0383),    # ... of 1038 samples at the odd frame offset 505
]


def bound(N):
    """What tests/test_gpu_spectrum.py allows in err_norm at FFT size N.  Why 4: a radix-16 transform with float64-rounded
    table twiddles and a CPU library FFT are both O(u sqrt(log N)) in RMS; the factor covers their different constants and the
    maximum over up to 2.7e8 outputs.  One flipped mask pixel is 95 times above it at the largest sampled size (pn 8192, N 16384)
    (test_spectrum_cpu.py, test_the_bound_resolves_one_sample_faults)."""
    return BOUND_FACTOR * FP32_CHAIN_FLOOR[N]


def case_seed(pn, N, entry=0):
    return 1000003 * entry + 64 * pn + N.bit_length()


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _bytes(pn, seed):
    return torch.from_numpy(np.random.default_rng([int(seed), int(pn)]).integers(0, 256, size=(pn, pn), dtype=np.uint8))


def pm1_mask(pn, seed):
    """Seeded i.i.d. +-1 int16 'geometry': zero mean, so no order dominates.  (The kernels interpolate the int16 values, they
    do not inspect them.)"""
    return (_bytes(pn, seed) & 1).to(torch.int16).mul_(2).sub_(1)


def complex_map(pn, seed):
    """Seeded complex64 transmission: +-1 real part, +-1 imaginary part, 6 pixels in 64 (about a tenth) zero."""
    v = torch.arange(256)
    keep = (v >= 24).to(torch.float32)
    table = torch.complex(((v & 1) * 2 - 1) * keep, ((v & 2) - 1) * keep)
    return table[_bytes(pn, seed + 1).view(-1).to(torch.int32)].view(pn, pn)


def complex_gaussian(pn, seed):
    """Seeded complex64 field of full pn x pn support, unit-variance real and imaginary parts."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.complex(torch.randn(pn, pn, generator=g), torch.randn(pn, pn, generator=g))


def sample_lines(pn, seed):
    """The 24 output rows (equally: columns) compared at the sizes whose float64 frame does not fit: the edges, the centre
    and its neighbours, both sides of the 64 and 1024 boundaries, the rest seeded."""
    c = pn // 2
    fixed = [0, 1, c - 1, c, c + 1, pn - 2, pn - 1, 63, 64, 1023, 1024]
    fixed = sorted({q for q in fixed if 0 <= q < pn})
    rest = [int(q) for q in np.random.default_rng([int(seed), int(pn), 7]).permutation(pn) if int(q) not in fixed]
    return sorted(fixed + rest[:max(0, min(24, pn) - len(fixed))])


# ---------------------------------------------------------------------------------------------------------------------------
# mask spectrum
# ---------------------------------------------------------------------------------------------------------------------------
def _resize(img, eps):
    """oracle.abbe_oracle.bilinear_resize (pinned to the reference by golden g3) with the x interpolation done once per input
    row instead of once per output row: l0y (l0x a + l1x b) + l1y (l0x c + l1x d) reads its two brackets from
    X = l0x img[:, i0] + l1x img[:, i1].  The same fp32 operations on the same operands, so the same bits
    (tests/test_spectrum_cpu.py compares them), at a quarter of the gathers: 16384^2 in 2 s instead of 6.5 s."""
    img = img.contiguous()
    n_in = img.shape[0]
    n_out = int(math.floor(n_in * eps))
    if n_out == n_in:
        return img.clone()
    rs = torch.tensor(1.0 / eps, dtype=torch.float32)
    dst = torch.arange(n_out, dtype=torch.float64)
    src = torch.clamp((rs.double() * (dst + 0.5) - 0.5).to(torch.float32), min=0.0)
    i0 = src.floor().to(torch.int64)
    i1 = torch.clamp(i0 + 1, max=n_in - 1)
    l1 = src - i0.to(torch.float32)
    l0 = 1.0 - l1
    X = img[:, i0].mul_(l0[None, :]).add_(img[:, i1].mul_(l1[None, :]))
    return X[i0].mul_(l0[:, None]).add_(X[i1].mul_(l1[:, None]))


def scaled_image(x, eps):
    """The fp32 image the transform under test starts from: the reference's bilinear resize by epsilon, applied to the real
    and to the imaginary part of a complex input.  A resize fault of the code under test still shows: one scaled sample off by
    delta moves every order by delta."""
    x = torch.as_tensor(x)
    if x.is_complex():
        return torch.complex(_resize(x.real.to(torch.float32), eps), _resize(x.imag.to(torch.float32), eps))
    return _resize(x.to(torch.float32), eps)


def frame_window(ns, N):
    """Where the ns x ns scaled image sits in the N x N frame (mask.py:79-81): frame[j] = image[j - pW] with
    pW = ((N - pn) - (ns - pn)) // 2 in Python floor division (pn cancels); the reference pads pW before and pW + ns % 2
    after, and a negative pad crops.  Returns (pW, j0, j1): the frame samples [j0, j1) hold image samples."""
    pW = (N - ns) // 2
    assert pW + ns + pW + ns % 2 == N
    return pW, max(pW, 0), min(pW + ns, N)


def _frame(scaled, N, pW=None):
    ns = scaled.shape[0]
    if pW is None:
        pW = frame_window(ns, N)[0]
    j0, j1 = max(pW, 0), min(pW + ns, N)
    f = torch.zeros((N, N), dtype=C128)
    f[j0:j1, j0:j1] = scaled[j0 - pW:j1 - pW, j0 - pW:j1 - pW].to(C128)
    return f


def _crop(pn, N):
    lo = (N - pn) // 2
    return slice(lo, lo + pn)


def spectrum_f64(scaled, pn, N, pW=None):
    """complex128 [pn, pn]: the scaled image in its frame, centred forward DFT, centre pn x pn.  (pW: a displaced window, for
    the sensitivity checks only.)"""
    f = torch.fft.fftshift(torch.fft.fft2(torch.fft.ifftshift(_frame(scaled, N, pW))))
    k = _crop(pn, N)
    return f[k, k].contiguous()


def _phase_matrix(u, j, N, sign):
    """exp(sign 2 pi i u[r] j[k] / N) with the product reduced modulo N in integers: every angle is exact to one rounding."""
    k = torch.remainder(torch.outer(u.to(torch.int64), j.to(torch.int64)), N).to(torch.float64)
    ang = (sign * 2.0 * math.pi / N) * k
    return torch.complex(torch.cos(ang), torch.sin(ang))


def _project(x, Er, Ec, block=512):
    """(Er @ x, x @ Ec^T) in complex128 in one pass over x, a block of rows at a time; either matrix may be None.  x is a
    tensor [n, n] of any dtype, or a pair (P, M) standing for the elementwise product P M taken in complex128."""
    pair = isinstance(x, tuple)
    n = (x[0] if pair else x).shape[0]
    R = torch.zeros((Er.shape[0], n), dtype=C128) if Er is not None else None
    C = torch.empty((n, Ec.shape[0]), dtype=C128) if Ec is not None else None
    for i0 in range(0, n, block):
        i1 = min(i0 + block, n)
        blk = x[0][i0:i1].to(C128) * x[1][i0:i1].to(C128) if pair else x[i0:i1].to(C128)
        if R is not None:
            R += Er[:, i0:i1] @ blk
        if C is not None:
            C[i0:i1] = blk @ Ec.transpose(0, 1)
    return R, C


def _centred_lines(lines, j0, N, pn, sign):
    """lines [R, w] sit at frame samples [j0, j0 + w): centred 1-D DFT of length N along the last axis, centre pn bins."""
    f = torch.zeros((lines.shape[0], N), dtype=C128)
    f[:, j0:j0 + lines.shape[1]] = lines
    f = torch.fft.ifftshift(f, dim=1)
    f = torch.fft.fft(f, dim=1) if sign < 0 else torch.fft.ifft(f, dim=1, norm="forward")
    return torch.fft.fftshift(f, dim=1)[:, _crop(pn, N)].contiguous()


def _window_of(scaled, N, pW):
    ns = scaled.shape[0]
    if pW is None:
        pW = frame_window(ns, N)[0]
    j0, j1 = max(pW, 0), min(pW + ns, N)
    return scaled[j0 - pW:j1 - pW, j0 - pW:j1 - pW], j0, j1


def spectrum_lines_f64(scaled, pn, N, rows, cols, pW=None):
    """Rows `rows` ([len(rows), pn]) and columns `cols` ([pn, len(cols)]) of spectrum_f64 without the N x N frame: an explicit
    DFT-matrix product over the image window along one axis (E[r, j] = exp(-2 pi i (q_r - c)(j - N/2) / N)), then a centred
    1-D FFT along the other.  Either list may be None."""
    win, j0, j1 = _window_of(scaled, N, pW)
    j = torch.arange(j0, j1) - N // 2
    Er, Ec = (None if q is None else _phase_matrix(torch.as_tensor(list(q)) - pn // 2, j, N, -1.0) for q in (rows, cols))
    R, C = _project(win, Er, Ec)
    return (None if R is None else _centred_lines(R, j0, N, pn, -1),
            None if C is None else _centred_lines(C.transpose(0, 1), j0, N, pn, -1).transpose(0, 1).contiguous())


def spectrum_rows_f64(scaled, pn, N, rows, pW=None):
    return spectrum_lines_f64(scaled, pn, N, rows, None, pW)[0]


def spectrum_cols_f64(scaled, pn, N, cols, pW=None):
    return spectrum_lines_f64(scaled, pn, N, None, cols, pW)[1]


def fp32_chain(scaled, pn, N):
    """The reference's chain from the scaled image on, op for op in fp32 / complex64 (oracle.abbe_oracle.mask_spectrum with
    epsilon and N chosen by the caller): pad, fftshift, fft2, ifftshift, crop.  Used to measure FP32_CHAIN_FLOOR."""
    ns = scaled.shape[0]
    pW = ((N - pn) - (ns - pn)) // 2
    corr = ns % 2
    padded = torch.nn.functional.pad(scaled, (pW, pW + corr, pW, pW + corr))
    spec = torch.fft.ifftshift(torch.fft.fft2(torch.fft.fftshift(padded), norm="backward"))
    trim = (N - pn) // 2
    return torch.nn.functional.pad(spec, (-trim, -trim, -trim, -trim))


# ---------------------------------------------------------------------------------------------------------------------------
# single-point field
# ---------------------------------------------------------------------------------------------------------------------------
def field_f64(A, pn, N):
    """complex128 E = F A F^T, F[q, i] = exp(+2 pi i (q - c)(i - c) / N) (oracle.centred_dft_matrix), as A centred in the
    N x N frame, unnormalised centred inverse DFT, centre pn x pn."""
    k = _crop(pn, N)
    f = torch.zeros((N, N), dtype=C128)
    f[k, k] = A.to(C128)
    return torch.fft.fftshift(torch.fft.ifft2(torch.fft.ifftshift(f), norm="forward"))[k, k].contiguous()


def field_lines_f64(A, pn, N, rows, cols):
    """Rows and columns of field_f64, as spectrum_lines_f64: the matrix product along one axis, a centred inverse-sign 1-D FFT
    along the other.  A: a [pn, pn] tensor, or a pair (P, M) for A = P M multiplied in complex128 block by block (a 16384^2
    product is 4 GB otherwise)."""
    c = pn // 2
    i = torch.arange(pn) - c
    Er, Ec = (None if q is None else _phase_matrix(torch.as_tensor(list(q)) - c, i, N, +1.0) for q in (rows, cols))
    R, C = _project(A, Er, Ec)
    return (None if R is None else _centred_lines(R, N // 2 - c, N, pn, +1),
            None if C is None else _centred_lines(C.transpose(0, 1), N // 2 - c, N, pn, +1).transpose(0, 1).contiguous())


def field_rows_f64(A, pn, N, rows):
    return field_lines_f64(A, pn, N, rows, None)[0]


def field_cols_f64(A, pn, N, cols):
    return field_lines_f64(A, pn, N, None, cols)[1]


# ---------------------------------------------------------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------------------------------------------------------
def fro(x):
    """||x||_F in double, a block of rows at a time; a pair (P, M) stands for the elementwise product."""
    if isinstance(x, tuple):
        return math.sqrt(sum(fro(p.to(C128) * m.to(C128)) ** 2 for p, m in zip(x[0].split(1024), x[1].split(1024))))
    return math.sqrt(sum(float(torch.linalg.vector_norm(torch.view_as_real(b) if b.is_complex() else b, dtype=torch.float64)) ** 2
                         for b in torch.split(torch.as_tensor(x), 1024)))


def err_norm(got, ref, scaled):
    """max |got - ref| / ||scaled||_F: the error in the natural unit of an FFT, the 2-norm of its input (every output of an
    fp32 transform carries a rounding error proportional to it, whatever the output's own size).  `scaled` may be the norm."""
    norm = scaled if isinstance(scaled, float) else fro(scaled)
    return float((torch.as_tensor(got).to(C128) - torch.as_tensor(ref).to(C128)).abs().max()) / norm


def measure_floor(N, ratio, sampled=None):
    """err_norm of the reference's fp32 chain against float64 at FFT size N, ratio 'half' (pn = N / 2) or 'full' (pn = N), on
    the seeded +-1 mask.  sampled: compare the sample_lines rows and columns only (default: from N = 8192 up)."""
    pn, eps = (N // 2, EPS_HALF) if ratio == "half" else (N, EPS_FULL)
    scaled = scaled_image(pm1_mask(pn, SEED_FLOOR), eps)
    got = fp32_chain(scaled, pn, N)
    if sampled is None:
        sampled = N > 4096
    if not sampled:
        return err_norm(got, spectrum_f64(scaled, pn, N), scaled)
    q = sample_lines(pn, SEED_FLOOR)
    norm = fro(scaled)
    R, C = spectrum_lines_f64(scaled, pn, N, q, q)
    return max(err_norm(got[q, :], R, norm), err_norm(got[:, q], C, norm))


def product_mask(kind, pn):
    """The product's own 0 / 1 masks (lithographysimulator_amd.synthetic) and their epsilon, N at 25 nm pixels, 193 nm."""
    from lithographysimulator_amd.synthetic import bernoulli_mask, lines_mask
    eps, N = O.calculate_epsilon_n(4 / pn, 25, 193.0)
    return (lines_mask(pn) if kind == "lines" else bernoulli_mask(pn)), eps, N


def measure_floor_product(kind, pn):
    """measure_floor on `product_mask(kind, pn) - 0.5` (N = 2 pn; whole array at N = 4096, sampled lines at 8192)."""
    geo, eps, N = product_mask(kind, pn)
    scaled = scaled_image(geo.to(torch.float32) - 0.5, eps)
    got = fp32_chain(scaled, pn, N)
    if N <= 4096:
        return err_norm(got, spectrum_f64(scaled, pn, N), scaled)
    q = sample_lines(pn, SEED_FLOOR)
    norm = fro(scaled)
    R, C = spectrum_lines_f64(scaled, pn, N, q, q)
    return max(err_norm(got[q, :], R, norm), err_norm(got[:, q], C, norm))
