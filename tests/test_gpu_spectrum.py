"""The mask-spectrum chain (k_scale_mask*, k_xpass<LOG2N, -1, RealImageLoader | ComplexImageLoader>, k_ypass_field<LOG2N, -1>) and
the single-point field (xpass_general, k_ypass_field<LOG2N, +1>) order by order against float64 (tests/spectrum_oracle.py), at every
FFT size N = 16 ... 16384, at the two ratios the product runs (pn = N / 2, pn = N), through both loaders.

Inputs are zero-mean (seeded +-1 int16 masks, seeded +-1 +- i maps with a tenth of the pixels zero, complex-Gaussian fields), so no
order dominates and the error is measured in the unit of an FFT, err_norm = max |got - f64| / ||input||_F.  The bound is
4 x FP32_CHAIN_FLOOR[N]: four times what the reference's own fp32 chain (torch's CPU FFT in complex64) is away from float64 at the
same size -- recorded in spectrum_oracle.py, re-measured by test_spectrum_cpu.py, which also shows on the reference alone that a
single wrong sample is 95 times above the bound at the largest size.  N <= 4096 compares the whole pn x pn array (the field: N <=
2048), the larger sizes 24 output rows and 24 output columns (spectrum_oracle.sample_lines).

Measured on an MI355X: err_norm and its quotient by the floor (the bound is a quotient of 4).

                       forward, pn = N / 2 (eps 1.0363)   forward, pn = N (eps 0.9948)     inverse (field)
    N      floor       int16           complex           int16           complex           pn = N / 2      pn = N
   16   2.01e-07    1.87e-07 0.93   1.48e-07 0.74   2.85e-07 1.42   2.95e-07 1.47     2.12e-07 1.05   2.93e-07 1.46
   32   3.04e-07    3.41e-07 1.12   2.26e-07 0.74   3.29e-07 1.08   4.34e-07 1.43     2.46e-07 0.81   3.26e-07 1.07
   64   4.20e-07    4.53e-07 1.08   3.85e-07 0.92   3.98e-07 0.95   4.45e-07 1.06     3.34e-07 0.79   4.27e-07 1.02
  128   5.84e-07    4.25e-07 0.73   5.58e-07 0.96   5.57e-07 0.95   6.25e-07 1.07     4.09e-07 0.70   4.94e-07 0.85
  256   5.82e-07    7.47e-07 1.28   6.49e-07 1.12   6.82e-07 1.17   7.27e-07 1.25     4.97e-07 0.85   6.20e-07 1.07
  512   8.40e-07    7.32e-07 0.87   8.02e-07 0.95   8.49e-07 1.01   8.03e-07 0.96     6.14e-07 0.73   7.08e-07 0.84
 1024   7.88e-07    9.25e-07 1.17   9.32e-07 1.18   9.78e-07 1.24   9.29e-07 1.18     7.29e-07 0.93   7.69e-07 0.98
 2048   1.12e-06    1.01e-06 0.90   9.90e-07 0.88   9.37e-07 0.84   9.30e-07 0.83     7.70e-07 0.69   7.89e-07 0.70
 4096   1.10e-06    1.17e-06 1.07   1.26e-06 1.14   1.16e-06 1.05   1.09e-06 0.99     7.47e-07 0.68   8.52e-07 0.77
 8192   9.17e-07    1.12e-06 1.22   1.05e-06 1.15   1.15e-06 1.26   9.47e-07 1.03     8.30e-07 0.90   8.80e-07 0.96
16384   9.94e-07    1.07e-06 1.07   1.03e-06 1.04   1.11e-06 1.12   1.08e-06 1.08     8.71e-07 0.88   9.29e-07 0.93

Awkward shapes, product footprints - 0.5 and the limit cases (int16 | complex where both ran):
  awkward N 32 pn 30 eps 0.9 ns 27             floor 3.04e-07   3.57e-07 1.17  |  3.44e-07 1.13
  awkward N 64 pn 34 eps 0.92 ns 31            floor 4.20e-07   3.92e-07 0.93  |  3.97e-07 0.95
  awkward N 64 pn 64 eps 1.3264 ns 84          floor 4.20e-07   3.75e-07 0.89  |  3.91e-07 0.93
  awkward N 64 pn 64 eps 1.3 ns 83             floor 4.20e-07   3.74e-07 0.89  |  4.81e-07 1.14
  awkward N 64 pn 64 eps 1.0 ns 64             floor 4.20e-07   3.79e-07 0.90  |  3.53e-07 0.84
  awkward N 128 pn 64 eps 1.0 ns 64            floor 5.84e-07   3.44e-07 0.59  |  4.54e-07 0.78
  awkward N 128 pn 64 eps 2.0 ns 128           floor 5.84e-07   7.12e-07 1.22  |  9.28e-07 1.59
  awkward N 256 pn 64 eps 0.829 ns 53          floor 5.82e-07   5.11e-07 0.88  |  5.57e-07 0.96
  awkward N 16 pn 16 eps 0.07 ns 1             floor 2.01e-07   2.23e-07 1.11  |  1.74e-07 0.87
  awkward N 256 pn 96 eps 1.0363 ns 99         floor 5.82e-07   6.29e-07 1.08  |  6.38e-07 1.10
  awkward N 128 pn 100 eps 1.0363 ns 103       floor 5.84e-07   5.05e-07 0.87  |  5.48e-07 0.94
  awkward N 2048 pn 1000 eps 1.0363 ns 1036    floor 1.12e-06   1.09e-06 0.97  |  1.06e-06 0.95
  awkward N 2048 pn 1000 eps 1.0383 ns 1038    floor 1.12e-06   1.00e-06 0.89  |  9.72e-07 0.87
  product bern - 0.5 N 4096 pn 2048 complex    floor 1.10e-06   1.26e-06 1.14
  product bern - 0.5 N 8192 pn 4096 complex    floor 9.17e-07   1.22e-06 1.33
  product lines - 0.5 N 4096 pn 2048 complex   floor 9.62e-05   1.03e-04 1.07
  product lines - 0.5 N 8192 pn 4096 complex   floor 1.99e-04   1.97e-04 0.99
  limit N 16 pn 16 eps 11.3125 ns 181 int16    floor 2.01e-07   2.51e-08 0.12
  limit N 16 pn 16 eps 8.0 ns 128 complex      floor 2.01e-07                     4.81e-08 0.24

The product's 0 / 1 masks, max |d| / DC (bound 2e-6): Bernoulli 7.2e-8 (pn 2048) and 7.5e-8 (pn 4096), lines 1.4e-7 and 1.5e-7;
lines - 0.5 through the complex entry 7.6e-8 and 7.3e-8.

Largest quotient: 1.59 (awkward N 128 pn 64 eps 2.0 ns 128 complex).  Nothing failed: no kernel or host code changed.
"""
import math

import pytest
import torch

import spectrum_oracle as S
from helpers import PS, WL

pytestmark = pytest.mark.gpu
FULL_SPECTRUM, FULL_FIELD = 4096, 2048          # largest N compared as a whole array
RATIOS = {"half": S.EPS_HALF, "full": S.EPS_FULL}


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


def gpu_spectrum(L, dev, x, eps, N):
    """Mask._ffFraunhofer at a chosen epsilon and N: the int16 entry for an integer geometry, the complex entry otherwise."""
    mask = L.Mask(pixelSize=PS, device=dev, transmission=x) if x.is_complex() else L.Mask(x, PS, dev)
    assert (mask.transmission is not None) == x.is_complex()
    got = mask._ffFraunhofer(eps, N)
    torch.cuda.synchronize()
    assert got.dtype == torch.complex64 and tuple(got.shape) == (x.shape[0],) * 2
    return got


def _worst(d, rows=None, cols=None):
    """Where a residual sits: its largest element and the lines that carry it."""
    a = d.abs()
    i = int(a.argmax())
    r, c = divmod(i, a.shape[1])
    per_row, per_col = a.max(dim=1).values, a.max(dim=0).values
    top_r = [int(k) for k in per_row.argsort(descending=True)[:4]]
    top_c = [int(k) for k in per_col.argsort(descending=True)[:4]]
    name = lambda k, ids: int(ids[k]) if ids is not None else k
    return (f"largest at (row {name(r, rows)}, column {name(c, cols)}); worst rows {[name(k, rows) for k in top_r]}, "
            f"worst columns {[name(k, cols) for k in top_c]}; median row maximum {float(per_row.median()):.2e}, "
            f"median column maximum {float(per_col.median()):.2e}")


def residual(got, pn, N, full_limit, seed, full_fn, lines_fn):
    """max |got - f64| over the whole array (N <= full_limit) or the sampled rows and columns, and where it sits."""
    if N <= full_limit:
        d = got.cpu().to(S.C128) - full_fn()
        return float(d.abs().max()), _worst(d)
    q = S.sample_lines(pn, seed)
    qd = torch.as_tensor(q, device=got.device)
    R, C = lines_fn(q, q)
    dr = got[qd, :].cpu().to(S.C128) - R
    dc = got[:, qd].cpu().to(S.C128) - C
    er, ec = float(dr.abs().max()), float(dc.abs().max())
    return max(er, ec), "rows: " + _worst(dr, rows=q) + " | columns: " + _worst(dc, cols=q)


def spectrum_error(got, scaled, pn, N, seed):
    e, where = residual(got, pn, N, FULL_SPECTRUM, seed, lambda: S.spectrum_f64(scaled, pn, N),
                        lambda r, c: S.spectrum_lines_f64(scaled, pn, N, r, c))
    return e / S.fro(scaled), where


def hold(label, err, floor, where):
    """Print the error, the floor and their quotient; assert the quotient against the factor."""
    print(f"SPECTRUM-ROW | {label} | err_norm {err:.3e} | floor {floor:.3e} | quotient {err / floor:.2f}")
    assert err <= S.BOUND_FACTOR * floor, f"{label}: err_norm {err:.3e} is {err / floor:.2f} x the fp32 floor {floor:.3e}; {where}"


def make_input(entry, pn, seed):
    return S.pm1_mask(pn, seed) if entry == "int16" else S.complex_map(pn, seed)


# ---- every FFT size, both product ratios, both loaders -------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["int16", "complex"])
@pytest.mark.parametrize("ratio", ["half", "full"])
@pytest.mark.parametrize("log2n", range(4, 15))
def test_spectrum_every_size(L, dev, log2n, ratio, entry):
    N = 1 << log2n
    pn = N // 2 if ratio == "half" else N
    seed = S.case_seed(pn, N, entry == "complex")
    x = make_input(entry, pn, seed)
    got = gpu_spectrum(L, dev, x, RATIOS[ratio], N)
    scaled = S.scaled_image(x, RATIOS[ratio])
    del x
    err, where = spectrum_error(got, scaled, pn, N, seed)
    hold(f"forward N {N} pn {pn} eps {RATIOS[ratio]} ns {scaled.shape[0]} {entry}", err, S.FP32_CHAIN_FLOOR[N], where)


# ---- awkward shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["int16", "complex"])
@pytest.mark.parametrize("pn,N,eps", S.AWKWARD)
def test_spectrum_awkward_shapes(L, dev, pn, N, eps, entry):
    seed = S.case_seed(pn, N, entry == "complex") + int(eps * 10000)
    x = make_input(entry, pn, seed)
    got = gpu_spectrum(L, dev, x, eps, N)
    scaled = S.scaled_image(x, eps)
    err, where = spectrum_error(got, scaled, pn, N, seed)
    hold(f"awkward N {N} pn {pn} eps {eps} ns {scaled.shape[0]} {entry}", err, S.FP32_CHAIN_FLOOR[N], where)


# ---- the product's own masks, whole array --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product_cases():
    """(geometry, epsilon, N, scaled 0 / 1 image) of the four product masks, once for both tests."""
    cache = {}

    def get(kind, pn):
        if (kind, pn) not in cache:
            geo, eps, N = S.product_mask(kind, pn)
            cache[kind, pn] = (geo, eps, N, S.scaled_image(geo, eps))
        return cache[kind, pn]
    return get


@pytest.mark.parametrize("pn", [2048, 4096])
@pytest.mark.parametrize("kind", ["bern", "lines"])
def test_product_mask_spectrum_whole_array(L, dev, product_cases, kind, pn):
    """The 0 / 1 masks the headline numbers are measured on, every order (pn 4096: the sampled rows and columns) instead of the
    centre 64 x 64: the existing bound, 2e-6 of the largest order (DC)."""
    geo, eps, N, scaled = product_cases(kind, pn)
    mask = L.Mask(geo, PS, dev)
    assert mask.calculateEpsilonN(mask.deltaK, PS, WL) == (eps, N) and N == 2 * pn
    got = mask.fraunhofer(WL, True)
    dc = abs(complex(S.spectrum_rows_f64(scaled, pn, N, [pn // 2])[0, pn // 2]))
    assert dc == pytest.approx(float(scaled.double().sum()), rel=1e-12)
    e, where = residual(got, pn, N, FULL_SPECTRUM, 5, lambda: S.spectrum_f64(scaled, pn, N),
                        lambda r, c: S.spectrum_lines_f64(scaled, pn, N, r, c))
    print(f"product {kind} pn {pn} N {N}: max |d| / DC {e / dc:.2e} (err_norm {e / S.fro(scaled):.2e}); {where}")
    assert e / dc < 2e-6, where


@pytest.mark.parametrize("pn", [2048, 4096])
@pytest.mark.parametrize("kind", ["bern", "lines"])
def test_product_footprint_through_the_complex_entry(L, dev, product_cases, kind, pn):
    """The same footprints as geo - 0.5 through the complex loader.  Bernoulli - 0.5 is zero-mean: the bound of every other case.
    lines - 0.5 is not (mean -0.32): its floor is the reference chain's on that very input (FP32_CHAIN_FLOOR_LINES, where the
    arithmetic is written down), and it also meets 2e-6 of its largest order."""
    geo, eps, N, _ = product_cases(kind, pn)
    x = torch.complex(geo.to(torch.float32) - 0.5, torch.zeros(pn, pn))
    got = gpu_spectrum(L, dev, x, eps, N)
    scaled = S.scaled_image(x.real, eps)
    err, where = spectrum_error(got, scaled, pn, N, 6)
    floor = S.FP32_CHAIN_FLOOR_LINES[N] if kind == "lines" else S.FP32_CHAIN_FLOOR[N]
    hold(f"product {kind} - 0.5 N {N} pn {pn} complex", err, floor, where)
    if kind == "lines":
        dc = abs(float(scaled.double().sum()))
        print(f"product lines - 0.5 pn {pn}: max |d| / DC {err * S.fro(scaled) / dc:.2e}")
        assert err * S.fro(scaled) / dc < 2e-6


# ---- the inverse direction -----------------------------------------------------------------------------------------------
def gaussian(pn, seed, dev):
    """Seeded complex-Gaussian [pn, pn] of full support, made on the device (a 16384^2 pair costs the host 12 s)."""
    g = torch.Generator(device=dev).manual_seed(int(seed))
    return torch.complex(torch.randn(pn, pn, generator=g, device=dev), torch.randn(pn, pn, generator=g, device=dev))


@pytest.mark.parametrize("ratio", ["half", "full"])
@pytest.mark.parametrize("log2n", range(4, 15))
def test_field_every_size(L, dev, log2n, ratio):
    """calculateFFTAerial with a pupil and a mask spectrum of full pn x pn support at shift (0, 0): the whole input window, every
    output slot and the ragged or full last tile at the product's ratios.  max |dE| / ||A||_F, A = P M."""
    N = 1 << log2n
    pn = N // 2 if ratio == "half" else N
    seed = S.case_seed(pn, N, 2)
    P, M = gaussian(pn, seed, dev), gaussian(pn, seed + 1, dev)
    got = L.calculateFFTAerial(P, M, pn, N)
    torch.cuda.synchronize()
    sq = lambda z: z.real.double() ** 2 + z.imag.double() ** 2              # ||P M||_F, summed in float64 where the operands are
    norm = math.sqrt(sum(float((sq(p) * sq(m)).sum()) for p, m in zip(P.split(2048), M.split(2048))))
    A = (P.cpu(), M.cpu())                                                    # the product is taken in complex128, in blocks
    del P, M
    e, where = residual(got, pn, N, FULL_FIELD, seed, lambda: S.field_f64(A[0].to(S.C128) * A[1].to(S.C128), pn, N),
                        lambda r, c: S.field_lines_f64(A, pn, N, r, c))
    hold(f"inverse N {N} pn {pn} field", e / norm, S.FP32_CHAIN_FLOOR[N], where)


# ---- limits, through the C entry -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["int16", "complex"])
def test_limits_leave_the_output_alone(L, dev, entry):
    """A scaled image that does not fit the slab region (pn 16: 128 slabs of 1024 bytes = 131072 bytes; epsilon 40 makes
    ns = 640, 1.6 MB), epsilon 0 and NaN, an odd pn, N < pn: the error code, and not one byte of the output written."""
    from lithographysimulator_amd import _native as nat
    fn = nat.lib().litho_mask_spectrum_complex if entry == "complex" else nat.lib().litho_mask_spectrum
    ws = nat.workspace(dev, 16, 16)
    x = (S.complex_map(64, 1) if entry == "complex" else S.pm1_mask(64, 1)).to(dev)
    sentinel = complex(-7.25, 3.5)
    cases = [((16, 40.0, 16), nat.E_WORKSPACE), ((16, 0.0, 16), nat.E_ARG), ((16, float("nan"), 16), nat.E_ARG),
             ((15, 1.0, 16), nat.E_ARG), ((64, 1.0, 32), nat.E_NSMALL)]
    for (pn, eps, N), want in cases:
        out = torch.full((64, 64), sentinel, dtype=torch.complex64, device=dev)
        with torch.cuda.device(dev):
            rc = fn(nat.ptr(x), pn, eps, N, nat.ptr(out), nat.ptr(ws), ws.numel(), nat.stream_ptr(dev))
        torch.cuda.synchronize()
        assert rc == want, (pn, eps, N, rc)
        assert bool((out == sentinel).all()), (pn, eps, N)
    # and the largest epsilon that does fit at this size runs: ns * ns * bytes per sample <= 131072
    eps_fit = {"int16": 181 / 16, "complex": 128 / 16}[entry]                # ns = 181 (131044 bytes) | ns = 128 (131072 bytes)
    ns = int(math.floor(16 * eps_fit))
    assert ns * ns * (8 if entry == "complex" else 4) <= 131072 < (ns + 1) ** 2 * (8 if entry == "complex" else 4)
    small = make_input(entry, 16, 77)
    got = gpu_spectrum(L, dev, small, eps_fit, 16)
    scaled = S.scaled_image(small, eps_fit)
    err, where = spectrum_error(got, scaled, 16, 16, 0)
    hold(f"limit N 16 pn 16 eps {eps_fit:.4f} ns {ns} {entry}", err, S.FP32_CHAIN_FLOOR[16], where)
