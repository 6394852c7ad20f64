"""Vector (polarised, high-NA) Hopkins imaging on the GPU: litho_vector_pupils and litho_tcc_apply_vector (csrc/socs.hip),
vectorPupils / vectorSocsKernels / vectorAbbeIntensity (lithographysimulator_amd/vector.py) and the unchanged consumers of the
kernels they return.

Truth is tests/vector_oracle.py in float64 (pinned to the two-beam closed form and the scalar Abbe sum in test_vector_cpu.py).
Bounds: the six planes 2^-22 |want| per element (one fp32 rounding per component of a complex product, plus slack for the device's
double sincos); the operator 4 x the error of the same 14-transform formula in torch CPU complex64 (the rule of
test_gpu_socs.py); images helpers.TOL_IMAGE_MAX / TOL_IMAGE_L2 at full rank (K = the oracle's matrix_rank); truncated kernels
socs_oracle.TRUNCATION_RULE and TOL_EIG; gradients socs_grad_oracle's.  Every test prints what it observed (-s).

Measured on an MI355X: planes 5.2e-8 ... 5.9e-8 relative (bound 2.4e-7); operator 1.01 ... 1.35 of the complex64 formula's own
error (bound 4), in place, a second call and chunks of one vector equal bit for bit; full-rank images max 3.4e-7 ... 1.5e-6, l2
1.6e-7 ... 6.4e-7 (bounds 2e-5, 5e-6), captured within 3e-7 of 1; vectorAbbeIntensity 2.1e-7 ... 3.3e-7 max; truncated K 64 of 1140:
residual 1.149 lambda_65 (bound 1.5); gradient 2.3e-7 max.  Planes with cells exactly on alpha^2 + beta^2 = 1 (NA 0.72 / 1.44 at
pn 64, 0.5 / 1 at pn 32): 5.6e-8 ... 5.9e-8, the two boundary cells exact zeros, everything finite.  vectorAbbeIntensity on a
[3,6,pn,pn] stack 2.2e-7 ... 2.8e-7 max, 1.5e-7 ... 1.9e-7 l2 per plane (unpolarised and 45 degrees at degree 0.5), plane 1 equal bit
for bit to the unstacked call; "y" 1.9e-7 max, 0.136 of the maximum (6,800 x the tolerance) away from "x"; with a PlanCache the
second call, the call after a change of polarisation and the call after Qd.mul_(0.5) equal the calls without a plan bit for
bit, the last exactly a quarter of the one before.  Polarisation as a pair of maps (vector_oracle.twisted_maps, degree 0.7):
K 30, max 5.3e-7, l2 3.7e-7, captured within 3e-7 of 1.  The operator at every size class and with walking batches:
test_gpu_vector_sizes.py.  The whole file takes six seconds."""
import ctypes

import numpy as np
import pytest
import torch

import opc_case as C
import socs_grad_oracle as GO
import socs_oracle as SO
import vector_oracle as VO
from helpers import DEMO_AB, NA, PS, TOL_IMAGE_L2, TOL_IMAGE_MAX, WL, f16, rel_l2, rel_max
from oracle import abbe_oracle as O

pytestmark = pytest.mark.gpu
WATER = (1.35, 1.44)


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


def _check(tag, got, want):
    e_max, e_l2 = rel_max(got.cpu(), want), rel_l2(got.cpu(), want)
    print(f"{tag}: max {e_max:.2e} (bound {TOL_IMAGE_MAX:.0e}), l2 {e_l2:.2e} (bound {TOL_IMAGE_L2:.0e})")
    assert e_max < TOL_IMAGE_MAX and e_l2 < TOL_IMAGE_L2, (tag, e_max, e_l2)


# ---- 1. litho_vector_pupils ------------------------------------------------------------------------------------------------------
def _planes_check(tag, got, want):
    got, want = got.cpu().numpy().astype(np.complex128), np.asarray(want)
    excess = np.abs(got - want) - 2.0 ** -22 * np.abs(want)
    worst = float((np.abs(got - want)[want != 0] / np.abs(want)[want != 0]).max())
    zeros = int((want == 0).sum())
    print(f"{tag}: worst relative error {worst:.2e} (bound {2.0 ** -22:.2e}), {zeros} exact zeros of {want.size}")
    assert (excess <= 0).all(), (tag, float(excess.max()))
    assert not got[want == 0].any(), tag


@pytest.mark.parametrize("pn", [16, 30, 64])
def test_vector_pupils_against_the_oracle(L, nat, dev, pn):
    """One workgroup (16), an even size that is no multiple of the block or of anything else (30), 64; demo aberrations and a
    random pupil that is non-zero everywhere (so the zeroing beyond alpha^2 + beta^2 = 1 shows); one plane, and three with defocus."""
    g = torch.Generator().manual_seed(pn)
    pupils = {"demo": O.pupil_function(f16(DEMO_AB), pn, NA, WL).to(torch.complex64),
              "random": torch.view_as_complex(torch.randn((pn, pn, 2), generator=g, dtype=torch.float32) + 0.1)}
    zs = (-100.0, 0.0, 100.0)
    for name, P in pupils.items():
        p = P.numpy().astype(np.complex128)
        for na, n in VO.OPTICS:
            for rad in (False, True):
                got = L.vectorPupils(P.to(dev), na, n, rad)
                assert got.dtype == torch.complex64 and tuple(got.shape) == (6, pn, pn)
                _planes_check(f"pn {pn} {name} NA {na} n {n} radiometric {rad}", got, VO.vector_pupils(p, na, n, rad))
                stack = L.vectorPupils(P.to(dev), na, n, rad, defocus=list(zs), wavelength=WL)
                assert tuple(stack.shape) == (3, 6, pn, pn)
                for i, z in enumerate(zs):
                    _planes_check(f"pn {pn} {name} NA {na} n {n} radiometric {rad} z {z:+.0f}", stack[i],
                                  VO.vector_pupils(p, na, n, rad, z, WL))
    if pn == 64:
        inside = VO.cosines(pn, 0.7, 1.0)[3]
        assert (~inside).any() and bool((pupils["random"] != 0).all())
    # a pupil stack with one defocus value per plane
    two = torch.stack([pupils["demo"], pupils["random"]]).to(dev)
    got = L.vectorPupils(two, *WATER, True, defocus=[50.0, -30.0], wavelength=WL)
    for i, (name, z) in enumerate((("demo", 50.0), ("random", -30.0))):
        _planes_check(f"pn {pn} stack plane {i}", got[i], VO.vector_pupils(pupils[name].numpy().astype(np.complex128), *WATER, True, z, WL))


@pytest.mark.parametrize("na,n,pn", [(0.72, 1.44, 64), (0.5, 1.0, 32)])
def test_vector_pupils_on_the_evanescent_boundary(L, dev, na, n, pn):
    """Two further cases of the test above, kept apart because their optics are not VO.OPTICS: NA sigma / n is exactly +-1 at
    the grid edge (0.72 . 2 = 1.44 exactly in binary64), so alpha^2 + beta^2 is exactly 1.0 at cells (pn/2, 0) and (0, pn/2),
    where `!(s < 1.0)` decides between an exact zero and 1 / sqrt(0).  The smallest gamma inside is 0.054 and 0.153, so
    1 / sqrt(gamma) stays below 4.4 and the bound of _planes_check holds unchanged.
    Only these exactly representable cases: NA 0.8, n 1.0, pn 64 puts 8 further cells within 1e-12 of the boundary, where the
    compiler's contraction of a*a + b*b may legitimately classify a cell differently from numpy -- a test of rounding, not of
    the kernel."""
    a, b, gamma, inside = VO.cosines(pn, na, n)
    on = (a * a + b * b) == 1.0
    assert int(on.sum()) == 2 and bool(on[pn // 2, 0]) and bool(on[0, pn // 2]) and not inside[on].any()
    print(f"NA {na} n {n} pn {pn}: 2 cells with alpha^2 + beta^2 == 1.0 exactly, smallest gamma inside {gamma[inside].min():.3f}")
    g = torch.Generator().manual_seed(pn)
    P = torch.view_as_complex(torch.randn((pn, pn, 2), generator=g, dtype=torch.float32) + 0.1)
    assert bool((P != 0).all())
    p = P.numpy().astype(np.complex128)
    for rad in (False, True):
        got = L.vectorPupils(P.to(dev), na, n, rad)
        assert bool(torch.isfinite(torch.view_as_real(got)).all())
        assert not got.cpu()[:, torch.from_numpy(on)].any()                                          # exact zeros, all six planes
        _planes_check(f"pn {pn} random NA {na} n {n} radiometric {rad}", got, VO.vector_pupils(p, na, n, rad))
        stack = L.vectorPupils(P.to(dev), na, n, rad, defocus=[-100.0, 100.0], wavelength=WL)
        assert bool(torch.isfinite(torch.view_as_real(stack)).all()) and not stack.cpu()[:, :, torch.from_numpy(on)].any()
        for i, z in enumerate((-100.0, 100.0)):
            _planes_check(f"pn {pn} random NA {na} n {n} radiometric {rad} z {z:+.0f}", stack[i], VO.vector_pupils(p, na, n, rad, z, WL))


def test_vector_pupils_argument_errors(nat, dev):
    pn = 16
    P = torch.ones((pn, pn), dtype=torch.complex64, device=dev)
    out = torch.full((6, pn, pn), 7.0, dtype=torch.complex64, device=dev)
    f, st = nat.lib().litho_vector_pupils, nat.stream_ptr(dev)
    assert f(nat.ptr(P), 1, pn, 1.44, 1.44, 0, None, 0.0, nat.ptr(out), st) == nat.E_ARG          # NA >= index
    assert f(nat.ptr(P), 1, pn, 1.5, 1.44, 0, None, 0.0, nat.ptr(out), st) == nat.E_ARG
    assert f(nat.ptr(P), 0, pn, 0.7, 1.0, 0, None, 0.0, nat.ptr(out), st) == nat.E_ARG            # planes < 1
    assert f(None, 1, pn, 0.7, 1.0, 0, None, 0.0, nat.ptr(out), st) == nat.E_ARG
    assert f(nat.ptr(P), 1, pn, 0.7, 1.0, 0, None, 0.0, None, st) == nat.E_ARG
    assert f(nat.ptr(P), 1, 15, 0.7, 1.0, 0, None, 0.0, nat.ptr(out), st) == nat.E_ARG            # odd
    assert f(nat.ptr(P), 1, 14, 0.7, 1.0, 0, None, 0.0, nat.ptr(out), st) == nat.E_ARG            # < 16
    z = (ctypes.c_double * 1)(float("nan"))
    assert f(nat.ptr(P), 1, pn, 0.7, 1.0, 0, z, WL, nat.ptr(out), st) == nat.E_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                             # a refused call writes nothing


# ---- 2. litho_tcc_apply_vector ---------------------------------------------------------------------------------------------------
_formula64 = VO.formula64        # the floor of the bound, shared with test_gpu_vector_sizes.py


def _device_apply(nat, dev, qh, wsh, X, Y, work=None, work_bytes=None):
    batch, n = X.shape[0], X.shape[-1]
    need = int(nat.lib().litho_tcc_apply_vector_work_bytes(batch, n))
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = nat.lib().litho_tcc_apply_vector(nat.ptr(qh), nat.ptr(wsh), nat.ptr(X), nat.ptr(Y), batch, n, nat.ptr(work),
                                          need if work_bytes is None else work_bytes, nat.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc


def _spectra(nat, dev, Q):
    qh = Q.to(dev).clone()
    nat.check(nat.lib().litho_fft2_c2c(nat.ptr(qh), 6, Q.shape[-1], 0, nat.stream_ptr(dev)), "litho_fft2_c2c")
    return qh


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("mode", ["te", "unpolarized"])
@pytest.mark.parametrize("name,batch", [("wrap32", 3), ("focus64", 2)])
def test_tcc_apply_vector_against_the_explicit_operator(L, nat, dev, name, batch, mode):
    from lithographysimulator_amd.vector import _VectorOperator
    P, W, M, N = SO.problem(name)
    pn = P.shape[0]
    Q = torch.from_numpy(VO.vector_pupils(P.numpy(), *WATER, True)).to(torch.complex64)
    maps = L.sourcePolarization(W, mode)
    g = torch.Generator().manual_seed(7)
    X = torch.view_as_complex(torch.randn((batch, pn, pn, 2), generator=g, dtype=torch.float32))
    A = VO.explicit_rows(Q.numpy(), W.numpy(), mode)
    x = X.numpy().astype(np.complex128).reshape(batch, -1)
    want = (A.T @ (A.conj() @ x.T)).T.reshape(batch, pn, pn)
    floor = _rel(_formula64(Q, maps, X), want)
    qh, wsh = _spectra(nat, dev, Q), torch.fft.ifftshift(maps, dim=(-2, -1)).contiguous().to(dev)
    Xd = X.to(dev)
    out = torch.empty_like(Xd)
    assert _device_apply(nat, dev, qh, wsh, Xd, out) == 0
    assert torch.equal(Xd.cpu(), X)                                            # out of place leaves X alone
    e_out = _rel(out.cpu().numpy(), want)
    again = torch.empty_like(Xd)
    assert _device_apply(nat, dev, qh, wsh, Xd, again) == 0
    chunked = _VectorOperator(Q.to(dev), wsh, 1)(Xd)                           # applyBytes 1: chunks of one vector
    torch.cuda.synchronize()
    inplace = Xd.clone()
    assert _device_apply(nat, dev, qh, wsh, inplace, inplace) == 0
    print(f"{name} batch {batch} {mode}: rows {A.shape[0]}, error {e_out:.3e}, complex64 floor {floor:.3e}, quotient "
          f"{e_out / floor:.2f} (bound 4); in place {'==' if torch.equal(inplace, out) else '!='} out of place, second call "
          f"{'==' if torch.equal(again, out) else '!='} first, chunks of one {'==' if torch.equal(chunked, out) else '!='} one call")
    assert e_out <= 4 * floor
    assert torch.equal(inplace, out) and torch.equal(again, out) and torch.equal(chunked, out)
    # overlapping but distinct buffers are refused, and so is a work buffer one byte short; neither writes anything
    both = torch.zeros((batch + 1, pn, pn), dtype=torch.complex64, device=dev)
    assert _device_apply(nat, dev, qh, wsh, both[:batch], both[1:]) == nat.E_ARG
    need = int(nat.lib().litho_tcc_apply_vector_work_bytes(batch, pn))
    assert need == 48 * (batch + 1) * pn * pn
    keep = torch.full_like(Xd, 3.0)
    assert _device_apply(nat, dev, qh, wsh, Xd, keep, work_bytes=need - 1) == nat.E_WORKSPACE
    assert bool((keep == 3.0).all()) and int(torch.count_nonzero(torch.view_as_real(both))) == 0


@pytest.mark.parametrize("n", [16, 1024])
def test_tcc_apply_vector_at_the_smallest_and_a_multi_pass_size(nat, dev, n):
    Q, maps, X = VO.random_setting(n)
    want = VO.fft_apply(Q.numpy(), maps.numpy(), X.numpy())
    floor = _rel(_formula64(Q, maps, X), want)
    moved = _rel(VO.fft_apply(Q.numpy().transpose(0, 2, 1), maps.numpy(), X.numpy()), want)        # the inputs can tell a transpose
    swapped = _rel(VO.fft_apply(Q.numpy()[[1, 0, 3, 2, 5, 4]], maps.numpy(), X.numpy()), want)      # and an exchange of j
    assert moved > 400 * floor and swapped > 400 * floor
    qh, wsh = _spectra(nat, dev, Q), torch.fft.ifftshift(maps, dim=(-2, -1)).contiguous().to(dev)
    out = torch.empty_like(X, device=dev)
    assert _device_apply(nat, dev, qh, wsh, X.to(dev), out) == 0
    e = _rel(out.cpu().numpy(), want)
    print(f"n {n}: error {e:.3e}, complex64 floor {floor:.3e}, quotient {e / floor:.2f} (bound 4); truth moves by {moved:.2e} under "
          f"Q^T and {swapped:.2e} under an exchange of the polarisation index")
    assert e <= 4 * floor


def test_tcc_apply_vector_refusals(nat, dev):
    n = 16
    qh = torch.zeros((6, n, n), dtype=torch.complex64, device=dev)
    w = torch.zeros((3, n, n), dtype=torch.float32, device=dev)
    X = torch.ones((1, n, n), dtype=torch.complex64, device=dev)
    Y = torch.full((1, n, n), 2.0, dtype=torch.complex64, device=dev)
    lib, st = nat.lib(), nat.stream_ptr(dev)
    work = torch.zeros(int(lib.litho_tcc_apply_vector_work_bytes(1, n)), dtype=torch.uint8, device=dev)
    f = lib.litho_tcc_apply_vector
    args = [nat.ptr(qh), nat.ptr(w), nat.ptr(X), nat.ptr(Y), 1, n, nat.ptr(work), work.numel(), st]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (6, None), (4, 0), (5, 8), (5, 24), (5, 8192)):
        a = list(args)
        a[i] = bad
        assert f(*a) == nat.E_ARG, (i, bad)
    a = list(args)
    a[4] = (1 << 20) + 1                                                       # one vector more than the entry takes
    assert f(*a) == nat.E_ARG
    for batch, size in ((0, n), (1, 8), (1, 48), (1, 8192), ((1 << 20) + 1, n)):
        assert lib.litho_tcc_apply_vector_work_bytes(batch, size) == 0
    torch.cuda.synchronize()
    assert bool((X == 1).all()) and bool((Y == 2).all()) and not work.any()


# ---- 3. full-rank parity ----------------------------------------------------------------------------------------------------------
_kernels = {}


def _full_rank(L, dev, key, P, W, optics, mode, degree, radiometric=False):
    """(SOCSKernels at K = the oracle's matrix_rank with oversample 0, the float64 planes, the rank); made once per key."""
    if key not in _kernels:
        Q = VO.vector_pupils(P.numpy(), *optics, radiometric)
        rank = VO.rank_of(Q, W.numpy(), mode, degree)
        k = L.vectorSocsKernels(P.to(dev), W.to(dev), optics[0], polarization=mode, degree=degree, mediumIndex=optics[1],
                                radiometric=radiometric, kernels=rank, oversample=0)
        _kernels[key] = (k, Q, rank)
    return _kernels[key]


def _outside_box_is_zero(k, pn):
    if k.boxes[0] is None:
        return None
    r_lo, r_hi, c_lo, c_hi = k.boxes[0]
    outside = torch.ones((pn, pn), dtype=torch.bool, device=k.kernels.device)
    outside[r_lo:r_hi + 1, c_lo:c_hi + 1] = False
    return int((k.kernels[:, outside] != 0).sum()) == 0 and bool(outside.any())


@pytest.mark.parametrize("mode,degree", [("x", 1.0), ("te", 1.0), ("tm", 1.0), ("unpolarized", 1.0), ("te", 0.5)])
@pytest.mark.parametrize("optics", VO.OPTICS)
def test_full_rank_parity_six_points(L, dev, optics, mode, degree):
    P, W, M, N = VO.six_points()
    k, Q, rank = _full_rank(L, dev, ("six", optics, mode, degree), P, W, optics, mode, degree)
    pure = mode != "unpolarized" and degree == 1.0
    assert k.K == rank == (3 if pure else 5) * 6 and k.lit_points == 6
    got = L.hopkinsIntensity(M.to(dev), k, N)
    zero = _outside_box_is_zero(k, 32)
    print(f"NA {optics[0]} n {optics[1]} {mode} degree {degree}: K {rank}, captured {k.captured:.8f}, box {k.boxes[0]}, zeros outside {zero}")
    _check("  hopkins vs float64 vector Abbe", got, VO.abbe_truth(Q, M, W.numpy(), mode, degree, N))
    assert abs(k.captured - 1.0) < 1e-5 and zero is not False


def test_full_rank_parity_with_a_wrapping_source(L, dev):
    """wrap32: S = 92, the source wraps the pupil around the grid (no box), TE, radiometric, K = 276."""
    P, W, M, N = SO.problem("wrap32")
    k, Q, rank = _full_rank(L, dev, "wrap32", P, W, WATER, "te", 1.0, True)
    assert k.K == rank == 276 and k.boxes == [None]
    print(f"wrap32 te: K {rank}, captured {k.captured:.8f}")
    _check("  hopkins vs float64 vector Abbe", L.hopkinsIntensity(M.to(dev), k, N), VO.abbe_truth(Q, M, W.numpy(), "te", 1.0, N))
    assert abs(k.captured - 1.0) < 1e-5


def test_full_rank_parity_at_n_equal_4_pn(L, dev, nat):
    """(pn, N) = (64, 256), TM, 40 strided points of the annular 0.4-0.8 source with grey weights."""
    from lithographysimulator_amd.synthetic import bernoulli_mask
    pn, N = 64, 256
    P = O.pupil_function(f16(DEMO_AB), pn, NA, WL)
    W = SO.grey_weights(SO.strided_points(O.source_annular(0.4, 0.8, pn), 40))
    M = O.mask_spectrum(bernoulli_mask(pn), PS, WL)
    k, Q, rank = _full_rank(L, dev, "n4pn", P, W, WATER, "tm", 1.0)
    assert k.K == rank == 120
    got = L.hopkinsIntensity(M.to(dev), k, N)
    zero = _outside_box_is_zero(k, pn)
    print(f"pn 64 N 256 tm: K {rank}, captured {k.captured:.8f}, box {k.boxes[0]}, zeros outside {zero}, plan {nat.last_plan()}")
    _check("  hopkins vs float64 vector Abbe", got, VO.abbe_truth(Q, M, W.numpy(), "tm", 1.0, N))
    assert abs(k.captured - 1.0) < 1e-5 and zero is not False


# ---- 4. vectorAbbeIntensity -------------------------------------------------------------------------------------------------------
_strided = {}


def _strided_problem(L, dev, pn, N):
    """The `_strided_problem` recipe of test_gpu_socs.py: Bernoulli mask spectrum, demo pupil, 40 strided points of the annular
    0.4-0.8 list with weights in (0, 2], as a list and as a weight map."""
    if (pn, N) not in _strided:
        from lithographysimulator_amd.synthetic import bernoulli_mask
        mft = L.Mask(bernoulli_mask(pn), PS, dev).fraunhofer(WL, True)
        pf = L.Pupil(pn, WL, NA, f16(DEMO_AB), dev).generatePupilFunction()
        sh = L.sourceShifts(L.LightSource(0.4, 0.8, pn, NA, device=dev).generateAnnular(), pn)
        sel = sh[(torch.arange(40, device=dev) * sh.shape[0]) // 40].contiguous()
        g = torch.Generator().manual_seed(5)
        w = (2.0 * (1.0 - torch.rand(40, generator=g, dtype=torch.float64))).to(torch.float32).to(dev)
        W = torch.zeros((pn, pn), dtype=torch.float32, device=dev)
        W[(sel[:, 0] + pn // 2).long(), (sel[:, 1] + pn // 2).long()] = w
        _strided[(pn, N)] = (mft, pf, sel, w, W)
    return _strided[(pn, N)]


@pytest.mark.parametrize("pn,N", [(32, 64), (128, 256)])
def test_vector_abbe_intensity(L, dev, pn, N):
    mft, pf, sel, w, W = _strided_problem(L, dev, pn, N)
    Qd = L.vectorPupils(pf, *WATER, True)
    Q = VO.vector_pupils(pf.cpu().numpy(), *WATER, True)
    images = {}
    for mode in ("x", "unpolarized"):
        images[mode] = L.vectorAbbeIntensity(mft, Qd, sel, N, polarization=mode, weights=w)
        _check(f"pn {pn} N {N} {mode}: vectorAbbeIntensity vs float64 truth", images[mode],
               VO.abbe_truth(Q, mft.cpu(), W.cpu().numpy(), mode, 1.0, N))
    half = L.vectorAbbeIntensity(mft, Qd, sel, N, polarization=(1.0, 1.0), degree=0.5, weights=w)
    _check(f"pn {pn} N {N} 45 degrees at degree 0.5: vectorAbbeIntensity vs float64 truth", half,
           VO.abbe_truth(Q, mft.cpu(), W.cpu().numpy(), (1.0, 1.0), 0.5, N))
    acc = torch.ones_like(images["x"])
    assert L.vectorAbbeIntensity(mft, Qd, sel, N, polarization="x", weights=w, out=acc) is acc
    assert rel_max(acc - 1.0, images["x"]) < 1e-5
    # weights=None with a bitmap source: every lit point with weight 1
    bitmap = (W > 0)
    sh = L.sourceShifts(bitmap, pn)
    plain = L.vectorAbbeIntensity(mft, Qd, sh, N, polarization="unpolarized")
    _check(f"pn {pn} N {N} unpolarized, bitmap source", plain,
           VO.abbe_truth(Q, mft.cpu(), bitmap.cpu().numpy().astype(np.float64), "unpolarized", 1.0, N))
    if pn == 32:
        for mode in ("x", "unpolarized"):
            k, _, rank = _full_rank(L, dev, ("strided32", mode), pf.cpu(), W.cpu(), WATER, mode, 1.0, True)
            hop = L.hopkinsIntensity(mft, k, N)
            print(f"  {mode}: full-rank Hopkins K {rank}, captured {k.captured:.8f}")
            _check(f"  {mode}: full-rank Hopkins vs vectorAbbeIntensity", hop, images[mode].cpu().double())


def test_vector_abbe_intensity_plane_stack(L, dev):
    """vectorPupils [3,6,pn,pn] through vectorAbbeIntensity: planes x 3 (pure) or planes x 6 (mixed) effective pupils reach
    litho_socs_fold in the group-major order [planes, states, 3]."""
    pn, N = 32, 64
    mft, pf, sel, w, W = _strided_problem(L, dev, pn, N)
    zs = [-100.0, 0.0, 100.0]
    Qd = L.vectorPupils(pf, *WATER, True, defocus=zs, wavelength=WL)
    assert tuple(Qd.shape) == (3, 6, pn, pn)
    flat = L.vectorPupils(pf, *WATER, True)
    assert torch.equal(Qd[1], flat)                                            # z = 0: the phase factor is exactly 1
    Qs = [VO.vector_pupils(pf.cpu().numpy(), *WATER, True, z, WL) for z in zs]
    for mode, degree in (("unpolarized", 1.0), ((1.0, 1.0), 0.5)):
        got = L.vectorAbbeIntensity(mft, Qd, sel, N, polarization=mode, degree=degree, weights=w)
        assert tuple(got.shape) == (3, pn, pn)
        for i, z in enumerate(zs):
            _check(f"stack {mode} degree {degree} plane {i} z {z:+.0f}: vectorAbbeIntensity vs float64 truth", got[i],
                   VO.abbe_truth(Qs[i], mft.cpu(), W.cpu().numpy(), mode, degree, N))
        # The effective pupils of plane 1 are the same bits as those of the unstacked call, and every plane's fp32 sum runs
        # over the source points in list order; only a launch plan that splits the 18 items of the stack differently from the
        # 6 of the single plane could reorder that sum, and then by roundings of the sum alone.
        single = L.vectorAbbeIntensity(mft, flat, sel, N, polarization=mode, degree=degree, weights=w)
        same, e = torch.equal(got[1], single), rel_max(got[1], single)
        print(f"stack {mode} degree {degree}: plane 1 {'==' if same else '!='} the unstacked call at z = 0 (max {e:.2e})")
        assert same or e <= 1e-6
        acc = torch.ones_like(got)
        assert L.vectorAbbeIntensity(mft, Qd, sel, N, polarization=mode, degree=degree, weights=w, out=acc) is acc
        assert rel_max(acc - 1.0, got) < 1e-5


def test_vector_abbe_intensity_y(L, dev):
    pn, N = 32, 64
    mft, pf, sel, w, W = _strided_problem(L, dev, pn, N)
    Qd = L.vectorPupils(pf, *WATER, True)
    Q = VO.vector_pupils(pf.cpu().numpy(), *WATER, True)
    y = L.vectorAbbeIntensity(mft, Qd, sel, N, polarization="y", weights=w)
    _check("y: vectorAbbeIntensity vs float64 truth", y, VO.abbe_truth(Q, mft.cpu(), W.cpu().numpy(), "y", 1.0, N))
    x = L.vectorAbbeIntensity(mft, Qd, sel, N, polarization="x", weights=w)
    apart = rel_max(y, x)
    print(f"y differs from x by {apart:.2e} of the maximum ({apart / TOL_IMAGE_MAX:.0f} x the tolerance)")
    assert apart > 100 * TOL_IMAGE_MAX                                          # a swapped index cannot pass


def test_vector_abbe_intensity_with_a_plan(L, dev):
    """One PlanCache: the effective-pupil stack is kept while (data_ptr, _version, shape, states) stay, and rebuilt when the
    polarisation changes or the planes are written in place."""
    pn, N = 32, 64
    mft, pf, sel, w, W = _strided_problem(L, dev, pn, N)
    Qd = L.vectorPupils(pf, *WATER, True)
    Q = VO.vector_pupils(pf.cpu().numpy(), *WATER, True)
    truth = {m: VO.abbe_truth(Q, mft.cpu(), W.cpu().numpy(), m, 1.0, N) for m in ("x", "y")}
    plan = L.PlanCache()
    first = L.vectorAbbeIntensity(mft, Qd, sel, N, polarization="x", weights=w, plan=plan)
    kept = plan._vector_stack[1]
    second = L.vectorAbbeIntensity(mft, Qd, sel, N, polarization="x", weights=w, plan=plan)
    assert torch.equal(first, second) and plan._vector_stack[1] is kept
    _check("plan, x: vs float64 truth", first, truth["x"])
    other = L.vectorAbbeIntensity(mft, Qd, sel, N, polarization="y", weights=w, plan=plan)       # same shape, other states
    assert plan._vector_stack[1] is not kept
    _check("plan, then y with the same cache: vs float64 truth", other, truth["y"])
    free = {"x": L.vectorAbbeIntensity(mft, Qd, sel, N, polarization="x", weights=w),
            "y": L.vectorAbbeIntensity(mft, Qd, sel, N, polarization="y", weights=w)}
    version, kept = Qd._version, plan._vector_stack[1]
    Qd.mul_(0.5)                                                               # same address and shape, _version moves
    assert Qd._version != version
    scaled = L.vectorAbbeIntensity(mft, Qd, sel, N, polarization="y", weights=w, plan=plan)
    assert plan._vector_stack[1] is not kept
    _check("plan, y after Qd.mul_(0.5): a quarter of the earlier image", scaled, other.cpu().double() / 4)
    _check("plan, y after Qd.mul_(0.5): vs float64 truth / 4", scaled, truth["y"] / 4)
    free_scaled = L.vectorAbbeIntensity(mft, Qd, sel, N, polarization="y", weights=w)
    for tag, a, b in (("first", first, free["x"]), ("second", second, free["x"]), ("other polarisation", other, free["y"]),
                      ("scaled", scaled, free_scaled)):
        _check(f"plan, {tag}: vs the call without a plan", a, b.cpu().double())


# ---- 4b. polarisation given as a pair of maps ---------------------------------------------------------------------------------------
def test_full_rank_parity_with_polarisation_maps(L, dev):
    """vector_oracle.twisted_maps on the six points: angle 2 phi + 0.3, un-normalised lengths, degree 0.7 -- a mixed state that
    no named mode expresses, imaged through the kernels and compared with the float64 vector Abbe sum."""
    P, W, M, N = VO.six_points()
    ex, ey = VO.twisted_maps(32)
    k, Q, rank = _full_rank(L, dev, ("six", WATER, "maps", 0.7), P, W, WATER, (ex, ey), 0.7)
    assert k.K == rank == 30 and k.lit_points == 6
    got = L.hopkinsIntensity(M.to(dev), k, N)
    print(f"map pair degree 0.7: K {rank}, captured {k.captured:.8f}, box {k.boxes[0]}")
    _check("  hopkins vs float64 vector Abbe", got, VO.abbe_truth(Q, M, W.numpy(), (ex, ey), 0.7, N))
    assert abs(k.captured - 1.0) < 1e-5


# ---- 5. through focus -------------------------------------------------------------------------------------------------------------
def test_through_focus_stack(L, dev):
    P, W, M, N = VO.six_points()
    zs = [-100.0, 0.0, 100.0]
    rank = 18
    k = L.vectorSocsKernels(P.to(dev), W.to(dev), WATER[0], polarization="te", mediumIndex=WATER[1], defocus=zs, wavelength=WL,
                            kernels=rank, oversample=0)
    assert tuple(k.kernels.shape) == (3, rank, 32, 32) and k.planes == 3 and k.stacked
    got = L.hopkinsIntensity(M.to(dev), k, N)
    assert tuple(got.shape) == (3, 32, 32)
    for i, z in enumerate(zs):
        Q = VO.vector_pupils(P.numpy(), *WATER, False, z, WL)
        assert VO.rank_of(Q, W.numpy(), "te") == rank
        _check(f"plane {i} z {z:+.0f}", got[i], VO.abbe_truth(Q, M, W.numpy(), "te", 1.0, N))
    flat, _, _ = _full_rank(L, dev, ("six", WATER, "te", 1.0), P, W, WATER, "te", 1.0)
    _check("plane z = 0 vs the unstacked kernels", got[1], L.hopkinsIntensity(M.to(dev), flat, N).cpu().double())
    assert float((k.captured - 1.0).abs().max()) < 1e-5


# ---- 6. truncated -----------------------------------------------------------------------------------------------------------------
def test_truncated_kernels(L, dev):
    """pn 64, ideal pupil, annular 0.4-0.8 (S = 380), TE at NA 1.35 in water: 64 kernels of a rank-1140 operator."""
    P, W = SO.truncated_setting("a")
    K = 64
    Q = VO.vector_pupils(P.numpy(), *WATER)
    A = VO.explicit_rows(Q, W.numpy(), "te")
    lam = np.linalg.eigvalsh(A @ A.conj().T)[::-1]
    k = L.vectorSocsKernels(P.to(dev), W.to(dev), WATER[0], polarization="te", mediumIndex=WATER[1], kernels=K)
    theta = k.eigenvalues.numpy()
    res = SO.residual_norm(A, k.kernels.cpu().numpy())
    excess = float((theta - lam[:K]).max() / lam[0])
    tr = VO.trace(Q, VO.weight_maps(W.numpy(), "te"))
    print(f"S 380, rows {A.shape[0]}, K {K}: residual / lambda_K+1 {res / lam[K]:.4f} (bound {SO.TRUNCATION_RULE}); theta - lambda max "
          f"{excess:+.2e} lambda_1 (bound {SO.TOL_EIG:.0e}); captured {k.captured:.6f}, exact {lam[:K].sum() / tr:.6f}; trace "
          f"{k.trace:.4f} (oracle {tr:.4f})")
    assert k.K == K and A.shape[0] == 1140
    assert res <= SO.TRUNCATION_RULE * lam[K]
    assert (np.diff(theta) <= 0).all() and (theta >= 0).all() and excess <= SO.TOL_EIG
    assert abs(k.trace - tr) <= 1e-6 * tr and abs(k.captured - theta.sum() / k.trace) <= 1e-12


# ---- 7. the consumers are unchanged -----------------------------------------------------------------------------------------------
def test_gradient_through_vector_kernels(L, dev):
    P, W, M, N = VO.six_points()
    k, _, _ = _full_rank(L, dev, ("six", WATER, "te", 1.0), P, W, WATER, "te", 1.0)
    G = GO.random_G((32, 32), 9)
    got = L.hopkinsGradient(M.to(dev), k, N, G.to(dev)).cpu().to(torch.complex128)
    want = GO.gradient(k.kernels.cpu(), M, N, G)
    e_max, e_l2 = float((got - want).abs().max() / want.abs().max()), float(torch.linalg.norm(got - want) / torch.linalg.norm(want))
    print(f"gradient through 18 TE kernels: max {e_max:.2e} (bound {GO.TOL_GRAD_MAX:.0e}), l2 {e_l2:.2e} (bound {GO.TOL_GRAD_L2:.0e})")
    assert e_max < GO.TOL_GRAD_MAX and e_l2 < GO.TOL_GRAD_L2


def test_correct_layout_takes_given_kernels(L, dev, golden):
    """One iteration of the correction loop on tests/opc_case.py through 16 TE kernels at NA 1.2 in water: it runs and measures a
    finite EPE.  Nothing is asserted about the values."""
    pupil = L.Pupil(C.PN, C.WAVELENGTH, C.NA, None, device=dev).generatePupilFunction()
    source = L.LightSource(C.SIGMA_IN, C.SIGMA_OUT, C.PN, C.NA, device=dev).generateAnnular()
    k = L.vectorSocsKernels(pupil, source, 1.2, polarization="te", mediumIndex=1.44, kernels=16)
    res = L.correctLayout(C.layout(), C.PN, C.PIXEL, C.ORIGIN, C.WAVELENGTH, pupil, source, float(golden("g19_opc_loop.npz")["threshold"]),
                          spacing=C.SPACING, iterations=1, gain=C.GAIN, maxBias=C.MAX_BIAS, antialias=C.ANTIALIAS,
                          searchRange=C.RANGE, model="socs", socs=k)
    rms, worst, lost = res.history[0]
    print(f"correctLayout(socs=): K {k.K}, captured {k.captured:.4f}, history {res.history}")
    assert isinstance(res, L.OPCResult) and len(res.history) == 1 and np.isfinite(rms) and np.isfinite(worst)
