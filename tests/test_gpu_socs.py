"""Hopkins imaging on the GPU: litho_tcc_apply and litho_socs_fold (csrc/socs.hip), socsKernels / hopkinsIntensity / hopkinsImage
and correctLayout(model="socs").

Truth for the operator is the explicit transmission cross coefficient of tests/socs_oracle.py (float64), bounded by 4 x the error
of the same formula in torch's CPU complex64; truth for every image is the reference's mathematics in float64, the weighted Abbe
sum through oracle.field_closed_form, under the project's TOL_IMAGE_MAX / TOL_IMAGE_L2 -- at FULL rank (K = the number of lit
points), where Hopkins and Abbe are the same sum.  The fold is checked bit for bit.  Every test prints what it observed (-s).

Measured on an MI355X: litho_tcc_apply 1.22 (pn 32) and 1.18 (pn 64) of the complex64 formula's own error (bound 4), in place equal
to out of place bit for bit; full-rank images max 5.1e-7 ... 8.7e-7 and l2 2.5e-7 ... 4.0e-7 of the float64 Abbe sum in the five
cases (bounds 2e-5 and 5e-6); chunked folds identical bit for bit; K = 24 of 92: 1.06 x the exact truncation's error (bound 1.5);
correctLayout at K = 797: first iterate 4.8e-6 max, 2.3e-6 l2 from the Abbe model's.  Fold edges (a 4,199,495-element row through
the grid-stride loop, 1 ... 3 elements, 65,535 groups, K 300, views 1 ... 3 floats into their allocations): no element differs.
N = 4 pn: (64, 256) ran at its own size on the generic kernels, one launch per kernel (embedded size 64, variant -1, 40 launches),
max 6.8e-7, l2 3.2e-7; (128, 512) ran embedded in 256 (variant 1, 4 launches), max 6.8e-7, l2 2.6e-7; the wrapping source at pn 64
(no box, generic kernels, chunks of 7): max 4.1e-7, l2 2.0e-7 (against abbeIntensity(weights=): 4.8e-7 ... 6.1e-7 max)."""
import numpy as np
import pytest
import torch

import opc_case as C
import socs_oracle as SO
from helpers import DEMO_AB, NA, PS, TOL_IMAGE_L2, TOL_IMAGE_MAX, WL, f16, rel_l2, rel_max

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


def _check(tag, got, want):
    e_max, e_l2 = rel_max(got.cpu(), want), rel_l2(got.cpu(), want)
    print(f"{tag}: max {e_max:.2e} (bound {TOL_IMAGE_MAX:.0e}), l2 {e_l2:.2e} (bound {TOL_IMAGE_L2:.0e})")
    assert e_max < TOL_IMAGE_MAX and e_l2 < TOL_IMAGE_L2, (tag, e_max, e_l2)


# ---- litho_tcc_apply ---------------------------------------------------------------------------------------------------------
def _tcc_apply(nat, dev, ph, wsh, X, Y):
    nat.check(nat.lib().litho_tcc_apply(nat.ptr(ph), nat.ptr(wsh), nat.ptr(X), nat.ptr(Y), X.shape[0], X.shape[-1],
                                        nat.stream_ptr(dev)), "litho_tcc_apply")
    torch.cuda.synchronize()
    return Y


@pytest.mark.parametrize("name,batch", [("wrap32", 3), ("focus64", 2)])
def test_tcc_apply_against_the_explicit_operator(nat, dev, name, batch):
    """pn 32: wrapping source, demo pupil, grey weights, batch 3; pn 64: defocus.  In place and out of place."""
    P, W, M, N = SO.problem(name)
    pn = P.shape[0]
    g = torch.Generator().manual_seed(7)
    X = torch.view_as_complex(torch.randn((batch, pn, pn, 2), generator=g, dtype=torch.float32))
    A = SO.explicit_A(P.numpy(), W.numpy())
    x = X.numpy().astype(np.complex128).reshape(batch, -1)
    want = (A.T @ (A.conj() @ x.T)).T.reshape(batch, pn, pn)                   # T x, T = A^T conj(A)
    ph32, wsh32 = torch.fft.fft2(P), torch.fft.ifftshift(W)
    same = torch.fft.ifft2(ph32 * torch.fft.fft2(wsh32 * torch.fft.ifft2(ph32.conj() * torch.fft.fft2(X)))).numpy()
    floor = np.abs(same - want).max() / np.abs(want).max()
    ph = P.to(dev).clone()
    nat.check(nat.lib().litho_fft2_c2c(nat.ptr(ph), 1, pn, 0, nat.stream_ptr(dev)), "litho_fft2_c2c")
    wsh = wsh32.to(dev).contiguous()
    Xd = X.to(dev)
    out = _tcc_apply(nat, dev, ph, wsh, Xd, torch.empty_like(Xd))
    assert torch.equal(Xd.cpu(), X)                                            # out of place leaves X alone
    e_out = np.abs(out.cpu().numpy() - want).max() / np.abs(want).max()
    inplace = _tcc_apply(nat, dev, ph, wsh, Xd, Xd)
    e_in = np.abs(inplace.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"{name} batch {batch}: out of place {e_out:.3e}, in place {e_in:.3e}, complex64 floor {floor:.3e}, "
          f"quotients {e_out / floor:.2f} {e_in / floor:.2f} (bound 4)")
    assert e_out <= 4 * floor and e_in <= 4 * floor
    assert torch.equal(inplace, out)
    # overlapping but distinct buffers are refused
    both = torch.zeros((batch + 1, pn, pn), dtype=torch.complex64, device=dev)
    assert nat.lib().litho_tcc_apply(nat.ptr(ph), nat.ptr(wsh), nat.ptr(both[:batch]), nat.ptr(both[1:]), batch, pn,
                                     nat.stream_ptr(dev)) == nat.E_ARG


# ---- litho_socs_fold ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elems", [33, 30 * 30, 256 * 256])
@pytest.mark.parametrize("K", [1, 2, 7, 64])
def test_fold_is_the_sequential_fp32_sum_bit_for_bit(nat, dev, K, elems):
    for groups in (1, 3):
        g = torch.Generator().manual_seed(K * 1000 + groups)
        stack = torch.randn((groups * K, elems), generator=g, dtype=torch.float32)
        start = torch.randn((groups, elems), generator=g, dtype=torch.float32)
        for accumulate in (0, 1):
            want = start.numpy().copy() if accumulate else np.zeros((groups, elems), dtype=np.float32)
            for gi in range(groups):
                for k in range(K):
                    want[gi] = want[gi] + stack[gi * K + k].numpy()
            sd, out = stack.to(dev), start.to(dev).clone()
            nat.check(nat.lib().litho_socs_fold(nat.ptr(sd), groups, K, elems, nat.ptr(out), accumulate, nat.stream_ptr(dev)),
                      "litho_socs_fold")
            torch.cuda.synchronize()
            assert want.dtype == np.float32 and np.array_equal(out.cpu().numpy(), want), (K, elems, groups, accumulate)
    f = nat.lib().litho_socs_fold
    assert f(nat.ptr(sd), 0, K, elems, nat.ptr(out), 0, nat.stream_ptr(dev)) == nat.E_ARG
    assert f(nat.ptr(sd), 1, 0, elems, nat.ptr(out), 0, nat.stream_ptr(dev)) == nat.E_ARG
    assert f(nat.ptr(sd), 1, K, 0, nat.ptr(out), 0, nat.stream_ptr(dev)) == nat.E_ARG
    assert f(None, 1, K, elems, nat.ptr(out), 0, nat.stream_ptr(dev)) == nat.E_ARG


def _fold_want(stack, start, groups, K, accumulate):
    """The sequential fp32 sum, k ascending, one running sum per element (numpy float32 adds)."""
    want = start.numpy().copy() if accumulate else np.zeros(tuple(start.shape), dtype=np.float32)
    for gi in range(groups):
        for k in range(K):
            want[gi] = want[gi] + stack[gi * K + k].numpy()
    assert want.dtype == np.float32
    return want


# beyond 4096 workgroups of 256 threads x 4 elements the kernel strides: a whole stride, a partial second one and a 3-element tail
FOLD_STRIDE = 4096 * 256 * 4
FOLD_EDGES = [(FOLD_STRIDE + 4 * (256 * 5 + 17) + 3, 3, 2),                     # (elems, K, groups)
              (1, 3, 2), (2, 3, 2), (3, 3, 2),                                 # the tail alone
              (6, 2, 65535),                                                    # the largest grid.y
              (1000, 300, 2)]


@pytest.mark.parametrize("elems,K,groups", FOLD_EDGES)
def test_fold_edges_bit_for_bit(nat, dev, elems, K, groups):
    g = torch.Generator().manual_seed(elems % 100003 + K)
    stack = torch.randn((groups * K, elems), generator=g, dtype=torch.float32)
    start = torch.randn((groups, elems), generator=g, dtype=torch.float32)
    sd = stack.to(dev)
    for accumulate in (0, 1):
        want = _fold_want(stack, start, groups, K, accumulate)
        out = start.to(dev).clone()
        nat.check(nat.lib().litho_socs_fold(nat.ptr(sd), groups, K, elems, nat.ptr(out), accumulate, nat.stream_ptr(dev)),
                  "litho_socs_fold")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        wrong = int((got != want).sum())
        print(f"fold elems {elems} K {K} groups {groups} accumulate {accumulate}: {wrong} of {want.size} elements differ")
        assert wrong == 0
        assert torch.equal(sd.cpu(), stack)                                     # the stack is read only


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_fold_from_views_that_are_only_4_byte_aligned(nat, dev, offset):
    """`stack` and `out` start `offset` floats into their allocations; elems is odd, so every row has another alignment.  The
    floats around the views stay what they were."""
    elems, K, groups = 1031, 5, 3
    g = torch.Generator().manual_seed(offset)
    stack = torch.randn((groups * K, elems), generator=g, dtype=torch.float32)
    start = torch.randn((groups, elems), generator=g, dtype=torch.float32)
    for accumulate in (0, 1):
        want = _fold_want(stack, start, groups, K, accumulate)
        sbuf = torch.full((offset + stack.numel() + 4,), 7.0, dtype=torch.float32, device=dev)
        obuf = torch.full((offset + start.numel() + 4,), 9.0, dtype=torch.float32, device=dev)
        sv, ov = sbuf[offset:offset + stack.numel()], obuf[offset:offset + start.numel()]
        sv.copy_(stack.reshape(-1).to(dev))
        ov.copy_(start.reshape(-1).to(dev))
        assert sv.data_ptr() % 16 == 4 * offset and ov.data_ptr() % 16 == 4 * offset
        nat.check(nat.lib().litho_socs_fold(nat.ptr(sv), groups, K, elems, nat.ptr(ov), accumulate, nat.stream_ptr(dev)),
                  "litho_socs_fold")
        torch.cuda.synchronize()
        assert np.array_equal(ov.cpu().numpy().reshape(groups, elems), want), (offset, accumulate)
        assert bool((obuf[:offset] == 9.0).all()) and bool((obuf[offset + start.numel():] == 9.0).all())
        assert bool((sbuf[:offset] == 7.0).all()) and bool((sbuf[offset + stack.numel():] == 7.0).all())


def test_fold_refuses_what_its_grid_cannot_hold(nat, dev):
    """groups = 65536 (grid.y ends at 65535) and elems = 2^40 + 1; both return before anything is launched, so the buffers may
    be small and stay as they were."""
    sd = torch.ones((4, 8), dtype=torch.float32, device=dev)
    out = torch.full((2, 8), 3.0, dtype=torch.float32, device=dev)
    f, st = nat.lib().litho_socs_fold, nat.stream_ptr(dev)
    assert f(nat.ptr(sd), 65536, 2, 6, nat.ptr(out), 0, st) == nat.E_ARG
    assert f(nat.ptr(sd), 1, 2, (1 << 40) + 1, nat.ptr(out), 0, st) == nat.E_ARG
    assert f(nat.ptr(sd), 1, 2, 8, None, 0, st) == nat.E_ARG
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((sd == 1.0).all())


# ---- full-rank parity --------------------------------------------------------------------------------------------------------
_strided = {}


def _strided_problem(L, dev, pn, N, ab="demo", mask="bernoulli"):
    """The `_problem` recipe of test_gpu_weighted.py: Bernoulli mask spectrum, pupil, 40 strided points of the annular 0.4-0.8
    list with weights in (0, 2] -- here also as the weight map socsKernels takes -- and the float64 truth (computed once)."""
    key = (pn, N, ab, mask)
    if key not in _strided:
        from lithographysimulator_amd.synthetic import bernoulli_mask, lines_mask
        mft = L.Mask(bernoulli_mask(pn) if mask == "bernoulli" else lines_mask(pn), PS, dev).fraunhofer(WL, True)
        pf = L.Pupil(pn, WL, NA, f16(DEMO_AB) if ab == "demo" else f16(ab), dev).generatePupilFunction()
        sh = L.sourceShifts(L.LightSource(0.4, 0.8, pn, NA, device=dev).generateAnnular(), pn)
        sel = sh[(torch.arange(40, device=dev) * sh.shape[0]) // 40].contiguous()
        g = torch.Generator().manual_seed(5)
        w = (2.0 * (1.0 - torch.rand(40, generator=g, dtype=torch.float64))).to(torch.float32).to(dev)
        W = torch.zeros((pn, pn), dtype=torch.float32, device=dev)
        W[(sel[:, 0] + pn // 2).long(), (sel[:, 1] + pn // 2).long()] = w
        truth = SO.abbe_truth(pf.cpu(), mft.cpu(), W.cpu().numpy(), N)
        _strided[key] = (mft, pf, sel, w, W, truth)
    return _strided[key]


@pytest.mark.parametrize("name", ["plain32", "wrap32"])
def test_full_rank_parity_at_32(L, dev, nat, name):
    """(pn, N) = (32, 64), S = 92, the plain annular source and the shifted one that wraps the pupil around the grid."""
    P, W, M, N = SO.problem(name)
    Pd, Wd, Md = P.to(dev), W.to(dev), M.to(dev)
    k = L.socsKernels(Pd, Wd, kernels=92, oversample=0)
    assert k.K == 92 and k.lit_points == 92 and (k.boxes == [None]) == (name == "wrap32")
    got = L.hopkinsIntensity(Md, k, N)
    print(f"{name}: captured {k.captured:.8f}, plan {nat.last_plan()}")
    _check(f"{name} hopkins vs float64 Abbe", got, SO.truth(name))
    sh, w = L.sourceWeights(Wd, 32)
    _check(f"{name} hopkins vs abbeIntensity(weights=)", got, L.abbeIntensity(Md, Pd, sh, N, weights=w).cpu().double())
    assert abs(k.captured - 1.0) < 1e-5


@pytest.mark.parametrize("pn,N", [(128, 256), (128, 128), (256, 512)])
def test_full_rank_parity_strided(L, dev, nat, pn, N):
    mft, pf, sel, w, W, truth = _strided_problem(L, dev, pn, N)
    k = L.socsKernels(pf, W, kernels=40, oversample=0)
    assert k.K == 40 and k.boxes[0] is not None
    got = L.hopkinsIntensity(mft, k, N)
    plan = nat.last_plan()
    print(f"pn {pn} N {N}: captured {k.captured:.8f}, box {k.boxes[0]}, engine box rows {plan['box_rows']} cols {plan['box_cols']}")
    r_lo, r_hi, c_lo, c_hi = k.boxes[0]
    outside = torch.ones((pn, pn), dtype=torch.bool, device=dev)
    outside[r_lo:r_hi + 1, c_lo:c_hi + 1] = False
    assert int((k.kernels[:, outside] != 0).sum()) == 0 and r_hi - r_lo + 1 < pn and c_hi - c_lo + 1 < pn
    _check(f"pn {pn} N {N} hopkins vs float64 Abbe", got, truth)
    _check(f"pn {pn} N {N} hopkins vs abbeIntensity(weights=)", got, L.abbeIntensity(mft, pf, sel, N, weights=w).cpu().double())


@pytest.mark.parametrize("pn,N", [(64, 256), (128, 512)])
def test_full_rank_parity_at_n_equal_4_pn(L, dev, nat, pn, N):
    """N = 4 pn: neither of the engine's specialised geometries (pn = N, pn = N / 2).  Which grid and which kernels the engine
    takes for the kernel stack is printed, not predicted."""
    from lithographysimulator_amd.imageformation import embeddedSize
    mft, pf, sel, w, W, truth = _strided_problem(L, dev, pn, N)
    k = L.socsKernels(pf, W, kernels=40, oversample=0)
    assert k.K == 40 and k.boxes[0] is not None
    got = L.hopkinsIntensity(mft, k, N)
    print(f"pn {pn} N {N}: captured {k.captured:.8f}, box {k.boxes[0]}, litho_abbe_embedded_size {embeddedSize(pn, N)}, "
          f"plan {nat.last_plan()}")
    _check(f"pn {pn} N {N} hopkins vs float64 Abbe", got, truth)
    _check(f"pn {pn} N {N} hopkins vs abbeIntensity(weights=)", got, L.abbeIntensity(mft, pf, sel, N, weights=w).cpu().double())
    assert abs(k.captured - 1.0) < 1e-5


def test_full_rank_parity_with_a_wrapping_source_at_64(L, dev, nat):
    """The shifted annular source of the truncated tests' setting (c), thinned to 40 strided points: no masking box, so the
    engine sees full-grid kernels; folded in chunks of 7."""
    pn, N = SO.TRUNC_PN, SO.TRUNC_N
    P, Wc = SO.truncated_setting("c")
    W = Wc * SO.strided_points(Wc > 0, 40)
    M = SO.truncated_mask()
    Pd, Wd, Md = P.to(dev), W.to(dev), M.to(dev)
    k = L.socsKernels(Pd, Wd, kernels=40, oversample=0)
    assert k.K == 40 and k.lit_points == 40 and k.boxes == [None]
    got = L.hopkinsIntensity(Md, k, N, kernelChunk=7)
    print(f"wrapping source at pn 64: captured {k.captured:.8f}, plan {nat.last_plan()}")
    _check("wrap64 hopkins vs float64 Abbe", got, SO.abbe_truth(P, M, W.numpy(), N))
    sh, w = L.sourceWeights(Wd, pn)
    _check("wrap64 hopkins vs abbeIntensity(weights=)", got, L.abbeIntensity(Md, Pd, sh, N, weights=w).cpu().double())
    assert abs(k.captured - 1.0) < 1e-5


def test_kernel_chunks_give_the_same_image(L, dev):
    mft, pf, sel, w, W, truth = _strided_problem(L, dev, 128, 256)
    k = L.socsKernels(pf, W, kernels=40, oversample=0)
    whole = L.hopkinsIntensity(mft, k, 256, kernelChunk=40)
    for chunk in (1, 7):
        part = L.hopkinsIntensity(mft, k, 256, kernelChunk=chunk)
        e = rel_max(part, whole)
        print(f"kernelChunk {chunk} vs 40: {e:.2e}")
        assert e < 1e-6
    assert torch.equal(L.hopkinsIntensity(mft, k, 256), whole)                  # the default holds the whole set here
    acc = torch.ones_like(whole)
    assert L.hopkinsIntensity(mft, k, 256, out=acc, kernelChunk=7) is acc       # a given `out` is accumulated into
    assert rel_max(acc - 1.0, whole) < 1e-5
    with pytest.raises(ValueError):
        L.hopkinsIntensity(mft, k, 256, kernelChunk=0)


def test_through_focus_stack(L, dev):
    """Two planes, each against its own truth; a chunk that does not divide K."""
    mft, pf, sel, w, W, truth = _strided_problem(L, dev, 128, 256)
    ab2 = [0, 0, 0, 0, 120]
    _, pf2, _, _, _, truth2 = _strided_problem(L, dev, 128, 256, ab=tuple(ab2))
    k = L.socsKernels(torch.stack([pf, pf2]), W, kernels=40, oversample=0)
    assert tuple(k.kernels.shape) == (2, 40, 128, 128) and k.planes == 2
    for chunk in (None, 16):
        got = L.hopkinsIntensity(mft, k, 256, kernelChunk=chunk)
        assert tuple(got.shape) == (2, 128, 128)
        _check(f"stack plane 0 (demo), chunk {chunk}", got[0], truth)
        _check(f"stack plane 1 (defocus 120), chunk {chunk}", got[1], truth2)


def test_truncated_kernels_on_the_device(L, dev):
    """K = 24 of 92 at pn 32 under the CPU test's rule: error <= 1.5 x the exact rank-24 truncation's + TOL_IMAGE_MAX."""
    P, W, M, N = SO.problem("wrap32")
    phi, lam = SO.exact_kernels(P.numpy(), W.numpy())
    floor = rel_max(SO.kernel_image(torch.from_numpy(phi[:24]), M, N), SO.truth("wrap32"))
    k = L.socsKernels(P.to(dev), W.to(dev), kernels=24, oversample=8)
    err = rel_max(L.hopkinsIntensity(M.to(dev), k, N).cpu(), SO.truth("wrap32"))
    print(f"K 24 on the device: image error {err:.3e}, exact rank-24 truncation {floor:.3e}, ratio {err / floor:.3f}, "
          f"captured {k.captured:.4f} (exact {lam[:24].sum() / lam.sum():.4f})")
    assert err <= 1.5 * floor + TOL_IMAGE_MAX
    assert abs(k.captured - lam[:24].sum() / lam.sum()) < 1e-3


def test_plan_reuse_and_another_mask(L, dev, nat):
    mft, pf, sel, w, W, truth = _strided_problem(L, dev, 128, 256)
    k = L.socsKernels(pf, W, kernels=40, oversample=0)
    first = L.hopkinsIntensity(mft, k, 256, kernelChunk=16)
    assert nat.last_plan()["planned_from_record"] == 0
    again = L.hopkinsIntensity(mft, k, 256, kernelChunk=16)
    assert nat.last_plan()["planned_from_record"] == 1 and torch.equal(again, first)
    mft2, _, _, _, _, truth2 = _strided_problem(L, dev, 128, 256, mask="lines")
    other = L.hopkinsIntensity(mft2, k, 256, kernelChunk=16)
    assert nat.last_plan()["planned_from_record"] == 1
    _check("another mask through the same kernels", other, truth2)
    assert not torch.equal(other, first)


def test_hopkins_image_is_abbe_images_post_process(L, dev):
    from lithographysimulator_amd.synthetic import bernoulli_mask
    mft, pf, sel, w, W, truth = _strided_problem(L, dev, 128, 256)
    mask = L.Mask(bernoulli_mask(128), PS, dev)
    k = L.socsKernels(pf, W, kernels=40, oversample=0)
    for norm in (False, True):
        want = L.abbeImage(mask, mft, pf, W, PS, mask.deltaK, WL, True, dev, weighted=True, normalize=norm)
        got = L.hopkinsImage(mask, mft, k, PS, mask.deltaK, WL, normalize=norm)
        assert got.shape == want.shape
        _check(f"hopkinsImage normalize={norm}", got, want.cpu().double())


# ---- correctLayout(model="socs") --------------------------------------------------------------------------------------------
def test_correct_layout_with_the_socs_model(L, dev, golden):
    """tests/opc_case.py with K = the number of lit points: an OPCResult, and the first iterate's image within the image
    tolerances of the Abbe model's first iterate.  Nothing is asserted about EPE values."""
    from lithographysimulator_amd import metrology
    g = golden("g19_opc_loop.npz")
    pupil = L.Pupil(C.PN, C.WAVELENGTH, C.NA, None, device=dev).generatePupilFunction()
    source = L.LightSource(C.SIGMA_IN, C.SIGMA_OUT, C.PN, C.NA, device=dev).generateAnnular()
    S = int(torch.count_nonzero(source))
    assert S == int(g["source_points"])
    images, inner = {}, metrology.measureEPE
    results = {}
    for model in ("abbe", "socs"):
        seen = []

        def spy(image, *a, **k):
            seen.append(image.clone())
            return inner(image, *a, **k)

        metrology.measureEPE = spy
        try:
            results[model] = L.correctLayout(C.layout(), C.PN, C.PIXEL, C.ORIGIN, C.WAVELENGTH, pupil, source, float(g["threshold"]),
                                             spacing=C.SPACING, iterations=2, gain=C.GAIN, maxBias=C.MAX_BIAS, antialias=C.ANTIALIAS,
                                             searchRange=C.RANGE, model=model, kernels=S)
        finally:
            metrology.measureEPE = inner
        images[model] = seen[0]
    assert isinstance(results["socs"], L.OPCResult) and len(results["socs"].history) == 2
    print("abbe history", results["abbe"].history, "socs history", results["socs"].history)
    _check("first iterate, socs vs abbe", images["socs"], images["abbe"].cpu().double())
    with pytest.raises(ValueError):
        L.correctLayout(C.layout(), C.PN, C.PIXEL, C.ORIGIN, C.WAVELENGTH, pupil, source, 0.3, spacing=C.SPACING, maxBias=10.0,
                        model="hopkins")
