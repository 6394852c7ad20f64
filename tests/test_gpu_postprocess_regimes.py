"""The post-process pass (|raw| -> bilinear resample by 1/epsilon -> pad) and everything fused into it -- the resist
threshold (k_postprocess<true>), the diffused image (k_postprocess_diffused and both instantiations of its loader) -- in
every sizing regime, not only the one the demo grids reach.  With ns = floor(pn / epsilon) and
pW = (pn - round(pn / epsilon)) // 2 at 193 nm:

  pad   epsilon > 1: down-sample, zero border, pW > 0 (every power-of-two pn at 25 nm);
  copy  ns == pn: torch copies, with or without a one-pixel crop;
  crop  epsilon < 1: up-sample, then the pad's NEGATIVE width crops; ns odd makes the crop asymmetric.

Every bound is derived or is an equality; none is fitted.
 (a) plain image against a float64 bilinear on the fp32 coordinates of oracle.bilinear_resize (src one fused rounding,
     clamped at 0; l1 = src - i0 exact): the fp32 roundings are 1 - l1, the inner product, the inner sum, the outer product
     and the final sum -- five deep -- so 6 * 2^-24 * max|raw|; against torch's own F.interpolate + F.pad on the CPU (the
     reference's op chain), each side's six: 12 * 2^-24 * max|raw|.  optics.hip is built without contraction and performs
     the oracle's fp32 operations in the oracle's order: on the MI355X every element of every case (1 467 912 of 1 467 912
     over the fourteen 3-plane stacks) is bit-equal to oracle.post_process, so equality is asserted as well; against the
     float64 bilinear the worst case sits at 2.48 of the 6 units, against torch's chain at 2.67 of the 12.  The copy regime is
     |raw| cropped, exact.
 (b) resist == (image * fp32(dose) >= fp32(threshold)), the image of the same pass bit-equal to postProcess.
 (c) diffused image against resist_oracle.diffuse(float64(postProcess)) at test_gpu_resist.bound_factor:
     (2 (2R+2) + 4) 2^-24 max D, for R below the crop, above it, and larger than the image.
 (d) raw = 1 in the crop regime: the post-processed image is all ones with no border, so D[y, x] = c(y) c(x),
     c(j) = sum of the taps that stay inside the grid -- a closed form that shares nothing with the restatement.
 (e) NULL outputs and the plane stride of a cropped stack through the C entry.

Before the loader of the diffused pass took the output grid into account, (c) and (d) failed in every crop and copy + crop
row and nowhere else: the halo read the part of the resampled image that the pad had cropped away, where the definition
(include/litho_abbe.h) has zeros.  Worst |D_gpu - D_f64| / bound on the MI355X then: copy + crop 2.7e5, crop 2.9e5 (pad
0.193, copy 0.180), the corner of the constant image 1.0 where the closed form has 0.444 (R = 5); now 0.193 / 0.180 / 0.205 /
0.206 for pad / copy / copy + crop / crop, and the constant image within 0.070 of its bound."""
import ctypes

import numpy as np
import pytest
import torch

import resist_oracle as RO
from helpers import WL
from test_gpu_resist import U, bound_factor

pytestmark = pytest.mark.gpu

# (pn, pixel size nm, ns, pW, n_out, regime)
CASES = [
    (64, 25, 61, 1, 64, "pad"),             # odd ns
    (100, 25, 75, 12, 100, "pad"),          # not a power of two
    (200, 25, 150, 24, 198, "pad"),         # n_out < pn
    (118, 25, 104, 6, 116, "pad"),          # even ns, n_out < pn
    (64, 48, 64, 0, 64, "copy"),            # no crop
    (128, 48, 128, -1, 126, "copy+crop"),
    (14, 10, 14, -1, 12, "copy+crop"),      # smaller than one tile and than any R >= 12
    (64, 10, 77, -7, 64, "crop"),           # odd ns
    (96, 25, 138, -22, 94, "crop"),         # the default pixel size, n_out < pn
    (62, 40, 72, -5, 62, "crop"),           # even ns
    (256, 48, 257, -1, 256, "crop"),        # up-sample by one pixel, asymmetric crop (1 left, 0 right)
    (502, 64, 742, -120, 502, "crop"),      # crop wider than any halo, several tiles, partial last tile
    (256, 10, 308, -27, 254, "crop"),       # n_out a multiple of no tile
    (62, 64, 90, -15, 60, "crop"),          # n_out < pn
]
IDS = [f"{c[0]}-{c[1]}nm-{c[5]}" for c in CASES]
SINGLE_PLANE = {(118, 25), (64, 48), (128, 48), (62, 64)}       # one 2-D call per regime
SIGMAS_PX = (0.5, 1.2, 3.0, 8.0)                                # R = 2, 5, 12, 32
PLANES = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    import lithographysimulator_amd as L
    return L


def _eps(pn, ps):
    from oracle import abbe_oracle as O
    return O.calculate_epsilon_n(4 / pn, ps, WL)[0]


def _geometry(pn, eps):
    ns = int(np.floor(pn * (1.0 / eps)))
    pW = (pn - round(pn / eps)) // 2
    return ns, pW, ns + 2 * pW + ns % 2


def _pad(img, pW, corr):
    """F.pad(img, (pW, pW + corr, pW, pW + corr)) on the last two axes of a numpy array; a negative width crops."""
    lo, hi = pW, pW + corr
    n = img.shape[-1]
    img = img[..., max(0, -lo): n - max(0, -hi), max(0, -lo): n - max(0, -hi)]
    return np.pad(img, [(0, 0)] * (img.ndim - 2) + [(max(0, lo), max(0, hi))] * 2)


def _post_process_f64(raw, eps):
    """|raw| [planes, pn, pn] resampled in float64 on oracle.bilinear_resize's fp32 coordinates, then padded."""
    a = np.abs(raw.numpy().astype(np.float64))
    pn = a.shape[-1]
    ns, pW, _ = _geometry(pn, eps)
    if ns != pn:
        rs = np.float32(1.0 / (1.0 / eps))
        src = np.maximum((np.float64(rs) * (np.arange(ns, dtype=np.float64) + 0.5) - 0.5).astype(np.float32), np.float32(0))
        i0 = np.floor(src).astype(np.int64)
        i1 = np.minimum(i0 + 1, pn - 1)
        l1 = (src - i0.astype(np.float32)).astype(np.float64)
        l0 = 1.0 - l1
        r0, r1 = a[:, i0, :], a[:, i1, :]
        a = (l0[:, None] * (l0[None, :] * r0[:, :, i0] + l1[None, :] * r0[:, :, i1])
             + l1[:, None] * (l0[None, :] * r1[:, :, i0] + l1[None, :] * r1[:, :, i1]))
    return _pad(a, pW, ns % 2)


_cache = {}


def _case(L, dev, case):
    """Everything the tests of one case share, computed once: the seeded signed raw stack, the float64 and fp32 references
    of the plain pass and postProcess's own output."""
    if case not in _cache:
        from oracle import abbe_oracle as O
        pn, ps, ns, pW, n_out, regime = case
        eps = _eps(pn, ps)
        assert _geometry(pn, eps) == (ns, pW, n_out), (case, _geometry(pn, eps))     # the case is in the regime it claims
        size = ctypes.c_int(0)
        from lithographysimulator_amd import _native as nat
        assert nat.lib().litho_postprocess_size(pn, eps, ctypes.byref(size)) == 0 and size.value == n_out
        assert {"pad": eps > 1 and pW > 0, "copy": ns == pn and pW == 0, "copy+crop": ns == pn and pW < 0,
                "crop": eps < 1 and ns > pn and pW < 0}[regime]
        raw = torch.rand(PLANES, pn, pn, generator=torch.Generator().manual_seed(1000 * pn + ps)) * 3.0 - 1.5
        raw_dev = raw.to(dev)
        plain = L.postProcess(raw_dev, eps)
        assert tuple(plain.shape) == (PLANES, n_out, n_out) and plain.dtype == torch.float32
        _cache[case] = dict(eps=eps, raw=raw, raw_dev=raw_dev, plain=plain, plain_h=plain.cpu().numpy(),
                            ref64=_post_process_f64(raw, eps),
                            ref32=torch.stack([O.post_process(r, eps) for r in raw]).numpy())
    return _cache[case]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plain_postprocess_whole_array(L, dev, case):
    pn, ps, ns, pW, n_out, regime = case
    c = _case(L, dev, case)
    raw, eps, got = c["raw"], c["eps"], c["plain_h"]
    peak = float(raw.abs().max())
    assert got.shape == c["ref64"].shape == c["ref32"].shape
    err = float(np.abs(got.astype(np.float64) - c["ref64"]).max())
    x = torch.nn.functional.interpolate(raw.abs()[None], scale_factor=1.0 / eps, mode="bilinear", align_corners=False)[0]
    assert x.shape[-1] == ns
    chain = torch.nn.functional.pad(x, (pW, pW + ns % 2, pW, pW + ns % 2)).numpy()
    assert chain.shape == got.shape
    err_chain = float(np.abs(got.astype(np.float64) - chain.astype(np.float64)).max())
    equal = int(np.sum(got.view(np.int32) == c["ref32"].view(np.int32)))
    print(f"REGIME {regime} pn {pn} ps {ps}: max|I_gpu - I_f64| = {err / (U * peak):.3f} units of 2^-24 max|raw| (bound 6), against "
          f"F.interpolate + F.pad {err_chain / (U * peak):.3f} (bound 12), {equal} of {got.size} bit-equal to the fp32 oracle")
    assert err <= 6 * U * peak, (case, err / (U * peak))
    assert err_chain <= 12 * U * peak, (case, err_chain / (U * peak))
    assert equal == got.size                                                   # the oracle's operations in the oracle's order
    if ns == pn:                                                               # the copy: |raw| cropped, exact
        assert np.array_equal(got, _pad(raw.abs().numpy(), pW, 0))
    if pW > 0:                                                                 # the border is exactly zero, the far side one wider
        assert not got[:, :pW].any() and not got[:, :, :pW].any()
        assert not got[:, pW + ns:].any() and not got[:, :, pW + ns:].any()
    if (pn, ps) in SINGLE_PLANE:
        assert torch.equal(L.postProcess(c["raw_dev"][1], eps), c["plain"][1])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_resist_threshold_on_the_stack(L, dev, case):
    pn, ps = case[:2]
    c = _case(L, dev, case)
    raw, eps, plain = c["raw_dev"], c["eps"], c["plain"]
    for dose, thr in ((1.0, 0.75), (0.7, 0.4), (1.3, 0.0)):
        image, resist = L.resistContour(raw, eps, thr, dose=dose, return_image=True)
        assert resist.dtype == torch.uint8 and resist.shape == image.shape == plain.shape
        assert torch.equal(image, plain)
        expect = (image * torch.tensor(dose, dtype=torch.float32, device=dev)
                  >= torch.tensor(thr, dtype=torch.float32, device=dev)).to(torch.uint8)
        assert torch.equal(resist, expect)
        assert thr == 0.0 or 0 < int(resist.sum()) < resist.numel()
        assert torch.equal(L.resistContour(raw, eps, thr, dose=dose), resist)               # out = NULL
        if (pn, ps) in SINGLE_PLANE:
            img1, res1 = L.resistContour(raw[1], eps, thr, dose=dose, return_image=True)
            assert torch.equal(img1, plain[1]) and torch.equal(res1, resist[1])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_diffused_image_and_contour(L, dev, case):
    pn, ps, ns, pW, n_out, regime = case
    c = _case(L, dev, case)
    raw, eps, plain = c["raw_dev"], c["eps"], c["plain"]
    I64 = c["plain_h"].astype(np.float64)
    dose = 0.7
    failures = []
    for sigma_px in SIGMAS_PX:
        length = sigma_px * ps
        R = RO.radius(length / ps)                                             # the very division the wrapper performs
        assert R == {0.5: 2, 1.2: 5, 3.0: 12, 8.0: 32}[sigma_px]
        D64 = RO.diffuse(I64, length / ps)
        thr = 0.4 * float(D64.max())
        if float(D64.min()) >= thr:                                            # R = 32 on the 12^2 image: nowhere below 0.4 max D
            thr = 0.5 * float(D64.min() + D64.max())
        thr *= dose
        u64 = D64 * float(np.float32(dose))
        band = bound_factor(R) * float(u64.max())
        in_band = int((np.abs(u64 - float(np.float32(thr))) <= band).sum())    # the restatement's own count, before the device
        assert in_band <= max(2, 1e-4 * D64.size), (case, sigma_px, in_band)
        ref = RO.contour(D64.astype(np.float32), dose, thr)
        assert 0 < int(ref.sum()) < ref.size
        D, resist = L.resistContour(raw, eps, thr, dose=dose, return_image=True, diffusionLength=length, pixelSize=ps)
        assert D.shape == plain.shape and resist.shape == plain.shape and resist.dtype == torch.uint8
        err = float(np.abs(D.cpu().numpy().astype(np.float64) - D64).max())
        bound = bound_factor(R) * float(D64.max())
        print(f"REGIME {regime} pn {pn} ps {ps} R={R} (|pW| = {abs(pW)}, n_out = {n_out}): max|D_gpu - D_f64| = {err:.3e} = "
              f"{err / bound:.4g} of the bound")
        if err > bound:
            failures.append(f"R={R}: max|D_gpu - D_f64| = {err:.3e} = {err / bound:.4g} of the bound {bound:.3e}")
        # the contour is exactly the threshold on the D of the same pass ...
        expect = (D * torch.tensor(dose, dtype=torch.float32, device=dev)
                  >= torch.tensor(thr, dtype=torch.float32, device=dev)).to(torch.uint8)
        assert torch.equal(resist, expect)
        assert torch.equal(L.resistContour(raw, eps, thr, dose=dose, diffusionLength=length, pixelSize=ps), resist)
        # ... and the restatement's, except where the derived bound straddles the threshold
        differ = resist.cpu().numpy() != ref
        if not (np.abs(u64[differ] - float(np.float32(thr))) <= band).all() or int(differ.sum()) > in_band:
            failures.append(f"R={R}: the contour differs from the restatement's at {int(differ.sum())} pixels, {in_band} in the band")
        if (pn, ps) in SINGLE_PLANE:
            D1, res1 = L.resistContour(raw[1], eps, thr, dose=dose, return_image=True, diffusionLength=length, pixelSize=ps)
            assert torch.equal(D1, D[1]) and torch.equal(res1, resist[1])
    assert not failures, (case, failures)


@pytest.mark.parametrize("case", [CASES[8], CASES[5]], ids=[IDS[8], IDS[5]])
def test_sigma_zero_is_the_plain_pass_bit_for_bit(L, dev, case):
    from lithographysimulator_amd import _native as nat
    pn, ps, ns, pW, n_out, regime = case
    c = _case(L, dev, case)
    raw, eps, plain = c["raw_dev"], c["eps"], c["plain"]
    img0, res0 = L.resistContour(raw, eps, 0.5, dose=0.7, return_image=True)
    D, resist = L.resistContour(raw, eps, 0.5, dose=0.7, return_image=True, diffusionLength=0.0, pixelSize=ps)
    assert torch.equal(D, plain) and torch.equal(D, img0) and torch.equal(resist, res0)
    out, res = torch.full_like(plain, -7.0), torch.full_like(res0, 9)
    with torch.cuda.device(dev):                                               # and through the diffused entry itself
        assert nat.lib().litho_postprocess_resist_diffused(nat.ptr(raw), PLANES, pn, eps, 0.7, 0.5, 0.0, nat.ptr(out), nat.ptr(res),
                                                           nat.stream_ptr(dev)) == 0
        torch.cuda.synchronize()
    assert torch.equal(out, plain) and torch.equal(res, res0)


@pytest.mark.parametrize("pn,ps", [(64, 10), (128, 48), (96, 25)])
def test_constant_image_diffuses_to_the_closed_form(L, dev, pn, ps):
    """raw = 1 where the pad crops: the image is all ones up to its very edge, so D = c(y) c(x) with c(j) the sum of the
    taps k in [-R, R] that keep 0 <= j + k < n_out.  The corner is ((1 + g0) / 2)^2, not 1: a kernel and a restatement that
    shared a mistake about what lies outside the grid could not both satisfy this."""
    eps = _eps(pn, ps)
    ns, pW, n_out = _geometry(pn, eps)
    assert pW < 0
    raw = torch.ones(pn, pn, device=dev)
    plain = L.postProcess(raw, eps).cpu().numpy()
    assert plain.shape == (n_out, n_out) and float(np.abs(plain.astype(np.float64) - 1.0).max()) <= 3 * U
    failures = []
    for sigma_px in (1.2, 3.0):
        g, R = RO.taps(sigma_px), RO.radius(sigma_px * ps / ps)
        assert R == {1.2: 5, 3.0: 12}[sigma_px]
        j = np.arange(n_out)
        c = np.array([g[max(0, R - x): min(2 * R + 1, R + n_out - x)].sum() for x in j])
        want = np.outer(c, c)
        corner = ((g.sum() + g[R]) / 2.0) ** 2
        assert abs(want[0, 0] - corner) < 1e-15 and abs(corner - ((1.0 + g[R]) / 2.0) ** 2) < 1e-6 and corner < 0.5
        D = L.resistContour(raw, eps, 0.5, return_image=True, diffusionLength=sigma_px * ps, pixelSize=ps)[0].cpu().numpy()
        tol = bound_factor(R) * float(want.max()) + 3 * U
        err = float(np.abs(D.astype(np.float64) - want).max())
        print(f"pn {pn} ps {ps} R={R}: max|D_gpu - c(y) c(x)| = {err:.3e} = {err / tol:.4g} of the bound; corner {float(D[0, 0]):.7f}, "
              f"closed form {corner:.7f}")
        if err > tol or abs(float(D[0, 0]) - corner) > tol:
            failures.append(f"R={R}: {err:.3e} = {err / tol:.4g} of the bound {tol:.3e}; corner {float(D[0, 0]):.7f} for {corner:.7f}")
    assert not failures, (pn, ps, failures)


def test_null_outputs_and_the_plane_stride_of_a_cropped_stack(L, dev):
    """pn = 96 at 25 nm: planes of raw are 96^2 apart, planes of either output 94^2.  Through the C entry: resist = NULL gives
    the image only, out = NULL the contour only, and nothing is written behind the last plane of either output."""
    from lithographysimulator_amd import _native as nat
    case = CASES[8]
    pn, ps, ns, pW, n_out, regime = case
    c = _case(L, dev, case)
    raw, eps = c["raw_dev"], c["eps"]
    sigma_px, dose, thr = 1.2, 0.7, 0.3
    D, resist = L.resistContour(raw, eps, thr, dose=dose, return_image=True, diffusionLength=sigma_px * ps, pixelSize=ps)
    words, guard = PLANES * n_out * n_out, 4096
    f = nat.lib().litho_postprocess_resist_diffused
    st = nat.stream_ptr(dev)
    with torch.cuda.device(dev):
        for want_out, want_res in ((True, False), (False, True), (True, True)):
            out = torch.full((words + guard,), -7.0, dtype=torch.float32, device=dev)
            res = torch.full((words + guard,), 9, dtype=torch.uint8, device=dev)
            assert f(nat.ptr(raw), PLANES, pn, eps, dose, thr, sigma_px * ps / ps, nat.ptr(out) if want_out else None,
                     nat.ptr(res) if want_res else None, st) == 0
            torch.cuda.synchronize()
            assert bool((out[words:] == -7.0).all()) and bool((res[words:] == 9).all())
            assert torch.equal(out[:words].view_as(D), D) if want_out else bool((out == -7.0).all())
            assert torch.equal(res[:words].view_as(resist), resist) if want_res else bool((res == 9).all())
        # the plain pass and the threshold pass on the same stack
        out = torch.full((words + guard,), -7.0, dtype=torch.float32, device=dev)
        res = torch.full((words + guard,), 9, dtype=torch.uint8, device=dev)
        assert nat.lib().litho_postprocess_resist(nat.ptr(raw), PLANES, pn, eps, dose, thr, nat.ptr(out), nat.ptr(res), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[:words].view_as(D), c["plain"]) and bool((out[words:] == -7.0).all()) and bool((res[words:] == 9).all())
        out.fill_(-7.0)
        assert nat.lib().litho_postprocess(nat.ptr(raw), PLANES, pn, eps, nat.ptr(out), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[:words].view_as(D), c["plain"]) and bool((out[words:] == -7.0).all())
