"""Weighted (grey-level) sources on the GPU: I = sum_s w_s |E_s|^2 through every evaluation path of the HIP engine
(litho_abbe_accumulate_weighted, litho_source_compact_weighted, abbeIntensity(weights=), abbeImage(weighted=True)).

Truth is the reference's mathematics in float64 -- sum_s w_s |oracle.field_closed_form(P, M, dy, dx, N)|^2 -- or, at the
BASELINE sizes, the UNWEIGHTED engine on a list with every point repeated w times (the parent's tested path).  Tolerances are
the project's own (helpers.TOL_IMAGE_MAX = 2e-5 of the maximum, TOL_IMAGE_L2 = 5e-6); every test prints what it observed.
Run on the MI355X box with  python -m pytest tests/test_gpu_weighted.py -m gpu -s."""
import math
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from helpers import DEMO_AB, NA, PS, ROOT, TOL_IMAGE_L2, TOL_IMAGE_MAX, WL, f16, rel_l2, rel_max, subsample_bitmap

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


def O():
    from oracle import abbe_oracle
    return abbe_oracle


def _weights(n, dev, hi=2.0, seed=5):
    """n weights uniform in (0, hi]."""
    g = torch.Generator().manual_seed(seed)
    return (hi * (1.0 - torch.rand(n, generator=g, dtype=torch.float64))).to(torch.float32).to(dev)


def _truth(P, M, shifts, w, N):
    """sum_s w_s |E_s|^2 in float64 from the closed form of the reference's op chain (oracle.field_closed_form)."""
    Pc, Mc = P.cpu(), M.cpu()
    out = torch.zeros(M.shape, dtype=torch.float64)
    for (dy, dx), ws in zip(shifts.cpu().tolist(), w.cpu().double().tolist()):
        E = O().field_closed_form(Pc, Mc, dy, dx, N)
        out += ws * (E.real ** 2 + E.imag ** 2)
    return out


def _check(tag, got, want):
    e_max, e_l2 = rel_max(got.cpu(), want), rel_l2(got.cpu(), want)
    print(f"{tag}: max {e_max:.2e} (bound {TOL_IMAGE_MAX:.0e}), l2 {e_l2:.2e} (bound {TOL_IMAGE_L2:.0e})")
    assert e_max < TOL_IMAGE_MAX and e_l2 < TOL_IMAGE_L2, (tag, e_max, e_l2)
    return e_max, e_l2


_problem_cache = {}


def _problem(L, dev, pn, N, ab_tag, shift=(0, 0), K=40):
    """Mask spectrum, pupil, ~40 strided points of an annular list, weights in (0, 2] and the float64 truth (computed once)."""
    key = (pn, N, ab_tag, shift, K)
    if key not in _problem_cache:
        from lithographysimulator_amd.synthetic import bernoulli_mask
        mft = L.Mask(bernoulli_mask(pn), PS, dev).fraunhofer(WL, True)
        pf = L.Pupil(pn, WL, NA, f16(DEMO_AB) if ab_tag == "demo" else None, dev).generatePupilFunction()
        bm = L.LightSource(0.4, 0.8, pn, NA, shiftX=shift[0], shiftY=shift[1], device=dev).generateAnnular()
        sh = L.sourceShifts(bm, pn)
        sel = sh[(torch.arange(K, device=dev) * sh.shape[0]) // K].contiguous()
        w = _weights(K, dev)
        _problem_cache[key] = (mft, pf, sel, w, _truth(pf, mft, sel, w, N))
    return _problem_cache[key]


# ---- 1 (and 5): against the reference's mathematics -------------------------------------------------------------------------
SIZES = [(128, 128), (128, 256), (128, 512), (200, 512), (256, 512)]
CASES = [(pn, N, ab, v) for pn, N in SIZES for ab in ("default", "demo")
         for v in (("direct", "coarse", "general", "generic", "poison") if pn == 256 else ("direct", "general", "generic", "poison"))]


@pytest.mark.parametrize("pn,N,ab,variant", CASES)
def test_weighted_sum_vs_closed_form(L, dev, nat, pn, N, ab, variant):
    """pn 128 at N = 128 / 256; pn 128 and 200 at N = 512 (both embedded in a 256 grid); pn 256 at N = 512 in config 1's optical
    setting (the smallest size with a coarse grid).  Direct path, coarse grid (asserted to have run; the error is also taken on
    the pixels with an odd coordinate alone -- the ones the Nyquist correction with w_s-weighted edge products writes), general
    mode, the generic kernels, and poisoned scratch."""
    mft, pf, sel, w, truth = _problem(L, dev, pn, N, ab)
    opts = {"direct": {"coarse": 0}, "coarse": {"coarse": 2}, "general": {"coarse": 0, "force_general": 1},
            "generic": {"coarse": 0, "force_generic": 1}, "poison": {"poison": 1, "coarse": 2 if pn == 256 else 0}}[variant]
    raw = L.abbeIntensity(mft, pf, sel, N, options=opts, weights=w)
    plan, (kx, ky) = nat.last_plan(), nat.last_kernels()
    print(f"pn {pn} N {N} {ab} {variant}: {kx} + {ky}, plan general {plan['general']} variant {plan['variant']} coarse {plan['coarse_grid']}")
    assert not torch.isnan(raw).any()
    if pn in (128, 200) and N == 512 and variant != "general":
        assert L.embeddedSize(pn, N) == 256 and plan["box_rows"] <= 129       # ran embedded in the 256 grid (natural box there)
    if variant == "coarse" or (variant == "poison" and pn == 256):
        assert plan["coarse_grid"] == 1, plan                                  # field 12 of litho_abbe_last_plan
    else:
        assert plan["coarse_grid"] == 0, plan
    if variant == "general":
        assert plan["general"] == 1 and kx.startswith("k_xpass<") and "AbbeLoaderW" in kx, (plan, kx)
    elif variant == "generic":
        assert plan["variant"] == -1 and kx.startswith("k_xpass_abbe<") and "false" in kx and "float const*" in kx, (plan, kx)
    else:
        assert kx.startswith("k_xpass_") and "float const*" in kx, kx
    _check(f"pn {pn} N {N} {ab} {variant}", raw, truth)
    if plan["coarse_grid"] == 1:
        q = torch.arange(pn)
        odd = ((q % 2 == 1)[:, None] | (q % 2 == 1)[None, :])
        d = (raw.cpu().double() - truth)
        e_odd = float(d[odd].abs().max() / truth.max())
        l2_odd = float(torch.linalg.norm(d[odd]) / torch.linalg.norm(truth[odd]))
        print(f"pn {pn} N {N} {ab} {variant}, pixels with an odd coordinate: max {e_odd:.2e}, l2 {l2_odd:.2e}")
        assert e_odd < TOL_IMAGE_MAX and l2_odd < TOL_IMAGE_L2


# ---- 2, 3: ones are free, powers of four are exact ---------------------------------------------------------------------------
def _config1(L, dev):
    from lithographysimulator_amd.synthetic import bernoulli_mask
    pn = 256
    mask = L.Mask(bernoulli_mask(pn), PS, dev)
    mft = mask.fraunhofer(WL, True)
    eps, N = mask.calculateEpsilonN(mask.deltaK, PS, WL)
    bm = L.LightSource(0.0, 0.5, pn, NA, device=dev).generateAnnular()
    pf = L.Pupil(pn, WL, NA, None, dev).generatePupilFunction()
    return mask, mft, pf, bm, L.sourceShifts(bm, pn), N


@pytest.mark.parametrize("path", ["coarse", "direct", "general", "stack"])
def test_ones_are_free(L, dev, nat, path):
    """weights = 1 everywhere reproduces the unweighted call BIT FOR BIT: config 1 (256^2, its full annular source: the coarse
    grid by the default rule), the direct path, general mode and a 3-plane stack."""
    mask, mft, pf, bm, sh, N = _config1(L, dev)
    assert sh.shape[0] == 3233
    ones = torch.ones(sh.shape[0], dtype=torch.float32, device=dev)
    opts = {"coarse": None, "direct": {"coarse": 0}, "general": {"force_general": 1}, "stack": None}[path]
    P = L.throughFocusPupils(256, WL, NA, f16(DEMO_AB), [-80.0, 0.0, 60.0], dev) if path == "stack" else pf
    plain = L.abbeIntensity(mft, P, sh, N, options=opts)
    plan_u, k_u = nat.last_plan(), nat.last_kernels()
    wtd = L.abbeIntensity(mft, P, sh, N, options=opts, weights=ones)
    plan_w, k_w = nat.last_plan(), nat.last_kernels()
    print(f"ones, {path}: unweighted {k_u}, weighted {k_w}; max |diff| {float((wtd - plain).abs().max()):.3e}")
    assert plan_w == plan_u and k_w[1] == k_u[1] and k_w[0] != k_u[0]          # same plan, same y-pass, the weighted x-pass
    assert plan_w["coarse_grid"] == (1 if path in ("coarse", "stack") else 0) and plan_w["general"] == (1 if path == "general" else 0)
    assert torch.equal(wtd, plain)


def test_source_weights_of_a_bitmap_are_source_shifts(L, dev):
    for pn, shift in ((256, 0.0), (128, 0.3)):
        bm = L.LightSource(0.4, 0.8, pn, NA, shiftX=shift, device=dev).generateQuasar(4, -math.pi / 8)
        sh = L.sourceShifts(bm, pn)
        sw, w = L.sourceWeights(bm.to(torch.float32), pn)
        assert torch.equal(sw, sh) and torch.equal(w, torch.ones_like(w)) and w.dtype == torch.float32 and w.shape[0] == sh.shape[0]
        sa, wa, cnt = L.sourceWeightsAsync(bm.to(torch.float32), pn)
        assert int(cnt.item()) == sh.shape[0] and torch.equal(sa[:sh.shape[0]], sh)
    # a grey map: the weights come out in the list's order; zeros, negative values are not lit
    g = torch.Generator().manual_seed(3)
    wm = torch.rand((64, 64), generator=g).to(dev)
    wm[wm < 0.7] = 0.0
    wm[5, 7] = -1.0
    sw, w = L.sourceWeights(wm, 64)
    pts = torch.argwhere(wm > 0)
    assert torch.equal(sw, (pts - 32).int()) and torch.equal(w, wm[pts[:, 0], pts[:, 1]])


@pytest.mark.parametrize("path", ["coarse", "direct"])
def test_powers_of_four_are_exact(L, dev, nat, path):
    """weights = 4 everywhere: a = 2, every fp32 operation scales exactly, so the image is exactly 4 x the unweighted one."""
    mask, mft, pf, bm, sh, N = _config1(L, dev)
    four = torch.full((sh.shape[0],), 4.0, dtype=torch.float32, device=dev)
    opts = {"coarse": 2 if path == "coarse" else 0}
    plain = L.abbeIntensity(mft, pf, sh, N, options=opts)
    wtd = L.abbeIntensity(mft, pf, sh, N, options=opts, weights=four)
    assert nat.last_plan()["coarse_grid"] == (1 if path == "coarse" else 0)
    print(f"fours, {path}: max |weighted - 4 unweighted| / max = {float((wtd - 4 * plain).abs().max() / (4 * plain).max()):.3e}")
    assert torch.equal(wtd, 4.0 * plain)


# ---- 4: integer weights against repetition, at size --------------------------------------------------------------------------
def _repetition(L, dev, nat, pn, kind, lo, count, opts, ab):
    from lithographysimulator_amd.synthetic import bernoulli_mask
    mask = L.Mask(bernoulli_mask(pn), PS, dev)
    mft = mask.fraunhofer(WL, True)
    eps, N = mask.calculateEpsilonN(mask.deltaK, PS, WL)
    src = L.LightSource(0.4, 0.8, pn, NA, device=dev)
    sh = L.sourceShifts(src.generateQuasar(4, -math.pi / 8) if kind == "quasar" else src.generateAnnular(), pn)
    sel = sh[lo:lo + count].contiguous()
    wi = (torch.arange(count, device=dev) % 3) + 1                           # 1, 2, 3, 1, ...
    rep = torch.repeat_interleave(sel, wi, dim=0).contiguous()
    pf = L.Pupil(pn, WL, NA, f16(ab), dev).generatePupilFunction()
    results = []
    for o in opts:
        wtd = L.abbeIntensity(mft, pf, sel, N, options=o, weights=wi.to(torch.float32))
        plan_w, k_w = nat.last_plan(), nat.last_kernels()
        plain = L.abbeIntensity(mft, pf, rep, N, options=o)
        k_u = nat.last_kernels()
        e = (rel_max(wtd, plain), rel_l2(wtd, plain))
        print(f"{pn}^2 N {N} {o}: {count} points weights 1,2,3 vs {rep.shape[0]} repeated: max {e[0]:.2e} l2 {e[1]:.2e}; "
              f"weighted {k_w}, unweighted {k_u}")
        assert e[0] < TOL_IMAGE_MAX and e[1] < TOL_IMAGE_L2, e
        results.append((plan_w, k_w, k_u))
        del wtd, plain
    return N, results


def test_integer_weights_vs_repetition_2048(L, dev, nat):
    """Config 3: 2,000 consecutive points of the 2048^2 quasar list (default plan: the coarse grid)."""
    N, ((plan, (kx, ky), (ux, uy)),) = _repetition(L, dev, nat, 2048, "quasar", 60000, 2000, [None], DEMO_AB)
    assert N == 4096 and plan["coarse_grid"] == 1
    assert kx.startswith("k_xpass_abbe<11, 0, true, 1") and "float const*" in kx and ky == uy and ux == "k_xpass_abbe<11, 0, true, 1, 1>"


def test_integer_weights_vs_repetition_1024_and_512(L, dev, nat):
    """1024^2 (k_xpass_abbe<10, ..> on the coarse grid) and, for the third default x-pass family, 512^2 on the direct path
    (N = 1024: k_xpass_rect<10, ..>)."""
    N, ((plan, (kx, ky), (ux, uy)),) = _repetition(L, dev, nat, 1024, "annular", 30000, 2000, [None], [0, 0, 0, 0, 100])
    assert N == 2048 and plan["coarse_grid"] == 1 and kx.startswith("k_xpass_abbe<10, 0, true, 1") and "float const*" in kx and ky == uy
    N, ((plan, (kx, ky), (ux, uy)),) = _repetition(L, dev, nat, 512, "annular", 8000, 2000, [{"coarse": 0}], DEMO_AB)
    assert N == 1024 and plan["coarse_grid"] == 0 and plan["fused_xpass"] == 3
    assert kx.startswith("k_xpass_rect<10, false") and "float const*" in kx and ux == "k_xpass_rect<10, false>" and ky == uy


def test_integer_weights_vs_repetition_4096(L, dev, nat):
    """Config 4's size: 240 points on the coarse grid (k_ypass_coop_dma behind the weighted k_xpass_abbe<12, 0, ..>) and 60 on
    the direct path at N = 8192 (k_xpass_split<13, ..>)."""
    N, ((plan, (kx, ky), (ux, uy)),) = _repetition(L, dev, nat, 4096, "annular", 400000, 240, [None], [0, 0, 0, 0, 100])
    assert N == 8192 and plan["coarse_grid"] == 1
    assert kx.startswith("k_xpass_abbe<12, 0, true, 1") and "float const*" in kx and ky.startswith("k_ypass_coop_dma") and ky == uy
    N, ((plan, (kx, ky), (ux, uy)),) = _repetition(L, dev, nat, 4096, "annular", 400000, 60, [{"coarse": 0}], [0, 0, 0, 0, 100])
    assert plan["coarse_grid"] == 0 and plan["fused_xpass"] == 2
    assert kx.startswith("k_xpass_split<13") and "float const*" in kx and ux == "k_xpass_split<13>" and ky == uy


# ---- 6: a partly wrapping list is not split -------------------------------------------------------------------------------
def test_partly_wrapping_weighted_list_runs_whole_on_the_general_path(L, dev, nat):
    """A shifted annular source whose shifts wrap the pupil around the grid for SOME points: an unweighted call splits the list
    (options split = 2: whatever its length), a weighted one runs it whole on the general path -- the documented limit -- and
    still computes the reference's sum."""
    pn, N = 128, 256
    mft, pf, sel, w, truth = _problem(L, dev, pn, N, "demo", shift=(0.25, -0.5))
    nz = torch.argwhere(pf.abs() > 0)
    r0, r1, c0, c1 = int(nz[:, 0].min()), int(nz[:, 0].max()), int(nz[:, 1].min()), int(nz[:, 1].max())
    wraps = (r0 + sel[:, 0] < 0) | (r1 + sel[:, 0] > pn - 1) | (c0 + sel[:, 1] < 0) | (c1 + sel[:, 1] > pn - 1)
    assert 0 < int(wraps.sum()) < sel.shape[0]                                 # some wrap, some do not
    L.abbeIntensity(mft, pf, sel, N, options={"split": 2})
    assert nat.last_plan()["planned_from_record"] == 2                         # the unweighted list IS split
    raw = L.abbeIntensity(mft, pf, sel, N, options={"split": 2}, weights=w)
    plan, (kx, ky) = nat.last_plan(), nat.last_kernels()
    assert plan["general"] == 1 and plan["planned_from_record"] != 2 and "AbbeLoaderW" in kx, (plan, kx)
    _check(f"partly wrapping list ({int(wraps.sum())} of {sel.shape[0]} wrap)", raw, truth)


# ---- 7: plan reuse ----------------------------------------------------------------------------------------------------------
def _apodised(L, dev, pn, sigma_in=0.4, sigma_out=0.8, keep=None, scale=1.0):
    """A Gaussian-apodised annulus as a weight map (optionally only `keep` of its pixels lit)."""
    bm = L.LightSource(sigma_in, sigma_out, pn, NA, device=dev).generateAnnular()
    if keep is not None:
        bm = subsample_bitmap(bm.cpu(), keep).to(dev)
    ax = (torch.arange(pn, dtype=torch.float32, device=dev) - pn // 2) * (4.0 / pn)
    r2 = ax[:, None] ** 2 + ax[None, :] ** 2
    return scale * torch.exp(-r2 / 0.5) * bm.to(torch.float32)


@pytest.mark.parametrize("coarse", [0, 2])
def test_plan_cache_with_a_weighted_source(L, dev, nat, coarse):
    from lithographysimulator_amd.synthetic import bernoulli_mask, lines_mask
    pn = 256
    pf = L.Pupil(pn, WL, NA, f16(DEMO_AB), dev).generatePupilFunction()
    m1, m2 = L.Mask(bernoulli_mask(pn), PS, dev), L.Mask(lines_mask(pn), PS, dev)
    f1, f2 = m1.fraunhofer(WL, True), m2.fraunhofer(WL, True)
    wm = _apodised(L, dev, pn)
    kw = dict(options={"coarse": coarse}, weighted=True)
    cache = L.PlanCache()
    a1 = L.abbeImage(m1, f1, pf, wm, PS, m1.deltaK, WL, True, dev, plan_cache=cache, **kw)
    assert nat.last_plan()["planned_from_record"] == 0 and cache.valid and cache.weights is not None
    a2 = L.abbeImage(m1, f1, pf, wm, PS, m1.deltaK, WL, True, dev, plan_cache=cache, **kw)
    assert nat.last_plan()["planned_from_record"] == 1 and nat.last_plan()["coarse_grid"] == (1 if coarse else 0)
    assert torch.equal(a2, a1)
    assert torch.equal(a1, L.abbeImage(m1, f1, pf, wm, PS, m1.deltaK, WL, True, dev, **kw))       # ... and to the uncached call
    # another map of the same support: the cache notices and the image follows the new weights
    wm2 = wm * (1.0 + 0.5 * torch.sin(torch.arange(pn, device=dev, dtype=torch.float32))[None, :] ** 2)
    assert torch.equal(wm2 > 0, wm > 0)
    b1 = L.abbeImage(m1, f1, pf, wm2, PS, m1.deltaK, WL, True, dev, plan_cache=cache, **kw)
    assert nat.last_plan()["planned_from_record"] == 0
    fresh = L.abbeImage(m1, f1, pf, wm2, PS, m1.deltaK, WL, True, dev, **kw)
    assert torch.equal(b1, fresh) and not torch.equal(b1, a1)
    # an in-place change of the same tensor is noticed too (version counter)
    wm2.mul_(0.5)
    b2 = L.abbeImage(m1, f1, pf, wm2, PS, m1.deltaK, WL, True, dev, plan_cache=cache, **kw)
    assert rel_max(b2, 0.5 * fresh) < 1e-6
    # a planned weighted call captured in a HIP graph replays to the same image, also for another mask spectrum
    e1 = L.abbeImage(m1, f1, pf, wm2, PS, m1.deltaK, WL, True, dev, plan_cache=cache, **kw)
    e2 = L.abbeImage(m2, f2, pf, wm2, PS, m2.deltaK, WL, True, dev, plan_cache=cache, **kw)
    assert nat.last_plan()["planned_from_record"] == 1
    static = f1.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        L.abbeImage(m1, static, pf, wm2, PS, m1.deltaK, WL, True, dev, plan_cache=cache, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = L.abbeImage(m1, static, pf, wm2, PS, m1.deltaK, WL, True, dev, plan_cache=cache, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, e1)
    static.copy_(f2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, e2) and not torch.equal(e1, e2)


# ---- 8: drop-in level -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", [128, 256])
def test_abbe_image_weighted_vs_oracle(L, dev, nat, pn):
    """abbeImage(weighted=True) on a Gaussian-apodised annulus (40 lit pixels, so that the float64 truth stays cheap) against
    oracle.post_process(sum_s w_s |E_s|^2); normalize=True divides by sum_s w_s; weighted=False on the same tensor is the
    reference's bitmap semantics -- the int64 cast -- exactly."""
    from lithographysimulator_amd.synthetic import bernoulli_mask
    mask = L.Mask(bernoulli_mask(pn), PS, dev)
    mft = mask.fraunhofer(WL, True)
    eps, N = mask.calculateEpsilonN(mask.deltaK, PS, WL)
    pf = L.Pupil(pn, WL, NA, None if pn == 256 else f16(DEMO_AB), dev).generatePupilFunction()
    wm = _apodised(L, dev, pn, keep=40, scale=3.0)                             # values in (0, 3): some below 1
    sh, w = L.sourceWeights(wm, pn)
    assert sh.shape[0] == 40 and float(w.min()) > 0 and float(w.min()) < 1 < float(w.max())
    truth_raw = _truth(pf, mft, sh, w, N)
    want = O().post_process(truth_raw.to(torch.float32), eps)
    opts = {"coarse": 2}
    img = L.abbeImage(mask, mft, pf, wm, PS, mask.deltaK, WL, True, dev, options=opts, weighted=True)
    assert nat.last_plan()["coarse_grid"] == (1 if pn == 256 else 0)           # the coarse grid exists from 256^2 up
    _check(f"abbeImage weighted, pn {pn}", img, want)
    norm = L.abbeImage(mask, mft, pf, wm, PS, mask.deltaK, WL, True, dev, options=opts, weighted=True, normalize=True)
    _check(f"abbeImage weighted normalised, pn {pn}", norm, want / float(w.double().sum()))
    # the default is untouched: a float tensor is still cast to int64 (values below 1 are dropped, the others count once)
    as_bitmap = L.abbeImage(mask, mft, pf, wm, PS, mask.deltaK, WL, True, dev, options=opts)
    expect = L.abbeImage(mask, mft, pf, wm.to(torch.int64), PS, mask.deltaK, WL, True, dev, options=opts)
    assert 0 < int((wm.to(torch.int64) != 0).sum()) < 40
    assert torch.equal(as_bitmap, expect) and not torch.equal(as_bitmap, img)


# ---- 9: invalid weights ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["array", "counted", "planned"])
def test_invalid_weights_are_an_error_of_the_planning_call(L, dev, nat, bad, where):
    from lithographysimulator_amd.imageformation import ShapeError
    mft, pf, sel, w, truth = _problem(L, dev, 128, 256, "demo")
    wb = w.clone()
    wb[17] = bad
    out = torch.full((128, 128), 7.0, dtype=torch.float32, device=dev)
    kw = {}
    if where == "counted":
        kw["count"] = torch.tensor([sel.shape[0]], dtype=torch.int32, device=dev)
    if where == "planned":
        kw["plan"] = L.PlanCache()
    with pytest.raises(ValueError):
        L.abbeIntensity(mft, pf, sel, 256, out=out, weights=wb, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))                         # nothing was accumulated
    if where == "planned":
        assert not kw["plan"].valid                                            # the failed call left no record behind
    # w = 0 is legal and contributes nothing
    wz = w.clone()
    wz[17] = 0.0
    keep = torch.ones(sel.shape[0], dtype=torch.bool, device=dev)
    keep[17] = False
    got = L.abbeIntensity(mft, pf, sel, 256, weights=wz)
    want = L.abbeIntensity(mft, pf, sel[keep].contiguous(), 256, weights=w[keep].contiguous())
    assert rel_max(got, want) < 1e-6
    # wrong shape / dtype / device are ShapeErrors before any launch
    for wrong in (w[:-1], w.double(), w.cpu(), w[:, None]):
        with pytest.raises(ShapeError):
            L.abbeIntensity(mft, pf, sel, 256, weights=wrong)


# ---- 10: two ranks sharing cuda:0 over gloo ----------------------------------------------------------------------------------
TWO_RANK = textwrap.dedent("""
    import math, os, sys, torch, torch.distributed as dist
    sys.path.insert(0, %r)
    rank = int(os.environ["RANK"])
    dist.init_process_group("gloo", rank=rank, world_size=2)
    dev = torch.device("cuda", 0)
    import lithographysimulator_amd as L
    from lithographysimulator_amd.synthetic import bernoulli_mask
    W = dist.group.WORLD
    pn = 256
    m = L.Mask(bernoulli_mask(pn), 25, dev); mft = m.fraunhofer(193., True)
    bm = L.LightSource(0.0, 0.5, pn, 0.7, device=dev).generateAnnular()                 # config 1's source: S = 3233 (odd)
    ax = (torch.arange(pn, dtype=torch.float32, device=dev) - pn // 2) * (4.0 / pn)
    wm = torch.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / 0.2) * bm.to(torch.float32)
    pf = L.Pupil(pn, 193., 0.7, None, dev).generatePupilFunction()
    res = []
    for norm in (False, True):
        sharded = L.abbeImage(m, mft, pf, wm, 25, m.deltaK, 193., True, dev, group=W, weighted=True, normalize=norm)
        whole = L.abbeImage(m, mft, pf, wm, 25, m.deltaK, 193., True, dev, weighted=True, normalize=norm)
        d = (sharded - whole).double()
        res += [float(d.abs().max() / whole.max()), float(torch.linalg.norm(d) / torch.linalg.norm(whole.double()))]
    unweighted = L.abbeImage(m, mft, pf, bm, 25, m.deltaK, 193., True, dev)
    torch.cuda.synchronize()
    print("RESULT", rank, *res, float(whole.double().sum()), float((wm > 0).sum()), float(whole.max() / unweighted.max()))
    dist.barrier()
    dist.destroy_process_group()
""") % ROOT


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_share_one_gpu_over_gloo_weighted():
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, "-c", TWO_RANK], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              cwd=ROOT, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                                                 RANK=str(r), WORLD_SIZE="2"))
             for r in range(2)]
    outs = []
    try:
        for p in procs:                                    # each rank's process under its own time limit
            outs.append(p.communicate(timeout=600))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    for so, _ in outs:
        f = [float(v) for v in [l for l in so.splitlines() if l.startswith("RESULT")][0].split()[2:]]
        print("two ranks, weighted: sharded vs whole max / l2", f[:2], "normalised", f[2:4])
        assert f[0] < TOL_IMAGE_MAX and f[1] < TOL_IMAGE_L2 and f[2] < TOL_IMAGE_MAX and f[3] < TOL_IMAGE_L2, f
        assert f[5] == 3233 and 0 < f[6] < 1                                   # a normalised grey-level image of config 1's source
