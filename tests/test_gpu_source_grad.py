"""Source gradients on the GPU: litho_source_sensitivity (csrc/socs_grad.hip), sourceSensitivities, sourceGradient, optimizeSource
and optimizeSourceMask, against the float64 definitions of tests/source_grad_oracle.py and against the weighted Abbe sum the
project already pins.

Regimes of the row kernel k_centred_rows<log2 pn, +1, load, store> with the rolled load and the reducing store, and the case that
reaches each (SG.ORACLE_CASES, held against the oracle; the sizes above 1024 against the engine):
  * lines per workgroup (plane_fft.hpp, LineShape): pn 16, the one-thread line, 64 lines per workgroup and no shuffle at all; pn 32
    ... 512, T = pn / 16 lanes per line reduced by shuffles inside one wave, 64 / T lines per workgroup; pn 1024, one workgroup of
    one wave per line; pn 2048 and 4096, a line of 2 and 4 waves whose sums meet in LDS (the engine tie below);
  * transforms per line: m = N / pn = 1 -- (16,16), (64,64), (256,256), (1024,1024); 1 < m <= pn -- (16,64), (32,64), (64,128),
    (128,256), (2048,4096); m > pn, where k_centred_rows skips the residues without an output -- (16,512).

Bounds: SG.TOL_SENS_MAX / TOL_SENS_L2 on max_s |d sens| / max_s |sens| and the l2 ratio (the project's image tolerances: the
complex64 floor of the formula is 7.4e-7 / 8.3e-7, under a quarter of them); the loop by four times its own complex64 floor
(SG.TOL_SMO_LOSS / TOL_SMO_UPDATE).  Every test prints what it observed (-s)."""
import ctypes
import math

import pytest
import torch

import source_grad_oracle as SG
from helpers import NA, PS, TOL_IMAGE_MAX, WL

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


def _on(dev, *tensors):
    return [t.to(dev) for t in tensors]


def _errors(got, want):
    d = got.detach().cpu().double() - want
    return float(d.abs().max() / want.abs().max()), float(torch.linalg.norm(d) / torch.linalg.norm(want))


# ---- 1: against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,N,groups,K,points", SG.ORACLE_CASES)
def test_sensitivities_against_the_oracle(L, dev, pn, N, groups, K, points):
    P, M, G, sh = SG.case(pn, N, groups, K, points)
    listed = sh.tolist()
    if points == 8:
        assert [0, 0] in listed and any(abs(a) > pn or abs(b) > pn for a, b in listed) and len({tuple(s) for s in listed}) < points
        assert any(a < 0 for a, _ in listed) and [pn // 2, -pn // 2] in listed
    want = SG.reference(pn, N, groups, K, points)
    Pd, Md, Gd, shd = _on(dev, P, M, G, sh)
    got = L.sourceSensitivities(Md, Pd, shd, N, Gd, pupilsPerPlane=K)
    assert got.dtype == torch.float32 and tuple(got.shape) == (points,)
    e_max, e_l2 = _errors(got, want)
    print(f"pn {pn} N {N} groups {groups} K {K}: max {e_max:.2e} (bound {SG.TOL_SENS_MAX:.1e}), l2 {e_l2:.2e} ({SG.TOL_SENS_L2:.1e})")
    assert e_max < SG.TOL_SENS_MAX and e_l2 < SG.TOL_SENS_L2
    if points == 8:
        assert got[2].item() == got[5].item()                                  # the duplicate, bit for bit


# ---- 2: sens[s] depends on point s alone, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("pn,N,groups,K", [(16, 64, 1, 1), (16, 16, 2, 1), (64, 128, 2, 3), (256, 256, 1, 1)])
def test_a_points_bits_do_not_depend_on_the_call(L, dev, pn, N, groups, K):
    P, M, G, sh = _on(dev, *SG.case(pn, N, groups, K, 8))
    count = sh.shape[0]
    base = L.sourceSensitivities(M, P, sh, N, G, pupilsPerPlane=K, batch=count)
    for batch in (1, 3, count, count + 5, None):
        assert torch.equal(L.sourceSensitivities(M, P, sh, N, G, pupilsPerPlane=K, batch=batch), base), batch
    perm = torch.tensor([5, 0, 7, 2, 6, 1, 4, 3], device=dev)
    for batch in (3, count):
        assert torch.equal(L.sourceSensitivities(M, P, sh[perm].contiguous(), N, G, pupilsPerPlane=K, batch=batch), base[perm])
    for s in range(count):
        alone = L.sourceSensitivities(M, P, sh[s:s + 1].contiguous(), N, G, pupilsPerPlane=K)
        assert alone.item() == base[s].item(), s
    # counts whose last workgroup holds inactive lines: at pn 16 a workgroup carries 64 lines = 4 items of one plane
    for n in (1, 2, 3, 5, 7):
        assert torch.equal(L.sourceSensitivities(M, P, sh[:n].contiguous(), N, G, pupilsPerPlane=K), base[:n]), n


# ---- 3: against the weighted Abbe sum ----------------------------------------------------------------------------------------------
def _engine_setting(L, dev, pn, points):
    from lithographysimulator_amd.synthetic import bernoulli_mask
    g = torch.Generator().manual_seed(pn)
    pf = L.Pupil(pn, WL, NA, torch.tensor([0, 0, 0, 0, 30], dtype=torch.float16), dev).generatePupilFunction()
    if pn <= 2048:
        mask = L.Mask(bernoulli_mask(pn), PS, dev)
        mft = mask.fraunhofer(WL, True)
        _, N = mask.calculateEpsilonN(mask.deltaK, PS, WL)
    else:
        # beyond the mask spectrum's own sizes at this pixel: any spectrum ties the two paths; N = pn
        mft = torch.view_as_complex(torch.randn((pn, pn, 2), generator=g, dtype=torch.float32)).to(dev)
        N = pn
    sh = L.sourceShifts(L.LightSource(0.4, 0.8, pn, NA, device=dev).generateAnnular(), pn)
    sel = sh[(torch.arange(points, device=dev) * sh.shape[0]) // points].contiguous()
    w = (0.25 + torch.rand(points, generator=g, dtype=torch.float32)).to(dev)
    G = torch.randn((pn, pn), generator=g, dtype=torch.float32).to(dev)
    return mft, pf, sel, int(N), w, G


@pytest.mark.parametrize("pn,points", [(64, 40), (256, 64), (2048, 4), (4096, 2)])
def test_sensitivities_against_the_weighted_abbe_sum(L, dev, nat, pn, points):
    """<G, abbeIntensity(weights=w)> = w . sens, the linearity the gradient rests on, with the engine's default plan (its coarse
    grid where it has one, the direct path elsewhere).  No oracle here: 2048^2 and 4096^2 are the lines of two and four waves."""
    mft, pf, sel, N, w, G = _engine_setting(L, dev, pn, points)
    I = L.abbeIntensity(mft, pf, sel, N, weights=w)
    plan = nat.last_plan()
    sens = L.sourceSensitivities(mft, pf, sel, N, G)
    lhs = float((G.double() * I.double()).sum())
    rhs = float((w.double() * sens.double()).sum())
    bound = TOL_IMAGE_MAX * float(I.max()) * float(G.double().abs().sum()) + SG.TOL_SENS_MAX * float(sens.abs().max()) * float(w.double().sum())
    print(f"pn {pn} N {N} {points} points (coarse grid {plan['coarse_grid']}): <G, I_w> {lhs:.6e}, w . sens {rhs:.6e}, difference "
          f"{abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert math.isfinite(lhs) and abs(lhs - rhs) <= bound


# ---- 4: nothing else is written --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,N,groups,K,batch", [(16, 64, 2, 3, 3), (64, 64, 1, 1, 8), (1024, 1024, 1, 1, 1)])
def test_inputs_and_canaries_are_intact(L, dev, nat, pn, N, groups, K, batch):
    points = 8 if pn < 1024 else 2
    P, M, G, sh = _on(dev, *SG.case(pn, N, groups, K, points))
    lib = nat.lib()
    nbytes = int(lib.litho_source_sensitivity_work_bytes(groups, K, batch, pn))
    assert nbytes % 8 == 0 and nbytes > 0
    pad = 64                                                                   # canary words of 4 bytes on either side
    canary = 0x5A5AA5A5
    work = torch.full((nbytes // 4 + 2 * pad,), canary, dtype=torch.int32, device=dev)
    sens = torch.full((points + 2 * pad,), canary, dtype=torch.int32, device=dev)
    before = [t.clone() for t in (P, M, G, sh)]
    with torch.cuda.device(dev):
        rc = lib.litho_source_sensitivity(nat.ptr(P), nat.ptr(M), nat.ptr(G), groups, K, nat.ptr(sh), points, pn, N,
                                          ctypes.c_void_p(sens.data_ptr() + 4 * pad), batch,
                                          ctypes.c_void_p(work.data_ptr() + 4 * pad), nbytes, nat.stream_ptr(dev))
    assert rc == nat.LITHO_OK
    torch.cuda.synchronize(dev)
    for name, a, b in zip(("pupils", "maskFT", "gradI", "shifts"), (P, M, G, sh), before):
        assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b), name
    for name, t, n in (("work", work, nbytes // 4), ("sens", sens, points)):
        assert bool((t[:pad] == canary).all()) and bool((t[pad + n:] == canary).all()), name
    got = sens[pad:pad + points].view(torch.float32)
    assert torch.equal(got, L.sourceSensitivities(M, P, sh, N, G, pupilsPerPlane=K)), "the raw call and the Python layer"


# ---- 5: the Python layer -----------------------------------------------------------------------------------------------------------
def test_source_gradient_scatters_in_argwhere_order(L, dev):
    pn, N = 64, 128
    P, M, G, _ = _on(dev, *SG.case(pn, N))
    bitmap = L.LightSource(0.3, 0.7, pn, NA, device=dev).generateAnnular()
    grey = bitmap.to(torch.float32) * 0.37
    sh = L.sourceShifts(bitmap, pn)
    sens = L.sourceSensitivities(M, P[0], sh, N, G[0])
    for cand in (bitmap, grey):
        gmap = L.sourceGradient(M, P[0], cand, N, G[0])
        assert tuple(gmap.shape) == (pn, pn) and gmap.dtype == torch.float32
        assert torch.equal(gmap[bitmap != 0], sens) and float(gmap[bitmap == 0].abs().max()) == 0.0
        idx = (sh + pn // 2).long()
        assert torch.equal(gmap[idx[:, 0], idx[:, 1]], sens)


def test_python_layer_errors(L, dev):
    from lithographysimulator_amd.imageformation import ShapeError
    z = torch.zeros((48, 48), dtype=torch.complex64, device=dev)
    sh = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="sourceSensitivities.*power of two"):
        L.sourceSensitivities(z, z, sh, 64, z.real)
    P, M, G, s8 = _on(dev, *SG.case(32, 64))
    with pytest.raises(ValueError, match="sourceSensitivities.*power of two"):
        L.sourceSensitivities(M, P, s8, 96, G)
    with pytest.raises(RuntimeError, match="smaller than the mask"):
        L.sourceSensitivities(M, P, s8, 16, G)
    with pytest.raises(ShapeError, match="sourceSensitivities"):
        L.sourceSensitivities(M, P[0, :16], s8, 64, G)
    with pytest.raises(ShapeError, match="sourceSensitivities"):
        L.sourceSensitivities(M, P, s8.reshape(4, 4), 64, G)
    with pytest.raises(ShapeError, match="sourceSensitivities"):
        L.sourceSensitivities(M, P, s8, 64, G[0, :16])
    with pytest.raises(ShapeError, match="sourceSensitivities"):
        L.sourceSensitivities(M, torch.cat([P, P]), s8, 64, G, pupilsPerPlane=3)
    with pytest.raises(ValueError, match="batch"):
        L.sourceSensitivities(M, P, s8, 64, G, batch=0)
    assert tuple(L.sourceSensitivities(M, P, s8[:0], 64, G).shape) == (0,)
    with pytest.raises(ShapeError, match="sourceGradient"):
        L.sourceGradient(M, P[0], torch.ones((16, 16), device=dev), 64, G[0])


# ---- 6: the device model of optimizeSource against the CPU chain -------------------------------------------------------------------
@pytest.mark.parametrize("pn,planes,normalize", SG.SMO_LOOP_CASES)
def test_one_iteration_of_the_device_loop_against_the_cpu_chain(L, dev, pn, planes, normalize):
    c = SG.smo_case(pn, planes, normalize)
    ref, got = c.reference(), c.loop(dev=dev)
    e_loss = max(abs(a - b) / b for a, b in zip(got.losses, ref.losses))
    e_update = float((SG.update_of(c, got) - SG.update_of(c, ref)).abs().max())
    print(f"pn {pn} planes {planes} normalize {normalize}: losses {got.losses} (oracle {ref.losses}), relative {e_loss:.2e} (bound "
          f"{SG.TOL_SMO_LOSS:.1e}); update {e_update:.2e} (bound {SG.TOL_SMO_UPDATE:.1e})")
    assert len(got.losses) == 2 and e_loss < SG.TOL_SMO_LOSS and e_update < SG.TOL_SMO_UPDATE


# ---- 7, 8: end to end ---------------------------------------------------------------------------------------------------------------
def _grating_setting(L, dev, pn, pitch=8):
    """A dense vertical line-space grating (pitch 8 pixels of 25 nm: k1 = 0.36) under a conventional disc of candidates; the
    target is the grating itself on the post-processed grid, the threshold 0.3 of the normalised clear field."""
    cols = (torch.arange(pn) % pitch) < pitch // 2
    geometry = cols[None, :].expand(pn, pn).to(torch.int16).contiguous()
    mask = L.Mask(geometry, PS, dev)
    deltaK = mask.deltaK
    pupil = L.Pupil(pn, WL, NA, None, dev).generatePupilFunction()
    disc = L.LightSource(0.0, 0.9, pn, NA, device=dev).generateAnnular()
    open_mask = L.Mask(torch.ones((pn, pn), dtype=torch.int16), PS, dev)
    clear = L.abbeImage(open_mask, open_mask.fraunhofer(WL, True), pupil, disc, PS, deltaK, WL, True, dev, normalize=True)
    n_out = clear.shape[-1]
    threshold = 0.3 * float(clear[n_out // 2, n_out // 2])
    target = torch.zeros((n_out, n_out), dtype=torch.float32, device=dev)
    k = min(pn, n_out)
    target[:k, :k] = geometry[:k, :k].to(dev).float()
    return geometry.to(dev), mask, pupil, disc, deltaK, threshold, target


def test_optimize_source_end_to_end(L, dev):
    pn = 64
    geometry, mask, pupil, disc, deltaK, threshold, target = _grating_setting(L, dev, pn)
    res = L.optimizeSource(target, geometry.to(torch.complex64), pupil, disc, PS, deltaK, WL, threshold, iterations=10)
    print(f"pn {pn}: {int(disc.sum())} candidates, losses {['%.5f' % v for v in res.losses]}, best {res.best}")
    assert len(res.losses) == 11 and res.losses[-1] < res.losses[0] and res.losses[res.best] == min(res.losses)
    assert bool(torch.isfinite(res.source).all()) and float(res.source.min()) >= 0.0
    assert res.source.dtype == torch.float32 and tuple(res.source.shape) == (pn, pn) and float(res.source[disc == 0].abs().max()) == 0.0
    image = L.abbeImage(mask, mask.fraunhofer(WL, True), pupil, res.source, PS, deltaK, WL, True, dev, normalize=True, weighted=True)
    assert bool(torch.isfinite(image).all()) and tuple(image.shape) == tuple(target.shape)
    # the returned map gives the recorded best loss through the public weighted image
    resist = torch.sigmoid((25.0 / threshold) * (image - threshold))
    loss = float(((resist - target) ** 2).mean())
    assert abs(loss - res.losses[res.best]) <= 1e-4 * res.losses[res.best], (loss, res.losses[res.best])
    socs = L.socsKernels(pupil, res.source, kernels=8)
    assert socs.K >= 1 and math.isclose(socs.weight_sum, float(res.source.double().sum()), rel_tol=1e-5)


def test_optimize_source_mask_one_round(L, dev):
    """One round at pn 32 with at least as many kernels as candidates, so that Hopkins imaging is exact and the mask stage starts
    at the loss the source stage ended with, up to the re-factorisation."""
    pn = 32
    geometry, mask, pupil, _, deltaK, threshold, target = _grating_setting(L, dev, pn)
    cand = L.LightSource(0.0, 0.5, pn, NA, device=dev).generateAnnular()
    S = int(cand.sum())
    theta0 = torch.where(geometry > 0, 1.0, -1.0).to(torch.float32)
    src, ilt = L.optimizeSourceMask(target, pupil, cand, PS, deltaK, WL, threshold, rounds=1, kernels=S, sourceIterations=5,
                                    maskIterations=5, initialTheta=theta0)
    slack = SG.TOL_SMO_LOSS * src.losses[0]
    print(f"pn {pn}, {S} candidates: source stage {src.losses[0]:.6f} -> {src.losses[src.best]:.6f}, mask stage {ilt.losses[0]:.6f} -> "
          f"{ilt.losses[ilt.best]:.6f}")
    assert src.losses[src.best] <= src.losses[0]
    assert ilt.losses[ilt.best] <= src.losses[src.best] + slack
    assert bool(ilt.mask.any()) and tuple(ilt.theta.shape) == (pn, pn)
