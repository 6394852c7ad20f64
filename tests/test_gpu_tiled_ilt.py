"""Tiled inverse lithography on the GPU: litho_socs_vjp_batch (csrc/socs_grad.hip) against socs_grad_oracle.gradient tile by tile,
its bit promises on both routes (the fused sum up to pn 2048, the stored adjoints at 4096), hopkinsGradientBatch against
hopkinsGradient; litho_tiles_cut / litho_tiles_overlap_add / litho_tiles_unstitch (csrc/tiling.hip) bit for bit against
tests/tiled_ilt_oracle.py; one iterate of optimizeMaskTiled against the oracle's tiled loss and gradient, a short run, and the
wrappers' errors.

Shapes of the batch entry: where the row pass changes shape (plane_fft.hpp LineShape: T = pn / 16 threads per line, L = 64 / T
lines per workgroup, so a workgroup's sums cover several tiles' rows at pn 16), N / pn = 1 ... 64, and the two routes."""
import numpy as np
import pytest
import torch

import socs_grad_oracle as GO
import tiled_ilt_oracle as TI
from test_gpu_tiling import _socs, random_kernels, spectra

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    import lithographysimulator_amd as L
    return L


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    assert _native.lib().litho_target_arch() == b"gfx950"
    return _native


def grads_of(tiles, groups, pn, seed):
    """fp32 [tiles,groups,pn,pn]: GO.random_G per tile."""
    return torch.stack([GO.random_G((groups, pn, pn), seed + 13 * b) for b in range(tiles)])


def vjp_batch(nat, dev, kernels, specs, G, N, out=None, accumulate=0):
    """The raw entry on device tensors: kernels [groups,K,pn,pn], specs [tiles,pn,pn], G [tiles,groups,pn,pn] -> complex64
    [tiles,pn,pn]."""
    groups, K, pn = kernels.shape[0], kernels.shape[1], kernels.shape[-1]
    tiles = specs.shape[0]
    lib = nat.lib()
    need = int(lib.litho_socs_vjp_batch_work_bytes(tiles, groups, K, pn))
    assert need == tiles * groups * K * pn * pn * 8 + tiles * groups * pn * pn * 4
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.full((tiles, pn, pn), float("nan"), dtype=torch.complex64, device=dev)
    k, m, g = kernels.contiguous(), specs.contiguous(), G.contiguous()
    with torch.cuda.device(dev):
        rc = lib.litho_socs_vjp_batch(nat.ptr(k), nat.ptr(m), nat.ptr(g), tiles, groups, K, pn, N, nat.ptr(out), accumulate,
                                      nat.ptr(work), need, nat.stream_ptr(dev))
    assert rc == nat.LITHO_OK, rc
    return out


# ---- the batched gradient against the oracle ---------------------------------------------------------------------------------------
BATCH_CASES = [(16, 16, 1, 1, 1), (16, 64, 5, 2, 3), (16, 1024, 3, 1, 2), (32, 64, 3, 2, 3), (128, 256, 5, 1, 3), (512, 512, 3, 2, 2),
               (1024, 2048, 3, 1, 2), (2048, 2048, 1, 1, 1), (4096, 4096, 1, 1, 2)]


@pytest.mark.parametrize("pn,N,K,groups,tiles", BATCH_CASES)
def test_gradient_batch_against_the_oracle(nat, dev, pn, N, K, groups, tiles):
    k, M, G = random_kernels(pn, groups, K), spectra(pn, tiles), grads_of(tiles, groups, pn, pn + N)
    got = vjp_batch(nat, dev, k.to(dev), M.to(dev), G.to(dev), N).cpu()
    worst = (0.0, 0.0)
    for b in range(tiles):
        want = GO.gradient(k, M[b], N, G[b])
        e = (GO.rel_max(got[b], want), GO.rel_l2(got[b], want))
        del want
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
        print(f"litho_socs_vjp_batch pn {pn} N {N} K {K} groups {groups} tile {b} of {tiles}: rel-to-max {e[0]:.2e} (bound "
              f"{GO.TOL_GRAD_MAX:.0e}), rel-L2 {e[1]:.2e} (bound {GO.TOL_GRAD_L2:.0e})")
        assert e[0] <= GO.TOL_GRAD_MAX and e[1] <= GO.TOL_GRAD_L2, (pn, N, K, b, e)


# ---- bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,N", [(16, 32), (32, 64), (512, 512), (1024, 1024), (4096, 4096)])
def test_a_tiles_bits_are_its_own(L, nat, dev, pn, N):
    K, tiles = 4, 2 if pn == 4096 else 3
    k, M, G = random_kernels(pn, 1, K).to(dev), spectra(pn, tiles).to(dev), grads_of(tiles, 1, pn, 5 * pn).to(dev)
    whole = vjp_batch(nat, dev, k, M, G, N)
    assert bool(torch.isfinite(torch.view_as_real(whole)).all())
    assert torch.equal(vjp_batch(nat, dev, k, M, G, N), whole)                     # two calls, equal bits
    for b in range(tiles):
        assert torch.equal(vjp_batch(nat, dev, k, M[b:b + 1], G[b:b + 1], N)[0], whole[b]), ("alone", b)
    order = [1, 0] if tiles == 2 else [2, 0, 1]
    moved = vjp_batch(nat, dev, k, M[order], G[order], N)
    assert all(torch.equal(moved[i], whole[j]) for i, j in enumerate(order))
    # the wrapper: the default (one call) against the raw entry, tileChunk 1 and 2 against the default
    socs = GO.socs_around(k[0].cpu(), dev)
    default = L.hopkinsGradientBatch(M, socs, N, G[:, 0])
    assert torch.equal(default, whole)
    for chunk in (1, 2):
        assert torch.equal(L.hopkinsGradientBatch(M, socs, N, G[:, 0], tileChunk=chunk), default), chunk
    # accumulate: K / 2 kernels, then the other half into the same gradients, is the one call on all K
    first = vjp_batch(nat, dev, k[:, :2], M, G, N)
    both = vjp_batch(nat, dev, k[:, 2:], M, G, N, out=first.clone(), accumulate=1)
    assert torch.equal(both, whole) and not torch.equal(first, whole)
    # and `out=` of the wrapper adds to what is there
    twice = L.hopkinsGradientBatch(M, socs, N, G[:, 0], out=default.clone())
    again = vjp_batch(nat, dev, k, M, G, N, out=whole.clone(), accumulate=1)
    assert torch.equal(twice, again) and not torch.equal(twice, whole)


def test_the_batch_agrees_with_the_single_gradient_route(L, dev):
    """hopkinsGradient (natural-layout fields, a reduction kernel) and the batch entry compute one gradient in two orders of
    transforms: equal under the gradient tolerances, not bit for bit."""
    pn, N = 64, 128
    k, M, G = random_kernels(pn, 2, 5), spectra(pn, 2).to(dev), grads_of(2, 2, pn, 77).to(dev)
    socs = GO.socs_around(k, dev)
    batch = L.hopkinsGradientBatch(M, socs, N, G)
    for b in range(2):
        single = L.hopkinsGradient(M[b], socs, N, G[b])
        e = (GO.rel_max(batch[b], single), GO.rel_l2(batch[b], single))
        print(f"hopkinsGradientBatch against hopkinsGradient, tile {b}: rel-to-max {e[0]:.2e}, rel-L2 {e[1]:.2e}")
        assert e[0] <= GO.TOL_GRAD_MAX and e[1] <= GO.TOL_GRAD_L2


# ---- cut, overlap-add, unstitch -----------------------------------------------------------------------------------------------------
# (nx, ny, pn, halo): halo 0, halo < core, halo > core (a pixel in up to 25 windows), and planes of 140 x 210 and 1 x 1 tile
GEOMETRIES = [(3, 2, 8, 0), (3, 2, 12, 3), (3, 2, 10, 4), (3, 2, 80, 5), (1, 1, 12, 3)]


def _complex(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize("nx,ny,pn,halo", GEOMETRIES)
def test_cut_and_overlap_add(L, dev, nx, ny, pn, halo):
    core = pn - 2 * halo
    rows, cols = ny * core, nx * core
    place = TI.plan_place(nx, ny, core)
    pl = torch.from_numpy(place).to(dev)
    rng = np.random.default_rng(pn + halo)
    plane, windows = _complex(rng, (rows, cols)), _complex(rng, (nx * ny, pn, pn))
    fill = 0.25 - 0.5j
    got = L.cutTiles(torch.from_numpy(plane).to(dev), pl, pn, halo, fill).cpu().numpy()
    assert np.array_equal(got.view(np.int32), TI.cut(plane, place, pn, halo, np.complex64(fill)).view(np.int32))
    back = L.overlapAddTiles(torch.from_numpy(windows).to(dev), pl, halo, rows, cols).cpu().numpy()
    want = TI.overlap_add(windows, place, halo, rows, cols)
    assert want.dtype == np.complex64 and np.array_equal(back.view(np.int32), want.view(np.int32))
    # a permuted tile list is another order of the sum: the kernel follows the list, as the oracle does
    perm = np.arange(nx * ny)[::-1].copy()
    back = L.overlapAddTiles(torch.from_numpy(windows[perm]).to(dev), pl[torch.from_numpy(perm).to(dev)], halo, rows, cols).cpu().numpy()
    assert np.array_equal(back.view(np.int32), TI.overlap_add(windows[perm], place[perm], halo, rows, cols).view(np.int32))


@pytest.mark.parametrize("nx,ny,pn,halo", GEOMETRIES)
def test_unstitch(L, dev, nx, ny, pn, halo):
    core, planes = pn - 2 * halo, 2
    nt, j0 = (pn, 0) if halo == 0 else (pn - 1, halo - 1)
    n = core * max(nx, ny)
    place = TI.plan_place(nx, ny, core)
    image = np.random.default_rng(pn).standard_normal((planes, n, n)).astype(np.float32)
    got = L.unstitchTiles(torch.from_numpy(image).to(dev), torch.from_numpy(place).to(dev), nt, j0, core).cpu().numpy()
    assert np.array_equal(got.view(np.int32), TI.unstitch(image, place, nt, j0, core).view(np.int32))


def test_unstitch_of_clipped_tiles(L, dev):
    place = np.array([(-2, 0), (3, 4), (40, 0)], dtype=np.int32)
    image = np.random.default_rng(9).standard_normal((1, 6, 6)).astype(np.float32)
    got = L.unstitchTiles(torch.from_numpy(image).to(dev), torch.from_numpy(place).to(dev), 7, 1, 4).cpu().numpy()
    assert np.array_equal(got, TI.unstitch(image, place, 7, 1, 4)) and (got[2] == 0).all() and (got[0] != 0).any()


# ---- one iterate of the tiled loop --------------------------------------------------------------------------------------------------
def _tiled(L, case, socs, **kw):
    return L.optimizeMaskTiled(case.target, socs, case.plan, case.threshold, dose=GO.ILT_DOSE, iterations=1, step=GO.ILT_STEP,
                               maskSteepness=GO.ILT_MASK_STEEPNESS, background=case.background, initial=case.theta0, **kw)


@pytest.mark.parametrize("pn,halo,ps,kind,planes", TI.ILT_TILED_CASES)
def test_one_iterate_against_the_oracle(L, dev, pn, halo, ps, kind, planes):
    case = TI.tiled_case(pn, halo, ps, kind, planes)
    if pn == 32 and ps == 25.0:
        assert (case.plan.n_tile, case.plan.j0) == (30, 7)                         # the crop regime
    socs = GO.socs_around(case.kernels if planes > 1 else case.kernels[0], dev, GO.ILT_WEIGHT_SUM)
    got = _tiled(L, case, socs)
    l0, l1, update = case.reference()
    assert got.best == 1 and got.plan is case.plan and tuple(got.theta.shape) == (case.rows, case.cols)
    up = (case.theta0.double() - got.theta.cpu().double()) / GO.ILT_STEP
    e = (abs(got.losses[0] - l0) / l0, abs(got.losses[1] - l1) / l1, float((up - update).abs().max()))
    print(f"optimizeMaskTiled pn {pn} halo {halo} pixel {ps:g} {kind} planes {planes}: losses {got.losses[0]:.6f} -> {got.losses[1]:.6f}, "
          f"relative error {e[0]:.2e}, {e[1]:.2e} (bound {TI.TOL_TILED_LOSS:.1e}); update {e[2]:.2e} (bound {TI.TOL_TILED_UPDATE:.1e})")
    assert e[0] <= TI.TOL_TILED_LOSS and e[1] <= TI.TOL_TILED_LOSS and e[2] <= TI.TOL_TILED_UPDATE
    for chunk in (1, 4):
        other = _tiled(L, case, socs, tileChunk=chunk)
        assert other.losses == got.losses and torch.equal(other.theta, got.theta), chunk


def test_recomputed_spectra_change_no_bit(L, dev, monkeypatch):
    """Spectra kept from the forward sweep, or recomputed because they would not fit under STACK_BYTES: the same bits."""
    from lithographysimulator_amd import socs as S
    case = TI.tiled_case(32, 8, TI.PS_EPS1, "attenuated", 1)
    socs = GO.socs_around(case.kernels[0], dev, GO.ILT_WEIGHT_SUM)
    kept = _tiled(L, case, socs, tileChunk=2)
    monkeypatch.setattr(S, "STACK_BYTES", 3 * 32 * 32 * 8)                         # room for three of the six spectra
    again = _tiled(L, case, socs, tileChunk=2)
    assert again.losses == kept.losses and torch.equal(again.theta, kept.theta)


def test_a_short_run_lowers_the_loss(L, nat, dev):
    """Eight iterations at pn 64, 2 x 2 tiles with cores of 32: two contacts, one across the vertical core boundary and one across
    the horizontal one."""
    pn, halo, ps = 64, 16, TI.PS_EPS1
    socs = _socs(L, dev)
    core = pn - 2 * halo
    plan = L.planTiles((0.0, 0.0, 2 * core * ps, 2 * core * ps), pn, ps, TI.WL, halo)
    assert (plan.nx, plan.ny, plan.n) == (2, 2, 64)
    target = torch.zeros((plan.n, plan.n), dtype=torch.float32, device=dev)
    target[10:18, 28:36] = 1.0
    target[28:36, 42:50] = 1.0
    open_spec = L.Mask(torch.ones((pn, pn), dtype=torch.int16), ps, dev).fraunhofer(TI.WL, True)
    N = nat.epsilon_n(4.0 / pn, ps, TI.WL)[1]
    clear = float(L.hopkinsIntensityBatch(open_spec[None], socs, N)[0, pn // 2, pn // 2]) / socs.weight_sum
    res = L.optimizeMaskTiled(target, socs, plan, 0.3 * clear, iterations=8)
    print("optimizeMaskTiled, 8 iterations, two contacts across core boundaries: losses " + " ".join(f"{v:.5f}" for v in res.losses))
    assert len(res.losses) == 9 and res.best > 0 and res.losses[res.best] < res.losses[0]
    assert tuple(res.mask.shape) == (64, 64) and res.transmission.dtype == torch.complex64
    polys = L.maskPolygons(plan, res)
    assert len(polys) >= 1 and all(q[:, 0].min() >= 0.0 and q[:, 0].max() <= 64 * ps for q in polys)


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_wrong_arguments_raise_before_any_launch(L, dev):
    from lithographysimulator_amd.imageformation import ShapeError
    pn = 32
    k = random_kernels(pn, 2, 3)
    socs, M, G = GO.socs_around(k, dev), spectra(pn, 2).to(dev), grads_of(2, 2, pn, 1).to(dev)
    for bad in (dict(maskFTs=M[0]), dict(maskFTs=M.real), dict(maskFTs=M[:, :16, :16]), dict(maskFTs=M.cpu()),
                dict(G=G[:, 0]), dict(G=G[:1]), dict(G=G.to(torch.complex64)), dict(G=G.cpu()),
                dict(out=torch.zeros((2, pn, pn), dtype=torch.complex128, device=dev)),
                dict(out=torch.zeros((3, pn, pn), dtype=torch.complex64, device=dev))):
        with pytest.raises((ShapeError, ValueError)):
            L.hopkinsGradientBatch(bad.get("maskFTs", M), socs, 64, bad.get("G", G), out=bad.get("out"))
    with pytest.raises(ValueError):
        L.hopkinsGradientBatch(M, socs, 64, G, tileChunk=0)
    with pytest.raises(TypeError):
        L.hopkinsGradientBatch(M, k, 64, G)
    place = torch.tensor([(0, 0), (0, 6)], dtype=torch.int32, device=dev)
    plane = torch.zeros((6, 12), dtype=torch.complex64, device=dev)
    windows = torch.zeros((2, 12, 12), dtype=torch.complex64, device=dev)
    image = torch.zeros((1, 12, 12), dtype=torch.float32, device=dev)
    for call in (lambda: L.cutTiles(plane.real, place, 12, 3), lambda: L.cutTiles(plane, place.long(), 12, 3),
                 lambda: L.cutTiles(plane, place, 12, 6), lambda: L.cutTiles(plane, place, 12, -1), lambda: L.cutTiles(plane, place.cpu(), 12, 3),
                 lambda: L.cutTiles(plane[:4], place, 12, 3),
                 lambda: L.overlapAddTiles(windows.real, place, 3, 6, 12), lambda: L.overlapAddTiles(windows, place[:1], 3, 6, 12),
                 lambda: L.overlapAddTiles(windows, place, 6, 6, 12), lambda: L.overlapAddTiles(windows, place, 3, 0, 12),
                 lambda: L.unstitchTiles(image.double(), place, 11, 2, 6), lambda: L.unstitchTiles(image, place, 11, 6, 6),
                 lambda: L.unstitchTiles(image, place, 11, -1, 6), lambda: L.unstitchTiles(image[0], place, 11, 2, 6),
                 lambda: L.unstitchTiles(image, place, 20, 2, 13)):
        with pytest.raises((ShapeError, ValueError)):
            call()
    case = TI.tiled_case(32, 8, TI.PS_EPS1, "binary", 1)
    socs1 = GO.socs_around(case.kernels[0], dev)
    for kw in (dict(target=case.target[:-1]), dict(target=case.target.to(torch.complex64)), dict(initial=case.theta0[:-1]),
               dict(iterations=0), dict(step=0.0), dict(tileChunk=0), dict(background=1)):
        with pytest.raises((ShapeError, ValueError)):
            L.optimizeMaskTiled(kw.pop("target", case.target), socs1, case.plan, case.threshold, **{"iterations": 1, **kw})
    with pytest.raises(ShapeError):
        L.optimizeMaskTiled(case.target, GO.socs_around(random_kernels(64, 1, 3)[0], dev), case.plan, case.threshold)
    with pytest.raises(TypeError):
        L.optimizeMaskTiled(case.target, socs1, None, case.threshold)
