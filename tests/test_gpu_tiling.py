"""Tiled imaging on the GPU: litho_socs_image_batch (csrc/socs_grad.hip) against socs_oracle.kernel_image, its bit promises
(a tile's bits depend on that tile alone; an accumulating call continues the sequence), its error codes; litho_tiles_stitch and
litho_tiles_seam (csrc/tiling.hip) bit for bit against numpy slicing; hopkinsImageTiled end to end against tests/tiling_oracle.py.

Shapes of the batch entry: where the row pass changes shape (plane_fft.hpp LineShape, fft_core.hpp LineFFT: T = pn / 16 threads
per line, L = 64 / T lines per workgroup) -- pn 16 (one thread per line, 64 lines per workgroup; with tiles groups pn < 64 lines
the workgroup has inactive lines), 32, 128, 256 (4 lines per workgroup), 1024 (one line per workgroup, one wave) and 2048 (the first
size with more than one wave per line); N = pn, 2 pn, 4 pn, and pn 16 at N 1024 (N / pn > pn: most residues own no output)."""
import numpy as np
import pytest
import torch

import socs_oracle as SO
import tiling_oracle as TO
from helpers import DEMO_AB, NA, TOL_IMAGE_L2, TOL_IMAGE_MAX, WL, f16, rel_l2, rel_max
from oracle import abbe_oracle as O

pytestmark = pytest.mark.gpu
PS_EPS1 = 193.0 / 8.0


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


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
_memo = {}


def spectra(pn, tiles):
    """complex64 [tiles,pn,pn]: the spectra of Bernoulli masks of different seeds through the oracle's chain."""
    from lithographysimulator_amd.synthetic import bernoulli_mask
    key = ("spectra", pn, tiles)
    if key not in _memo:
        _memo[key] = torch.stack([O.mask_spectrum(bernoulli_mask(pn, 1234 + 7 * b), 25, WL) for b in range(tiles)]).to(torch.complex64)
    return _memo[key]


def random_kernels(pn, groups, K):
    """complex64 [groups,K,pn,pn], random on the whole grid, of decaying norm."""
    key = ("kernels", pn, groups, K)
    if key not in _memo:
        g = torch.Generator().manual_seed(100 * pn + 10 * groups + K)
        k = torch.view_as_complex(torch.randn((groups, K, pn, pn, 2), generator=g, dtype=torch.float32))
        _memo[key] = (k * (0.8 ** torch.arange(K, dtype=torch.float32))[None, :, None, None]).contiguous()
    return _memo[key]


def image_batch(nat, dev, kernels, specs, N, out=None, accumulate=0):
    """The raw entry on device tensors: kernels [groups,K,pn,pn], specs [tiles,pn,pn] -> out fp32 [tiles,groups,pn,pn]."""
    groups, K, pn = kernels.shape[0], kernels.shape[1], kernels.shape[-1]
    tiles = specs.shape[0]
    lib = nat.lib()
    need = int(lib.litho_socs_image_batch_work_bytes(tiles, groups, K, pn))
    assert need == tiles * groups * K * pn * pn * 8 + tiles * groups * pn * pn * 4
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.full((tiles, groups, pn, pn), float("nan"), dtype=torch.float32, device=dev)
    k, m = kernels.contiguous(), specs.contiguous()
    with torch.cuda.device(dev):
        rc = lib.litho_socs_image_batch(nat.ptr(k), nat.ptr(m), tiles, groups, K, pn, N, nat.ptr(out), accumulate, nat.ptr(work), need,
                                        nat.stream_ptr(dev))
    assert rc == nat.LITHO_OK, rc
    return out


# ---- litho_socs_image_batch against the oracle ------------------------------------------------------------------------------------
BATCH_CASES = [(16, 16, 1, 1, 1), (16, 32, 3, 2, 3), (16, 64, 5, 1, 3), (16, 1024, 3, 2, 1),
               (32, 32, 3, 2, 1), (32, 64, 5, 1, 3), (32, 128, 1, 2, 3),
               (128, 128, 3, 1, 3), (128, 256, 5, 2, 1), (128, 512, 1, 1, 3),
               (256, 256, 1, 2, 1), (256, 512, 3, 1, 3), (256, 1024, 5, 1, 1),
               (1024, 2048, 3, 1, 1), (2048, 2048, 1, 1, 1)]


@pytest.mark.parametrize("pn,N,K,groups,tiles", BATCH_CASES)
def test_image_batch_against_the_oracle(nat, dev, pn, N, K, groups, tiles):
    k, M = random_kernels(pn, groups, K), spectra(pn, tiles)
    got = image_batch(nat, dev, k.to(dev), M.to(dev), N).cpu()
    worst = (0.0, 0.0)
    for b in range(tiles):
        for g in range(groups):
            want = SO.kernel_image(k[g], M[b], N)
            e = (rel_max(got[b, g], want), rel_l2(got[b, g], want))
            worst = (max(worst[0], e[0]), max(worst[1], e[1]))
            assert e[0] <= TOL_IMAGE_MAX and e[1] <= TOL_IMAGE_L2, (pn, N, K, b, g, e)
    print(f"litho_socs_image_batch pn {pn} N {N} K {K} groups {groups} tiles {tiles}: worst rel-to-max {worst[0]:.2e} (bound "
          f"{TOL_IMAGE_MAX:.0e}), rel-L2 {worst[1]:.2e} (bound {TOL_IMAGE_L2:.0e})")


# ---- bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn,N,groups", [(16, 32, 1), (16, 64, 2), (32, 64, 2), (256, 256, 1), (1024, 1024, 1)])
def test_a_tiles_bits_are_its_own(L, nat, dev, pn, N, groups):
    K = 4
    k, M = random_kernels(pn, groups, K).to(dev), spectra(pn, 3).to(dev)
    whole = image_batch(nat, dev, k, M, N)
    for b in range(3):
        assert torch.equal(image_batch(nat, dev, k, M[b:b + 1], N)[0], whole[b]), ("alone", b)
    moved = image_batch(nat, dev, k, M[[2, 0, 1]], N)
    assert torch.equal(moved[0], whole[2]) and torch.equal(moved[1], whole[0]) and torch.equal(moved[2], whole[1])
    # the wrapper: tileChunk = 1 and 2 against the default (one call), and against the raw entry
    import socs_grad_oracle as GO
    socs = GO.socs_around(k.cpu() if groups > 1 else k[0].cpu(), dev)
    default = L.hopkinsIntensityBatch(M, socs, N)
    assert torch.equal(default.reshape(whole.shape), whole)
    for chunk in (1, 2):
        assert torch.equal(L.hopkinsIntensityBatch(M, socs, N, tileChunk=chunk), default), chunk
    # accumulate: K / 2 kernels, then the other half into the same output, is the one call on all K
    first = image_batch(nat, dev, k[:, :2], M, N)
    both = image_batch(nat, dev, k[:, 2:], M, N, out=first.clone(), accumulate=1)
    assert torch.equal(both, whole) and not torch.equal(first, whole)
    # and `out=` of the wrapper adds to what is there
    twice = L.hopkinsIntensityBatch(M, socs, N, out=default.clone())
    again = image_batch(nat, dev, k, M, N, out=whole.clone(), accumulate=1)
    assert torch.equal(twice.reshape(whole.shape), again)


def test_the_batch_agrees_with_the_single_image_route(L, dev):
    """hopkinsIntensity (the Abbe engine and the fold) and the batch entry compute one image: equal under the image tolerances."""
    import socs_grad_oracle as GO
    pn, N = 64, 128
    k, M = random_kernels(pn, 2, 5), spectra(pn, 2).to(dev)
    socs = GO.socs_around(k, dev)
    batch = L.hopkinsIntensityBatch(M, socs, N)
    for b in range(2):
        single = L.hopkinsIntensity(M[b], socs, N)
        assert rel_max(batch[b].cpu(), single.cpu()) <= TOL_IMAGE_MAX and rel_l2(batch[b].cpu(), single.cpu()) <= TOL_IMAGE_L2


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_come_back_as_codes_and_launch_nothing(nat, dev):
    lib = nat.lib()
    poison = lambda n: torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)       # noqa: E731
    pn, K, groups, tiles = 16, 2, 2, 3
    cells = pn * pn
    kern, m, out = poison(groups * K * cells * 8), poison(tiles * cells * 8), poison(tiles * groups * cells * 4)
    need = int(lib.litho_socs_image_batch_work_bytes(tiles, groups, K, pn))
    assert need == tiles * groups * K * cells * 8 + tiles * groups * cells * 4
    work = poison(need)
    st, p = nat.stream_ptr(dev), nat.ptr

    def call(kernels=kern, masks=m, tiles=tiles, groups=groups, K=K, pn=pn, N=32, o=out, work=work, nbytes=need):
        q = lambda t: p(t) if t is not None else None                              # noqa: E731
        return lib.litho_socs_image_batch(q(kernels), q(masks), tiles, groups, K, pn, N, q(o), 0, q(work), nbytes, st)
    for kw in (dict(pn=24), dict(pn=8), dict(N=48), dict(N=8192), dict(tiles=0), dict(groups=0), dict(groups=65536), dict(K=0),
               dict(kernels=None), dict(masks=None), dict(o=None), dict(work=None), dict(tiles=1 << 30)):
        assert call(**kw) == nat.E_ARG, kw
    assert call(pn=32, N=16) == nat.E_NSMALL
    assert call(nbytes=need - 1) == nat.E_WORKSPACE
    for bad in ((0, groups, K, pn), (tiles, 0, K, pn), (tiles, 65536, K, pn), (tiles, groups, 0, pn), (tiles, groups, K, 24),
                (tiles, groups, K, 8192), (1 << 30, groups, K, pn)):
        assert int(lib.litho_socs_image_batch_work_bytes(*bad)) == 0, bad
    # the tiling kernels
    nt, core, j0, n = 12, 6, 3, 20
    t, place, img, so = poison(tiles * groups * nt * nt * 4), poison(tiles * 8), poison(groups * n * n * 4), poison(tiles * groups * 8)

    def stitch(tl=t, count=tiles, planes=groups, nt=nt, place=place, j0=j0, core=core, image=img, n=n):
        q = lambda x: p(x) if x is not None else None                              # noqa: E731
        return lib.litho_tiles_stitch(q(tl), count, planes, nt, q(place), j0, core, q(image), n, st)

    def seam(tl=t, count=tiles, planes=groups, nt=nt, nb=place, j0=j0, core=core, o=so):
        q = lambda x: p(x) if x is not None else None                              # noqa: E731
        return lib.litho_tiles_seam(q(tl), count, planes, nt, q(nb), j0, core, q(o), st)
    for kw in (dict(tl=None), dict(place=None), dict(image=None), dict(count=0), dict(planes=0), dict(nt=0), dict(core=0), dict(n=0),
               dict(j0=-1), dict(j0=7), dict(core=13)):
        assert stitch(**kw) == nat.E_ARG, kw
    for kw in (dict(tl=None), dict(nb=None), dict(o=None), dict(count=0), dict(planes=0), dict(nt=0), dict(core=0), dict(j0=0),
               dict(j0=6), dict(core=9)):
        assert seam(**kw) == nat.E_ARG, kw
    torch.cuda.synchronize(dev)
    for name, buf in (("out", out), ("work", work), ("image", img), ("seam", so)):
        assert bool((buf == 0xFF).all()), f"{name} was written by a refused call"


# ---- stitch and seam ----------------------------------------------------------------------------------------------------------------
def coded_tiles(count, planes, nt):
    """fp32 [count,planes,nt,nt] whose values are their own flat index (exact below 2^24)."""
    assert count * planes * nt * nt < 1 << 24
    return np.arange(count * planes * nt * nt, dtype=np.float32).reshape(count, planes, nt, nt)


STITCH_CASES = {
    "2x2 inside": (4, 1, 12, 3, 6, 14, [(0, 0), (0, 6), (6, 0), (6, 6)]),
    "clipped on every side, planes 2": (5, 2, 12, 2, 7, 16, [(-3, -2), (-3, 12), (12, -2), (12, 12), (4, 5)]),
    "core 1": (3, 2, 5, 2, 1, 4, [(0, 0), (3, 3), (4, 0)]),
    "a core wider than a wave, outside tiles": (4, 1, 80, 5, 70, 100, [(0, 0), (30, 70), (200, 0), (-70, 0)]),
    "j0 0, core = nt": (2, 1, 9, 0, 9, 18, [(0, 0), (9, 9)]),
}


@pytest.mark.parametrize("name", list(STITCH_CASES))
def test_stitch(nat, dev, name):
    from lithographysimulator_amd import tiling
    count, planes, nt, j0, core, n, place = STITCH_CASES[name]
    tiles = coded_tiles(count, planes, nt)
    want = TO.stitch_into(np.full((planes, n, n), -7.0, dtype=np.float32), tiles, place, j0, core)
    image = torch.full((planes, n, n), -7.0, dtype=torch.float32, device=dev)
    tiling.stitchTiles(torch.from_numpy(tiles).to(dev), torch.tensor(place, dtype=torch.int32, device=dev), j0, core, image)
    got = image.cpu().numpy()
    assert np.array_equal(got, want) and (want == -7.0).any() and (want != -7.0).any(), name


@pytest.mark.parametrize("count,planes,nt,j0,core", [(4, 1, 12, 3, 6), (5, 2, 9, 1, 1), (3, 2, 80, 4, 70), (4, 2, 20, 1, 18)])
def test_seam(nat, dev, count, planes, nt, j0, core):
    from lithographysimulator_amd import tiling
    rng = np.random.default_rng(count * 100 + nt)
    tiles = rng.uniform(-2.0, 3.0, (count, planes, nt, nt)).astype(np.float32)
    nb = np.full((count, 2), -1, dtype=np.int32)
    nb[0] = (1, 2)
    nb[1] = (-1, count - 1)
    nb[2] = (0, count)                       # a tile may be its neighbour's neighbour; `count` is outside the list: none
    want = TO.seam(tiles, nb, j0, core)
    got = tiling.seamTiles(torch.from_numpy(tiles).to(dev), torch.from_numpy(nb).to(dev), j0, core).cpu().numpy()
    assert got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.int32)[~np.isnan(want)], want.view(np.int32)[~np.isnan(want)])
    assert np.isnan(want).any() and (~np.isnan(want)).any()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _socs(L, dev, pn=64, points=12):
    key = ("socs", pn, points)
    if key not in _memo:
        pf = O.pupil_function(f16(DEMO_AB), pn, NA, WL).to(torch.complex64)
        src = SO.strided_points(O.source_annular(0.4, 0.8, pn), points)
        socs = L.socsKernels(pf.to(dev), src, kernels=points)
        assert socs.K == points and abs(socs.captured - 1.0) < 1e-4
        _memo[key] = socs
    return _memo[key]


@pytest.mark.parametrize("antialias", [1, 4])
@pytest.mark.parametrize("ps", [25.0, PS_EPS1])
def test_tiled_image_against_the_oracle(L, dev, ps, antialias):
    pn, halo = 64, 14
    core = pn - 2 * halo
    socs = _socs(L, dev)
    rects = TO.rectangles(21, 16, (3 * core, 2 * core))
    bounds = (0.0, 0.0, 3 * core * ps, 2 * core * ps)
    got = L.hopkinsImageTiled(TO.polygons_nm(rects, ps), socs, pn, ps, WL, bounds=bounds, halo=halo, antialias=antialias)
    plan = got.plan
    assert (plan.nx, plan.ny, plan.n) == (3, 2, 3 * core) and tuple(got.image.shape) == (plan.n, plan.n)
    want, seam, err, _ = TO.tiled_image(rects, socs.kernels.cpu(), plan, s=antialias)
    e = (rel_max(got.image.cpu(), want[0]), rel_l2(got.image.cpu(), want[0]))
    sm = got.seam.cpu().numpy()
    seam_gap = float(np.nanmax(np.abs(sm - seam)) / want.max())
    print(f"hopkinsImageTiled 3 x 2 tiles, pn 64, halo 14, pixel {ps:g} nm, antialias {antialias}: rel-to-max {e[0]:.2e} (bound "
          f"{TOL_IMAGE_MAX:.0e}), rel-L2 {e[1]:.2e} (bound {TOL_IMAGE_L2:.0e}); seamError {got.seamError:.5f}, oracle {err:.5f}")
    assert e[0] <= TOL_IMAGE_MAX and e[1] <= TOL_IMAGE_L2
    assert np.array_equal(np.isnan(sm), np.isnan(seam)) and seam_gap <= TOL_IMAGE_MAX
    assert abs(got.seamError - err) <= TOL_IMAGE_MAX
    assert float(got.image[2 * core:].abs().max()) == 0.0                          # the square's unused rows stay zero
    # the chunking of the driver changes no bit of the image or of the seam measure
    for chunk in (1, 4):
        other = L.hopkinsImageTiled(TO.polygons_nm(rects, ps), socs, pn, ps, WL, bounds=bounds, halo=halo, antialias=antialias,
                                    tileChunk=chunk)
        assert torch.equal(other.image, got.image) and other.seamError == got.seamError, chunk
        assert torch.equal(torch.nan_to_num(other.seam, nan=-1.0), torch.nan_to_num(got.seam, nan=-1.0)), chunk


def test_tiled_sites_measure_the_stitched_image(L, dev):
    """The existing metrology takes the stitched image unchanged: measureEPE at TiledImage.sites finds edges, and the traced
    contours come back through toLayout inside the imaged rectangle."""
    pn, halo, ps = 64, 14, PS_EPS1
    core = pn - 2 * halo
    socs = _socs(L, dev)
    rects = TO.rectangles(21, 16, (3 * core, 2 * core))
    polys = TO.polygons_nm(rects, ps)
    tiled = L.hopkinsImageTiled(polys, socs, pn, ps, WL, bounds=(0.0, 0.0, 3 * core * ps, 2 * core * ps), halo=halo)
    sites = tiled.sites(polys, 80.0)
    threshold = 0.3 * float(tiled.image.max())
    epe = L.measureEPE(tiled.image, threshold, sites, ps, searchRange=4.0).cpu().numpy()[0, 0]
    assert np.isfinite(epe[:, 0]).sum() > 10
    back = tiled.toLayout(L.traceContours(tiled.image, threshold)[0][0])
    assert len(back) > 0 and all(q[:, 0].min() > -ps and q[:, 0].max() < (3 * core + 1) * ps for q in back)
