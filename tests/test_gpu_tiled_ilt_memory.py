"""Where the entry points of tiled inverse lithography read and write: litho_socs_vjp_batch, litho_tiles_cut,
litho_tiles_overlap_add and litho_tiles_unstitch through the raw C ABI inside tests/arena.py's guarded, 0xFF-poisoned arena, with
the runs of tests/test_gpu_resist_memory.py (imported, not copied), as tests/test_gpu_tiling_memory.py does for the image batch:

  a  no guard byte and no input byte changes;
  b  every element of every output is written;
  c  the outputs equal the wrappers' results bit for bit, also in a second call into the used (dirty) workspace;
  d  the same bits with every buffer 8 (complex64) or 4 (fp32, int32) bytes past a 16-byte boundary, all at once and one at a time;
  e  the same bits on a side stream;
  f  a workspace one byte short launches nothing: the output and the workspace are still poison.

The workspace is exactly litho_socs_vjp_batch_work_bytes long, so the transposed gradIs end at the guard.  Shapes of the batch: pn
16 and 64 (the fused route; at pn 16 one workgroup's sums span several tiles and the last workgroup is partly empty), N = pn and
4 pn, K = 3, two groups, 1 and 3 tiles; and pn 4096 with K = 1 and one tile, the unfused route (aligned, and every buffer
misaligned at once)."""
import numpy as np
import pytest
import torch

import socs_grad_oracle as GO
import test_gpu_resist_memory as RM
import test_gpu_tiled_ilt as TT
import test_gpu_tiling as GT
import tiled_ilt_oracle as TI

pytestmark = pytest.mark.gpu

dev, L, nat, side = RM.dev, RM.L, RM.nat, RM.side                                 # the fixtures
SHAPES = [(16, 16), (16, 64), (64, 64), (64, 256)]
TILES = [1, 3]


def batch_case(L, nat, dev, pn, N, tiles, K=3, groups=2):
    k = GT.random_kernels(pn, groups, K)
    M = GT.spectra(pn, tiles).to(dev)
    G = TT.grads_of(tiles, groups, pn, pn + N).to(dev)
    kd = k.to(dev).reshape(groups * K, pn, pn).contiguous()
    want = RM.memo(("gradient batch", pn, N, tiles),
                   lambda: L.hopkinsGradientBatch(M, GO.socs_around(k if groups > 1 else k[0], dev), N, G if groups > 1 else G[:, 0]))
    need = int(nat.lib().litho_socs_vjp_batch_work_bytes(tiles, groups, K, pn))
    assert need == tiles * groups * K * pn * pn * 8 + tiles * groups * pn * pn * 4

    def call(p, st):
        return nat.lib().litho_socs_vjp_batch(p["kernels"], p["masks"], p["gradIs"], tiles, groups, K, pn, N, p["grads"], 0, p["work"],
                                              p["work_bytes"], st)
    return RM.Case("litho_socs_vjp_batch", (pn, N), f"tiles {tiles}", [("kernels", kd), ("masks", M), ("gradIs", G)], {"grads": want}, call,
                   (pn * pn + pn + 4) * 8, work_bytes=need, mod=8)


# (nx, ny, pn, halo)
GEOMETRIES = {"halo 0": (3, 2, 8, 0), "halo 3": (3, 2, 12, 3), "halo over core": (3, 2, 10, 4), "core 70": (2, 2, 80, 5)}


def _geometry(dev, name):
    nx, ny, pn, halo = GEOMETRIES[name]
    core = pn - 2 * halo
    return nx, ny, pn, halo, core, torch.from_numpy(TI.plan_place(nx, ny, core)).to(dev)


def _random(dev, key, shape, dtype):
    def make():
        rng = np.random.default_rng(len(key) + int(np.prod(shape)))
        v = rng.standard_normal(shape) if dtype == np.float32 else rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        return torch.from_numpy(v.astype(dtype)).to(dev)
    return RM.memo((key, tuple(shape)), make)


def cut_case(nat, dev, name):
    from lithographysimulator_amd import tiling
    nx, ny, pn, halo, core, place = _geometry(dev, name)
    rows, cols = ny * core, nx * core
    plane = _random(dev, "plane " + name, (rows, cols), np.complex64)
    want = RM.memo(("cut", name), lambda: tiling.cutTiles(plane, place, pn, halo, 0.5 - 0.25j))

    def call(p, st):
        return nat.lib().litho_tiles_cut(p["plane"], rows, cols, p["place"], nx * ny, pn, halo, 0.5, -0.25, p["windows"], st)
    return RM.Case("litho_tiles_cut", (pn, halo), name, [("plane", plane), ("place", place)], {"windows": want}, call,
                   2 * RM.guard_bytes(max(pn, cols)), mod=8)


def overlap_case(nat, dev, name):
    from lithographysimulator_amd import tiling
    nx, ny, pn, halo, core, place = _geometry(dev, name)
    rows, cols = ny * core, nx * core
    windows = _random(dev, "windows " + name, (nx * ny, pn, pn), np.complex64)
    want = RM.memo(("overlap", name), lambda: tiling.overlapAddTiles(windows, place, halo, rows, cols))

    def call(p, st):
        return nat.lib().litho_tiles_overlap_add(p["windows"], nx * ny, pn, halo, p["place"], p["plane"], rows, cols, st)
    return RM.Case("litho_tiles_overlap_add", (pn, halo), name, [("windows", windows), ("place", place)], {"plane": want}, call,
                   2 * RM.guard_bytes(max(pn, cols)), mod=8)


def unstitch_case(nat, dev, name):
    from lithographysimulator_amd import tiling
    nx, ny, pn, halo, core, place = _geometry(dev, name)
    planes, n = 2, core * max(nx, ny)
    nt, j0 = (pn, 0) if halo == 0 else (pn - 1, halo - 1)
    image = _random(dev, "image " + name, (planes, n, n), np.float32)
    want = RM.memo(("unstitch", name), lambda: tiling.unstitchTiles(image, place, nt, j0, core))

    def call(p, st):
        return nat.lib().litho_tiles_unstitch(p["image"], n, p["place"], nx * ny, planes, nt, j0, core, p["tiles"], st)
    return RM.Case("litho_tiles_unstitch", (nt, n), name, [("image", image), ("place", place)], {"tiles": want}, call,
                   RM.guard_bytes(max(nt, n)))


# ---- a-d -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("pn,N", SHAPES)
def test_socs_vjp_batch(L, nat, dev, pn, N, tiles):
    RM.run(nat, dev, batch_case(L, nat, dev, pn, N, tiles))


def test_socs_vjp_batch_unfused_route(L, nat, dev):
    case = batch_case(L, nat, dev, 4096, 4096, 1, K=1, groups=1)
    for label, mods in case.alignments()[:2]:                                      # aligned, and everything at 8 mod 16
        RM.check(nat, dev, case, label, mods)


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_tiles_cut(nat, dev, name):
    RM.run(nat, dev, cut_case(nat, dev, name))


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_tiles_overlap_add(nat, dev, name):
    RM.run(nat, dev, overlap_case(nat, dev, name))


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_tiles_unstitch(nat, dev, name):
    RM.run(nat, dev, unstitch_case(nat, dev, name))


# ---- e ---------------------------------------------------------------------------------------------------------------------------
def test_on_a_side_stream(L, nat, dev, side):
    for case in (batch_case(L, nat, dev, 16, 64, 3), batch_case(L, nat, dev, 64, 64, 1), cut_case(nat, dev, "halo 3"),
                 overlap_case(nat, dev, "halo over core"), unstitch_case(nat, dev, "core 70")):
        RM.run(nat, dev, case, side)


# ---- f ---------------------------------------------------------------------------------------------------------------------------
def test_a_refused_workspace_launches_nothing(L, nat, dev):
    case = batch_case(L, nat, dev, 16, 64, 3)
    a = case.arena(dev, {}, work_bytes=case.work_bytes - 1)
    rc, _ = RM.invoke(nat, dev, case, a)
    assert rc == nat.E_WORKSPACE
    rep = a.report(case.outs)
    untouched = a.still_poison("grads") and a.still_poison("work")
    print(f"litho_socs_vjp_batch, workspace one byte short: return code {rc}; output and workspace {'still poison' if untouched else 'TOUCHED'}")
    assert untouched and not rep.guards and not rep.inputs
