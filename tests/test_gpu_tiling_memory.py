"""Where the entry points of tiled imaging read and write: litho_socs_image_batch, litho_tiles_stitch and litho_tiles_seam through
the raw C ABI inside tests/arena.py's guarded, 0xFF-poisoned arena, with the runs of tests/test_gpu_resist_memory.py (imported,
not copied):

  a  no guard byte and no input byte changes;
  b  every element of every output is written -- for the stitch, every element the definition writes: its reference image starts
     as the arena's poison, so a pixel outside every core must still hold it and a pixel inside one must not;
  c  the outputs equal the wrappers' results bit for bit, also in a second call into the used (dirty) workspace;
  d  the same bits with every buffer 8 (complex64) or 4 (fp32, int32) bytes past a 16-byte boundary, all at once and one at a time;
  e  the same bits on a side stream;
  f  a workspace one byte short launches nothing: the output and the workspace are still poison.

The workspace is exactly litho_socs_image_batch_work_bytes long, so the transposed images end at the guard.  Shapes: pn 16 and 64,
N = pn and 4 pn, K = 3, two groups, 1 and 3 tiles; stitch and seam with clipped and missing tiles, two planes, cores of 1, 6 and 70."""
import numpy as np
import pytest
import torch

import socs_grad_oracle as GO
import test_gpu_resist_memory as RM
import test_gpu_tiling as GT

pytestmark = pytest.mark.gpu

dev, L, nat, side = RM.dev, RM.L, RM.nat, RM.side                                 # the fixtures
K, GROUPS = 3, 2
SHAPES = [(16, 16), (16, 64), (64, 64), (64, 256)]
TILES = [1, 3]


def batch_case(L, nat, dev, pn, N, tiles):
    k = GT.random_kernels(pn, GROUPS, K)
    M = GT.spectra(pn, tiles).to(dev)
    kd = k.to(dev).reshape(GROUPS * K, pn, pn).contiguous()
    want = RM.memo(("image batch", pn, N, tiles), lambda: L.hopkinsIntensityBatch(M, GO.socs_around(k, dev), N))
    need = int(nat.lib().litho_socs_image_batch_work_bytes(tiles, GROUPS, K, pn))
    assert need == tiles * GROUPS * K * pn * pn * 8 + tiles * GROUPS * pn * pn * 4

    def call(p, st):
        return nat.lib().litho_socs_image_batch(p["kernels"], p["masks"], tiles, GROUPS, K, pn, N, p["out"], 0, p["work"], p["work_bytes"], st)
    return RM.Case("litho_socs_image_batch", (pn, N), f"tiles {tiles}", [("kernels", kd), ("masks", M)], {"out": want}, call,
                   (pn * pn + pn + 4) * 8, work_bytes=need, mod=8)


TILINGS = {"core 6": (4, 2, 12, 3, 6, 14, [(0, 0), (0, 6), (6, 0), (9, 9)]),
           "core 1": (3, 2, 5, 2, 1, 4, [(0, 0), (3, 3), (-1, 0)]),
           "core 70": (3, 1, 80, 5, 70, 100, [(0, 0), (30, 70), (200, 0)])}


def _tiles(dev, name):
    count, planes, nt = TILINGS[name][:3]
    return RM.memo(("tiles", name), lambda: torch.from_numpy(
        np.random.default_rng(nt).uniform(0.0, 2.0, (count, planes, nt, nt)).astype(np.float32)).to(dev))


def stitch_case(nat, dev, name):
    from lithographysimulator_amd import tiling
    count, planes, nt, j0, core, n, place = TILINGS[name]
    tiles, pl = _tiles(dev, name), torch.tensor(place, dtype=torch.int32, device=dev)

    def reference():
        image = torch.full((planes, n, n), -1, dtype=torch.int32, device=dev).view(torch.float32)      # the arena's poison
        return tiling.stitchTiles(tiles, pl, j0, core, image)
    want = RM.memo(("stitch", name), reference)

    def call(p, st):
        return nat.lib().litho_tiles_stitch(p["tiles"], count, planes, nt, p["place"], j0, core, p["image"], n, st)
    return RM.Case("litho_tiles_stitch", (nt, n), name, [("tiles", tiles), ("place", pl)], {"image": want}, call, RM.guard_bytes(max(nt, n)))


def seam_case(nat, dev, name):
    from lithographysimulator_amd import tiling
    count, planes, nt, j0, core = TILINGS[name][:5]
    tiles = _tiles(dev, name)
    nb = torch.tensor([(1, 2), (-1, 0), (count, 1)] + [(-1, -1)] * (count - 3), dtype=torch.int32, device=dev)
    want = RM.memo(("seam", name), lambda: tiling.seamTiles(tiles, nb, j0, core))

    def call(p, st):
        return nat.lib().litho_tiles_seam(p["tiles"], count, planes, nt, p["neighbours"], j0, core, p["out"], st)
    return RM.Case("litho_tiles_seam", (nt,), name, [("tiles", tiles), ("neighbours", nb)], {"out": want}, call, RM.guard_bytes(nt))


# ---- a-d -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("pn,N", SHAPES)
def test_socs_image_batch(L, nat, dev, pn, N, tiles):
    RM.run(nat, dev, batch_case(L, nat, dev, pn, N, tiles))


@pytest.mark.parametrize("name", list(TILINGS))
def test_tiles_stitch(nat, dev, name):
    case = stitch_case(nat, dev, name)
    RM.run(nat, dev, case)
    words = case.outs["image"].view(torch.int32)
    assert bool((words == -1).any()) and bool((words != -1).any())                 # the case has pixels of both kinds


@pytest.mark.parametrize("name", list(TILINGS))
def test_tiles_seam(nat, dev, name):
    RM.run(nat, dev, seam_case(nat, dev, name))


# ---- e ---------------------------------------------------------------------------------------------------------------------------
def test_on_a_side_stream(L, nat, dev, side):
    for case in (batch_case(L, nat, dev, 16, 64, 3), batch_case(L, nat, dev, 64, 64, 1), stitch_case(nat, dev, "core 6"),
                 seam_case(nat, dev, "core 70")):
        RM.run(nat, dev, case, side)


# ---- f ---------------------------------------------------------------------------------------------------------------------------
def test_a_refused_workspace_launches_nothing(L, nat, dev):
    case = batch_case(L, nat, dev, 16, 64, 3)
    a = case.arena(dev, {}, work_bytes=case.work_bytes - 1)
    rc, _ = RM.invoke(nat, dev, case, a)
    assert rc == nat.E_WORKSPACE
    rep = a.report(case.outs)
    untouched = a.still_poison("out") and a.still_poison("work")
    print(f"litho_socs_image_batch, workspace one byte short: return code {rc}; output and workspace {'still poison' if untouched else 'TOUCHED'}")
    assert untouched and not rep.guards and not rep.inputs
