"""Where the forward-mode imaging entry points read and write: litho_socs_jvp, litho_measure_epe_jvp and litho_measure_cd_jvp
through the raw C ABI inside tests/arena.py's guarded, 0xFF-poisoned arena, with the runs of tests/test_gpu_resist_memory.py
(imported, not copied):

  a  no guard byte and no input byte changes;
  b  every element of every output is written;
  c  the outputs equal the wrappers' results bit for bit, also in a second call into the used (dirty) workspace;
  d  the same bits with every buffer 8 (complex64) or 4 (fp32) bytes past a 16-byte boundary, all at once and one at a time;
  e  the same bits on a side stream;
  f  a workspace one byte short launches nothing: the output and the workspace are still poison.

The workspace is exactly litho_socs_jvp_work_bytes long, so its last plane ends at the guard.  Shapes: pn 16 and 64, N = pn and
4 pn, K = 3, two groups, P = 1 and 16."""
import numpy as np
import pytest
import torch

import socs_grad_oracle as GO
import socs_tangent_oracle as TO
import test_gpu_resist_memory as RM

pytestmark = pytest.mark.gpu

dev, L, nat, side = RM.dev, RM.L, RM.nat, RM.side                                 # the fixtures
K, GROUPS = 3, 2
SHAPES = [(16, 16), (16, 64), (64, 64), (64, 256)]
DIRECTIONS = [1, 16]


def jvp_case(L, nat, dev, pn, N, P):
    k, M, _ = GO.sized_case(pn, N, K, GROUPS)
    dM = TO.directions(M, P, 40 + pn + P)
    kd, Md, dMd = k.to(dev).reshape(GROUPS * K, pn, pn).contiguous(), M.to(dev), dM.to(dev)
    want = RM.memo(("socs jvp", pn, N, P), lambda: L.hopkinsTangent(Md, GO.socs_around(k, dev), N, dMd))
    need = int(nat.lib().litho_socs_jvp_work_bytes(GROUPS, K, P, pn))
    assert need == 2 * GROUPS * K * pn * pn * 8 + GROUPS * pn * pn * 4            # two field stacks and one direction's planes

    def call(p, st):
        return nat.lib().litho_socs_jvp(p["kernels"], p["mask"], p["dmask"], P, GROUPS, K, pn, N, p["dI"], 0, p["work"], p["work_bytes"], st)
    return RM.Case("litho_socs_jvp", (pn, N), f"P {P}", [("kernels", kd), ("mask", Md), ("dmask", dMd)], {"dI": want}, call,
                   (pn * pn + pn + 4) * 8, work_bytes=need, mod=8)


def _images(dev, n, P):
    image, dimage = TO.smooth_pair(n, 50 + n, planes=2, P=P)
    return torch.from_numpy(image).to(dev), torch.from_numpy(dimage).to(dev)


def epe_jvp_case(L, nat, dev, n, P):
    img, dimg = _images(dev, n, P)
    rng = np.random.default_rng(n)
    ang = rng.uniform(0, 2 * np.pi, 37)
    sites = np.stack([rng.uniform(0, n - 1, 37), rng.uniform(0, n - 1, 37), np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
    sites[0, 0] = np.nan
    st = torch.from_numpy(sites).to(dev)
    gains = (0.8, 1.0, 1.25)
    want = RM.memo(("epe jvp", n, P), lambda: L.measureEPETangent(img, dimg, 0.5, st, 25.0, doses=gains, searchRange=6.0))
    g = RM.floats(gains)

    def call(p, s):
        return nat.lib().litho_measure_epe_jvp(p["image"], p["dimage"], P, 2, n, p["sites"], 37, g, 3, 0.5, 1, 6.0, 25.0, p["out"], s)
    return RM.Case("litho_measure_epe_jvp", (n,), f"P {P}", [("image", img), ("dimage", dimg), ("sites", st)], {"out": want}, call,
                   RM.guard_bytes(n))


def cd_jvp_case(L, nat, dev, n, P):
    img, dimg = _images(dev, n, P)
    rng = np.random.default_rng(2 * n)
    gauges = [(int(r), int(c), int(a)) for r, c, a in zip(rng.integers(0, n, 29), rng.integers(0, n, 29), rng.integers(0, 2, 29))]
    gauges += [(0, 0, 0), (n - 1, n - 1, 1), (n, 0, 0), (1, 1, 2)]
    gt = torch.tensor(gauges, dtype=torch.int32, device=dev)
    gains = (0.8, 1.0, 1.25)
    want = RM.memo(("cd jvp", n, P), lambda: L.measureCDTangent(img, dimg, gt, 0.5, 25.0, doses=gains))
    g = RM.floats(gains)

    def call(p, s):
        return nat.lib().litho_measure_cd_jvp(p["image"], p["dimage"], P, 2, n, p["gauges"], len(gauges), g, 3, 0.5, 1, 25.0, p["out"], s)
    return RM.Case("litho_measure_cd_jvp", (n,), f"P {P}", [("image", img), ("dimage", dimg), ("gauges", gt)], {"out": want}, call,
                   RM.guard_bytes(n))


# ---- a-d -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", DIRECTIONS)
@pytest.mark.parametrize("pn,N", SHAPES)
def test_socs_jvp(L, nat, dev, pn, N, P):
    RM.run(nat, dev, jvp_case(L, nat, dev, pn, N, P))


@pytest.mark.parametrize("P", DIRECTIONS)
@pytest.mark.parametrize("n", [16, 64])
def test_measure_epe_jvp(L, nat, dev, n, P):
    RM.run(nat, dev, epe_jvp_case(L, nat, dev, n, P))


@pytest.mark.parametrize("P", DIRECTIONS)
@pytest.mark.parametrize("n", [16, 64])
def test_measure_cd_jvp(L, nat, dev, n, P):
    RM.run(nat, dev, cd_jvp_case(L, nat, dev, n, P))


# ---- e ---------------------------------------------------------------------------------------------------------------------------
def test_on_a_side_stream(L, nat, dev, side):
    for case in (jvp_case(L, nat, dev, 16, 64, 16), jvp_case(L, nat, dev, 64, 64, 1), epe_jvp_case(L, nat, dev, 64, 16),
                 cd_jvp_case(L, nat, dev, 64, 16)):
        RM.run(nat, dev, case, side)


# ---- f ---------------------------------------------------------------------------------------------------------------------------
def test_a_refused_workspace_launches_nothing(L, nat, dev):
    case = jvp_case(L, nat, dev, 16, 64, 16)
    a = case.arena(dev, {}, work_bytes=case.work_bytes - 1)
    rc, _ = RM.invoke(nat, dev, case, a)
    assert rc == nat.E_WORKSPACE
    rep = a.report(case.outs)
    untouched = a.still_poison("dI") and a.still_poison("work")
    print(f"litho_socs_jvp, workspace one byte short: return code {rc}; output and workspace {'still poison' if untouched else 'TOUCHED'}")
    assert untouched and not rep.guards and not rep.inputs
