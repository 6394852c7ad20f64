"""Where the forward-mode entry points read and write: litho_peb_expose_jvp, litho_peb_bake_jvp, litho_develop_rate_jvp and
litho_develop_time_jvp through the raw C ABI inside tests/arena.py's guarded, 0xFF-poisoned arena, with the runs and the shapes
of tests/test_gpu_resist_memory.py (imported, not copied), P = 3 directions:

  a  no guard byte and no input byte changes;
  b  every element of every output is written (no 4-byte word still holds the poison where the reference does not);
  c  the outputs equal the wrappers' results bit for bit, also in a second call into the used workspace;
  d  the same bits with the fp32 volumes 4 bytes past a 16-byte boundary, all at once and one at a time (the workspace and the
     double directions of the rate law must stay aligned: that is LITHO_E_ARG, checked in test_resist_tangent_cpu.py);
  e  the same bits on a side stream;
  f  a workspace one byte short, or at 8 mod 16, launches nothing: every output and the workspace are still poison.

The workspace is exactly what the *_work_bytes function returns, so its last volume ends at the guard."""
import ctypes

import pytest
import torch

import test_gpu_resist_memory as RM

pytestmark = pytest.mark.gpu

SHAPES, ONE_SHAPE, THICK, H, DOSES, ids = RM.SHAPES, RM.ONE_SHAPE, RM.THICK, RM.H, RM.DOSES, RM.ids
dev, L, nat, peb, side = RM.dev, RM.L, RM.nat, RM.peb, RM.side                  # the fixtures
P = 3


def doubles(values):
    return (ctypes.c_double * len(values))(*values)


def expose_jvp_case(L, nat, dev, shape, variant):
    n, D, B = shape
    doses, V = DOSES[variant], RM.image_of(dev, shape)
    dI = RM.uniform_of(dev, "dI tangent", (P, B, D, n, n))
    dC = [0.5, 0.0, -1.25]
    want = RM.memo(("expose jvp", shape, variant), lambda: L.exposeAcidTangent(V, 0.9, doses, dC, dI))
    g, dc = RM.floats(doses), doubles(dC)

    def call(p, st):
        return nat.lib().litho_peb_expose_jvp(p["image"], B, D, n, g, len(doses), 0.9, P, dc, p["dimage"], p["dacid"], st)
    return RM.Case("litho_peb_expose_jvp", shape, variant, [("image", V), ("dimage", dI)], {"dacid": want}, call, RM.guard_bytes(n))


def bake_jvp_case(L, nat, dev, shape, S, quench):
    n, D, B = shape
    r = RM.car_of(L, D, 2.0 if quench == "finite" else float("inf"))
    h0 = RM.uniform_of(dev, "h0 jvp", (B, D, n, n), 0.0, 1.0)
    dh = RM.uniform_of(dev, "dh0 jvp", (P, B, D, n, n))
    dq0 = [0.25, 0.0, -0.5]
    dstep = [[0.01, -0.02, 0.005, 0.01, 0.3, -0.02], [0.0] * 6, [-0.01, 0.0, 0.0, 0.02, -1.0, 0.01]]
    want = RM.memo(("bake jvp", shape, S, quench), lambda: L.bakeTangent(h0, r, THICK, H, dAcid=dh, dQuencher=dq0, dStep=dstep, steps=S,
                                                                        returnPrimal=True))
    need = int(nat.lib().litho_peb_jvp_work_bytes(B, D, n, P))
    assert need == (5 + 2 * P) * h0.numel() * 4
    dq, ds = doubles(dq0), doubles([v for row in dstep for v in row])
    outs = dict(zip(("dacid", "dquencher", "dacid_dose", "acid", "quencher", "acid_dose"), want))

    def call(p, st):
        return nat.lib().litho_peb_bake_jvp(p["acid_in"], B, D, n, THICK, H, r.quencher, r.kQuench, r.kLoss, r.acidDiffusionLength,
                                            r.quencherDiffusionLength, r.verticalScale, r.bakeTime, S, P, p["dacid_in"], dq, ds, p["acid"],
                                            p["quencher"], p["acid_dose"], p["dacid"], p["dquencher"], p["dacid_dose"], p["work"],
                                            p["work_bytes"], st)
    return RM.Case("litho_peb_bake_jvp", shape, f"S {S}, {quench} quench", [("acid_in", h0), ("dacid_in", dh)], outs, call, RM.guard_bytes(n),
                   work_bytes=need)


def rate_jvp_case(L, nat, dev, shape, variant):
    from lithographysimulator_amd import tangent
    n, D, B = shape
    doses, V, mk = DOSES[variant], RM.image_of(dev, shape), RM.mack_of(L)
    dx = RM.uniform_of(dev, "dx tangent", (P, B, D, n, n))
    dphi = RM.memo(("dphi", D), lambda: tangent.rateParameterTangent([[1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 2.0, -0.01, 0.3, 0.1, 0.2, -4.0],
                                                                     [0.0] * 7], mk, THICK, D).to(dev))
    want = RM.memo(("rate jvp", shape, variant), lambda: L.developmentRateTangent(V, mk, THICK, doses, dX=dx, dPhi=dphi))
    g = RM.floats(doses)

    def call(p, st):
        return nat.lib().litho_develop_rate_jvp(p["x"], B, D, n, g, len(doses), mk.C, mk.rMax, mk.rMin, mk.q, mk.mTh, mk.surfaceRate,
                                                mk.surfaceDepth, THICK, P, p["dx"], p["dphi"], p["dslowness"], st)
    return RM.Case("litho_develop_rate_jvp", shape, variant, [("x", V), ("dx", dx), ("dphi", dphi)], {"dslowness": want}, call,
                   RM.guard_bytes(n), volumes=["x", "dx", "dslowness"])


def time_jvp_case(L, nat, dev, shape, variant):
    n, D, B = shape
    s, (T, _) = RM.slowness_of(dev, shape), RM.arrival_of(L, dev, shape)

    def direction():
        ds = RM.uniform_of(dev, "ds tangent", (P, B, D, n, n)).clone()
        ds[:, RM.walls_of(s)] = float("nan")                                   # NaN on the walls: ignored
        return ds
    ds = RM.memo(("time jvp in", shape), direction)
    want, launches = RM.memo(("time jvp", shape), lambda: L.developmentTimeTangent(s, T, ds, THICK, H, returnLaunches=True))
    cap = 1024 if variant == "cap 1024" else launches
    need = int(nat.lib().litho_develop_jvp_work_bytes(B, D, n, P, cap))
    assert need == (4 * cap + 255) // 256 * 256 + (4 + P) * s.numel() * 4

    def call(p, st):
        count = ctypes.c_int(-1)
        rc = nat.lib().litho_develop_time_jvp(p["slowness"], p["T"], p["dslowness"], B, D, n, P, THICK, H, cap, p["dT"], p["work"],
                                              p["work_bytes"], ctypes.byref(count), st)
        return rc, count.value
    return RM.Case("litho_develop_time_jvp", shape, f"{variant} (max_iterations {cap})", [("slowness", s), ("T", T), ("dslowness", ds)],
                   {"dT": want}, call, RM.guard_bytes(n), work_bytes=need, launches=launches)


# ---- a-d -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(DOSES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_peb_expose_jvp(L, nat, dev, shape, variant):
    RM.run(nat, dev, expose_jvp_case(L, nat, dev, shape, variant))


@pytest.mark.parametrize("quench", ["finite", "instantaneous"])
@pytest.mark.parametrize("S", [5, 6])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_peb_bake_jvp(L, nat, dev, shape, S, quench):
    RM.run(nat, dev, bake_jvp_case(L, nat, dev, shape, S, quench))


@pytest.mark.parametrize("variant", list(DOSES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_develop_rate_jvp(L, nat, dev, shape, variant):
    RM.run(nat, dev, rate_jvp_case(L, nat, dev, shape, variant))


@pytest.mark.parametrize("variant", ["cap 1024", "cap = the launches it needs"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_develop_time_jvp(L, nat, dev, shape, variant):
    RM.run(nat, dev, time_jvp_case(L, nat, dev, shape, variant))


def all_cases(L, nat, dev, shape):
    return [expose_jvp_case(L, nat, dev, shape, "three doses"), bake_jvp_case(L, nat, dev, shape, 5, "finite"),
            rate_jvp_case(L, nat, dev, shape, "three doses"), time_jvp_case(L, nat, dev, shape, "cap 1024")]


NAMES = ["peb_expose_jvp", "peb_bake_jvp", "develop_rate_jvp", "develop_time_jvp"]


# ---- e ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4), ids=NAMES)
def test_on_a_side_stream(L, nat, dev, side, which):
    for shape in (ONE_SHAPE, (16, 5, 2)):
        RM.run(nat, dev, all_cases(L, nat, dev, shape)[which], side)


# ---- f ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [1, 3], ids=[NAMES[1], NAMES[3]])
def test_a_refused_workspace_launches_nothing(L, nat, dev, which):
    case = all_cases(L, nat, dev, ONE_SHAPE)[which]
    for label, mods, nbytes, expected in (("workspace at 8 mod 16", {"work": 8}, case.work_bytes, nat.E_ARG),
                                          ("workspace one byte short", {}, case.work_bytes - 1, nat.E_WORKSPACE)):
        a = case.arena(dev, mods, work_bytes=nbytes)
        assert a.ptr("work") % 16 == mods.get("work", 0) and a.bufs["work"].nbytes == nbytes
        rc, _ = RM.invoke(nat, dev, case, a)
        assert rc == expected, (case.entry, label, rc)
        untouched = all(a.still_poison(nm) for nm in list(case.outs) + ["work"])
        rep = a.report(case.outs)
        print(f"{case.entry} {case.shape}, {label}: return code {rc}; outputs and workspace {'still poison' if untouched else 'TOUCHED'}; "
              f"guards {'intact' if not rep.guards else rep.guards[:4]}")
        assert untouched and not rep.guards and not rep.inputs
    torch.cuda.synchronize(dev)
