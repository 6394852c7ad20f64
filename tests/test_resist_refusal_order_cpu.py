"""The ORDER in which the resist chain's entry points report what is wrong with a call, pinned without a GPU: every entry that
takes a workspace, called with two faults at once, must name the one that its checks reach first (include/litho_abbe.h):
  1. null pointers, the shape and the parameter domains                    -> LITHO_E_ARG
  2. a misaligned workspace or sum output                                    -> LITHO_E_ARG
  3. a workspace shorter than the entry's work_bytes                         -> LITHO_E_WORKSPACE
  4. a buffer the call writes over the workspace at its needed size         -> LITHO_E_ARG
with one exception: the three front solvers test their output against their inputs BEFORE the workspace's size, and they zero
*launches_host before anything else.  The pointers are fakes that are never dereferenced (every refusal comes before the first
HIP call), as in tests/test_resist_param_cpu.py and tests/test_resist_tangent_cpu.py, which pin the single refusals."""
import ctypes

import pytest

V = 4 * 4 * 64                                                                 # bytes of a [1, 4, 8, 8] volume
P, S, C = 2, 8, 3                                                              # directions, bake steps, checkpointEvery
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    return _native


def far(i):
    return ctypes.c_void_p(1 << (20 + i))                                      # 1 MiB, 2 MiB, 4 MiB, ...: far apart


def near(base, off):
    return ctypes.c_void_p(base.value + off)


BAKE = dict(thickness=100.0, pixel=25.0, q0=0.1, kq=5.0, kl=0.01, sh=20.0, sq=5.0, vs=1.0, t=60.0, steps=S)
MACK = dict(rmax=120.0, rmin=0.05, q=5.0, mth=0.4, r0=1.0, delta=1.0, thick=100.0)


def entries(nat):
    """name -> (function, the arguments of a call that passes every check, the names of its outputs, of its 16-byte aligned sum
    output or None, of an input that the solver entries test before the workspace's size or None, and a bad parameter)."""
    lib = nat.lib()
    g = (ctypes.c_float * 2)(0.8, 1.3)
    two = (ctypes.c_double * 2)(0.5, -0.5)
    dstep = (ctypes.c_double * 12)(*([0.01] * 12))
    launches = ctypes.c_int(7)
    table = {
        "litho_peb_bake": (
            dict(acid_in=far(0), B=1, D=4, n=8, **BAKE, spl=0, h=far(1), q=far(2), a=far(3), work=far(8), wb=lib.litho_peb_work_bytes(1, 4, 8)),
            ("h", "q", "a"), None, None, dict(kl=INF)),
        "litho_peb_bake_vjp": (
            dict(acid_in=far(0), B=1, D=4, n=8, **BAKE, c=C, gh=far(1), gq=far(2), ga=far(3), oh=far(4), oq=far(5), work=far(8),
                 wb=lib.litho_peb_vjp_work_bytes(1, 4, 8, S, C)),
            ("oh", "oq"), None, None, dict(q0=-0.1)),
        "litho_peb_bake_vjp_params": (
            dict(acid_in=far(0), B=1, D=4, n=8, **BAKE, c=C, gh=far(1), gq=far(2), ga=far(3), oh=far(4), oq=far(5), os=far(6), work=far(8),
                 wb=lib.litho_peb_vjp_params_work_bytes(1, 4, 8, S, C)),
            ("oh", "oq", "os"), "os", None, dict(t=0.0)),
        "litho_peb_bake_jvp": (
            dict(acid_in=far(0), B=1, D=4, n=8, **BAKE, P=P, dh=far(1), dq0=two, dstep=dstep, h=far(2), q=far(3), a=far(4), oh=far(5), oq=far(6),
                 oa=far(7), work=far(8), wb=lib.litho_peb_jvp_work_bytes(1, 4, 8, P)),
            ("h", "q", "a", "oh", "oq", "oa"), None, None, dict(kq=NAN)),
        "litho_peb_expose_vjp_params": (
            dict(image=far(0), volumes=1, D=4, n=8, gains=g, n_gains=2, C=0.05, ga=far(1), out=far(2), work=far(8),
                 wb=lib.litho_peb_expose_params_work_bytes(1, 4, 8, 2)),
            ("out",), "out", None, dict(C=0.0)),
        "litho_develop_time": (
            dict(s=far(0), B=1, D=4, n=8, thick=100.0, pixel=25.0, it=64, T=far(1), work=far(8), wb=lib.litho_develop_work_bytes(1, 4, 8, 64),
                 launches=ctypes.byref(launches)),
            ("T",), None, "s", dict(pixel=NAN)),
        "litho_develop_time_vjp": (
            dict(s=far(0), T=far(1), gT=far(2), B=1, D=4, n=8, thick=100.0, pixel=25.0, it=64, out=far(3), work=far(8),
                 wb=lib.litho_develop_vjp_work_bytes(1, 4, 8, 64), launches=ctypes.byref(launches)),
            ("out",), None, "gT", dict(thick=0.0)),
        "litho_develop_time_jvp": (
            dict(s=far(0), T=far(1), ds=far(2), B=1, D=4, n=8, P=P, thick=100.0, pixel=25.0, it=64, out=far(3), work=far(8),
                 wb=lib.litho_develop_jvp_work_bytes(1, 4, 8, P, 64), launches=ctypes.byref(launches)),
            ("out",), None, "ds", dict(it=0)),
        "litho_develop_rate_vjp_params": (
            dict(x=far(0), volumes=1, D=4, n=8, gains=g, n_gains=2, kappa=0.05, **MACK, gs=far(1), out=far(2), work=far(8),
                 wb=lib.litho_develop_rate_params_work_bytes(1, 4, 8, 2)),
            ("out",), "out", None, dict(kappa=0.0)),
    }
    return {name: (getattr(lib, name),) + row for name, row in table.items()}, launches


NAMES = ("litho_peb_bake", "litho_peb_bake_vjp", "litho_peb_bake_vjp_params", "litho_peb_bake_jvp", "litho_peb_expose_vjp_params",
         "litho_develop_time", "litho_develop_time_vjp", "litho_develop_time_jvp", "litho_develop_rate_vjp_params")


def cases(name):
    """(label, the code the combination must return, keyword overrides as a function of the passing call) of one entry."""
    solver = name.startswith("litho_develop_time")
    out = [("misaligned and short workspace", "E_ARG", lambda ok, outs, total, inp: dict(work=near(ok["work"], 4), wb=ok["wb"] - 1)),
           ("misaligned and empty workspace", "E_ARG", lambda ok, outs, total, inp: dict(work=near(ok["work"], 8), wb=0)),
           ("a bad parameter and a short workspace", "E_ARG", None),
           ("a null input and a short workspace", "E_ARG", lambda ok, outs, total, inp: {next(iter(ok)): None, "wb": ok["wb"] - 1})]
    if name in ("litho_peb_bake_vjp_params", "litho_peb_expose_vjp_params", "litho_develop_rate_vjp_params"):
        out.append(("a misaligned sum output and a short workspace", "E_ARG",
                    lambda ok, outs, total, inp: {total: near(ok[total], 8), "wb": ok["wb"] - 1}))
    if solver:
        out.append(("short workspace and the output over an input", "E_ARG", lambda ok, outs, total, inp: {outs[0]: ok[inp], "wb": ok["wb"] - 1}))
        out.append(("empty workspace and the output into an input's tail", "E_ARG",
                    lambda ok, outs, total, inp: {outs[0]: near(ok[inp], V - 16), "wb": 0}))
    return out


def per_output(name):
    return {"litho_peb_bake": 3, "litho_peb_bake_vjp": 2, "litho_peb_bake_vjp_params": 3, "litho_peb_bake_jvp": 6}.get(name, 1)


@pytest.mark.parametrize("name", NAMES)
def test_two_faults_at_once_report_the_first_in_the_order(nat, name):
    table, launches = entries(nat)
    fn, ok, outs, total, inp, bad = table[name]
    codes = {"E_ARG": nat.E_ARG, "E_WORKSPACE": nat.E_WORKSPACE}
    solver = name.startswith("litho_develop_time")

    def call(kw):
        launches.value = 7
        rc = fn(*{**ok, **kw}.values(), None)
        if solver:
            assert launches.value == 0, (name, kw)                             # zeroed before anything else
        return rc

    assert ok["wb"] > 0 and len(outs) == per_output(name)
    # each fault alone, so that a combination below is known to combine two
    assert call(dict(wb=ok["wb"] - 1)) == nat.E_WORKSPACE and call(dict(work=near(ok["work"], 4))) == nat.E_ARG and call(bad) == nat.E_ARG
    for label, want, make in cases(name):
        kw = {**bad, "wb": ok["wb"] - 1} if make is None else make(ok, outs, total, inp)
        assert call(kw) == codes[want], (name, label)
    # a short workspace and a written buffer over the workspace: the size is reported, for every buffer the call writes
    for o in outs:
        for where in (ok["work"], near(ok["work"], max(ok["wb"] - 16, 0))):
            assert call({o: where}) == nat.E_ARG, (name, o)                    # alone it is an aliasing refusal ...
            assert call({o: where, "wb": ok["wb"] - 1}) == nat.E_WORKSPACE, (name, o)      # ... and second in the order
            assert call({o: where, "wb": 0}) == nat.E_WORKSPACE, (name, o)
    # and an input over the workspace as well
    first = next(iter(ok))
    assert call({first: ok["work"]}) == nat.E_ARG and call({first: ok["work"], "wb": ok["wb"] - 1}) == nat.E_WORKSPACE, name
