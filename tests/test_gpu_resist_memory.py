"""Where the resist chain reads and writes (csrc/film.hip, develop.hip, peb.hip, develop_grad.hip): twelve entry points through the
raw C ABI with every device buffer of a call -- inputs, outputs, workspace -- inside one guarded, poisoned arena (tests/arena.py,
itself checked by tests/test_arena_cpu.py).  The numerical tests (test_gpu_film.py, test_gpu_develop.py, test_gpu_peb.py,
test_gpu_peb_grad.py, test_gpu_develop_grad.py) pin WHAT these kernels compute against float64 oracles; they take their outputs
and workspaces from torch.empty, where an overrun lands in allocator slack, a just-freed block already holds the previous
result, and fresh memory is mostly zero.  Here nothing numerical is re-derived: the reference of every case is the project's
own Python wrapper on ordinary tensors on the default stream, and every assertion is bit equality or a return code.

Per case (entry, shape, variant, alignment):
  a  return code OK, every output equal to the reference bit for bit, equal launch counts;
  b  no guard byte and no input byte changed;
  c  no output word still holds the poison where the reference does not: this call wrote every element;
  d  the same call once more into the same arena, NOT re-poisoned (the workspace holds the first run's leftovers): same bits;
  e  alignments: every buffer 16-byte aligned; every volume pointer at 4 mod 16 (film: 8); one buffer at a time misaligned, the
     rest aligned -- the mixed selections of the 16-byte and the scalar variants of k_latent_diffuse, k_develop_rate,
     k_developed_depth, k_develop_links, k_develop_scale, k_develop_rate_vjp, k_peb_expose, k_peb_rate and k_peb_expose_vjp;
  f  litho_develop_time, litho_develop_time_vjp, litho_peb_bake, litho_peb_bake_vjp: a workspace at 8 mod 16 is LITHO_E_ARG, one
     byte too few LITHO_E_WORKSPACE, and every output and workspace byte is still poison afterwards;
  g  the same call on a side stream (no graph capture).
The arena is 0xFF: NaN as fp32, -1 as int32.  A guard is one plane + one row + one pack of the call's volume, (n n + n + 4)
elements rounded up to 256 bytes, in front of and behind every buffer; a workspace is exactly what its *_work_bytes returns
(litho_latent_diffuse: one volume when two or three passes run, NULL otherwise).

Shapes (n, D, B), the smallest at which each mechanism exists:
  (1, 1, 1)     the smallest volume
  (4, 2, 2)     the smallest n on the 16-byte path
  (15, 2, 3)    scalar path, partial tile
  (16, 5, 2)    exact tile
  (17, 3, 2)    a one-cell second tile, halo traffic both ways
  (12, 14, 2)   the first D at which the adjoint's tile leaves 64 KiB of LDS
  (20, 29, 1)   n % 4 == 0 but no multiple of 16; the first D at which the forward solver's tile leaves 64 KiB
LDS per plane of the tile, from the kernels' constants (test_the_shapes_sit_on_the_lds_thresholds asserts them; VOL_TILE 16 and
VOL_HALO 18 of csrc/resist_volume.hpp are the tile of both solvers):
  k_develop_time      VOL_TILE 16, halo 18: (18 18 + 16 16) floats = 2320 B; 28 planes 64960 B <= 65536 < 67280 B = 29 planes
  k_develop_time_vjp  VOL_TILE 16, halo 18: (3 18 18 + 16 16) floats = 4912 B; 13 planes 63856 B <= 65536 < 68768 B = 14 planes
  k_peb_fused         s steps per launch: D (4 (16 + 2 s)^2 + 256) floats against the 160 KiB of a workgroup: at D = 29 not even
                      s = 2 fits (215296 B), at D = 14 s = 2 (103936 B) and s = 4 (143360 B) both leave 64 KiB and fit
A change of the tile geometry shows there which shapes have to move.

Inputs: slowness volumes carry walls (NaN, 0, -1, +inf) where n > 1, images and acid doses a negative and a NaN cell, the
cotangents of the development and exposure adjoints NaN on the walls (where the slowness or the acid is NaN), the acid that is
baked forwards one NaN cell (it spreads; the comparison is of bit patterns).  The bake adjoint takes finite volumes: the header
leaves NaN there unspecified.

Observed on an MI355X (LABNOTES.md, "Memory discipline of the resist chain"): 361 tests, 1796 cases of two calls each, all of them
"guards intact / outputs fully written / bits equal"; NOTHING FOUND -- no guard or input byte moved, no output element was left
unwritten, no result depended on what the workspace held, and no 16-byte variant differed from its scalar twin in a single bit
(NaN cells included).  The eight refused calls returned LITHO_E_ARG / LITHO_E_WORKSPACE with outputs and workspace still poison.
Cases and time in the arenas per entry (arena set-up, two calls, two reports each):
    litho_film_pupils        17    0.19 s (0.18 of it the first call of the process)
    litho_latent_diffuse    127    0.07 s          litho_peb_expose         57    0.03 s
    litho_develop_rate       57    0.03 s          litho_peb_bake          465    0.50 s
    litho_develop_time       64    0.16 s          litho_peb_rate           64    0.04 s
    litho_developed_depth    29    0.02 s          litho_peb_bake_vjp      681    0.61 s
    litho_develop_time_vjp   93    0.21 s          litho_peb_expose_vjp     71    0.04 s
    litho_develop_rate_vjp   71    0.04 s
per shape, over the eleven volume entries: (1, 1, 1) 0.21 s, (4, 2, 2) 0.20 s, (15, 2, 3) 0.22 s, (16, 5, 2) 0.25 s, (17, 3, 2)
0.25 s, (12, 14, 2) 0.27 s, (20, 29, 1) 0.38 s.  Solver launches at these shapes, forward / adjoint: 2 / 2, 2 / 2, 2 / 2, 2 / 3,
6 / 6, 3 / 3, 8 / 8.  The whole file takes 5.1 s, wrapper references included; the slowest test 0.33 s (the first film case)."""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

import film_oracle as FO
from arena import Arena, Buf, differing

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (4, 2, 2), (15, 2, 3), (16, 5, 2), (17, 3, 2), (12, 14, 2), (20, 29, 1)]
ONE_SHAPE = (17, 3, 2)
THICK, H, BAKE = 100.0, 25.0, 60.0
NA, N0, WL = 1.35, 1.44, 193.0
LDS_DEFAULT, LDS_MAX = 64 * 1024, 160 * 1024
DOSES = {"three doses": (0.6, 1.0, 1.7), "one dose": (1.3,)}
ids = lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)        # noqa: E731


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


@pytest.fixture(scope="module")
def peb():
    from lithographysimulator_amd import peb
    return peb


@pytest.fixture(scope="module")
def side(dev):
    return torch.cuda.Stream(dev)


# ---- the shapes and the kernels' constants ---------------------------------------------------------------------------------------
def solver_lds(D):
    return D * (18 * 18 + 16 * 16) * 4


def adjoint_lds(D):
    return D * (3 * 18 * 18 + 16 * 16) * 4


def fused_lds(D, s):
    return D * (4 * (16 + 2 * s) ** 2 + 256) * 4


def fits(D, s):
    """test_gpu_peb.py's rule: whether the fused bake kernel's LDS at s steps per launch fits a workgroup."""
    return s <= 1 or fused_lds(D, s) <= LDS_MAX


def test_the_shapes_sit_on_the_lds_thresholds():
    assert solver_lds(1) == 2320 and solver_lds(28) <= LDS_DEFAULT < solver_lds(29)
    assert adjoint_lds(1) == 4912 and adjoint_lds(13) <= LDS_DEFAULT < adjoint_lds(14) and adjoint_lds(32) <= LDS_MAX
    assert (20, 29, 1) in SHAPES and (12, 14, 2) in SHAPES and 20 % 4 == 0 and 20 % 16 and 12 % 4 == 0
    assert not fits(29, 2) and fits(14, 4) and LDS_DEFAULT < fused_lds(14, 2) and fits(5, 4) and fused_lds(5, 4) < LDS_DEFAULT
    assert {n % 4 == 0 for n, _, _ in SHAPES} == {True, False} and {n for n, _, _ in SHAPES} >= {15, 16, 17}


# ---- a call, described once and run in many arenas -------------------------------------------------------------------------------
class Case:
    """ins: [(name, device tensor)]; outs: {name: reference tensor on the device} in the order of the arena; call(p, stream) ->
    rc or (rc, launches), p = {buffer name: c_void_p}, p["work_bytes"] = the workspace's size; `volumes`: the buffers whose
    alignment the library looks at (misaligned in turn)."""

    def __init__(self, entry, shape, variant, ins, outs, call, guard, work_bytes=0, launches=None, volumes=None, mod=4):
        self.entry, self.shape, self.variant, self.ins, self.outs, self.call = entry, shape, variant, ins, outs, call
        self.guard, self.work_bytes, self.launches, self.mod = guard, int(work_bytes), launches, mod
        self.volumes = volumes if volumes is not None else [nm for nm, _ in ins] + list(outs)

    def arena(self, dev, mods=None, work_bytes=None):
        mods = mods or {}
        bufs = [Buf(nm, "in", t.dtype, t.shape, mods.get(nm, 0)) for nm, t in self.ins]
        bufs += [Buf(nm, "out", t.dtype, t.shape, mods.get(nm, 0)) for nm, t in self.outs.items()]
        wb = self.work_bytes if work_bytes is None else work_bytes
        if wb:
            bufs.append(Buf("work", "work", torch.uint8, (wb,), mods.get("work", 0)))
        a = Arena(bufs, self.guard, dev)
        for nm, t in self.ins:
            a.fill(nm, t)
        a.seal()
        return a

    def alignments(self):
        """(label, {buffer: offset mod 16}): aligned, everything misaligned, one buffer at a time."""
        out = [("aligned", {}), (f"all at {self.mod} mod 16", {nm: self.mod for nm in self.volumes})]
        if len(self.volumes) > 1:
            out += [(f"{nm} at {self.mod} mod 16", {nm: self.mod}) for nm in self.volumes]
        return out


def invoke(nat, dev, case, a, side=None):
    p = {nm: ctypes.c_void_p(a.ptr(nm)) for nm in a.bufs}
    p.setdefault("work", None)
    p["work_bytes"] = a.bufs["work"].nbytes if "work" in a.bufs else 0
    with torch.cuda.device(dev):
        if side is None:
            res = case.call(p, nat.stream_ptr(dev))
        else:
            cur = torch.cuda.current_stream(dev)
            assert side.cuda_stream != cur.cuda_stream
            side.wait_stream(cur)                                              # the inputs were copied in on the current stream
            with torch.cuda.stream(side):
                assert nat.stream_ptr(dev).value == side.cuda_stream
                res = case.call(p, nat.stream_ptr(dev))
            cur.wait_stream(side)
    torch.cuda.synchronize(dev)
    return res if isinstance(res, tuple) else (res, None)


def check(nat, dev, case, label, mods=None, side=None):
    """Assertions a-d of one case in one arena; prints its line."""
    a = case.arena(dev, mods)
    for attempt in ("first", "second"):
        rc, launches = invoke(nat, dev, case, a, side)
        tag = f"{case.entry} {case.shape} {case.variant}, {label}, {attempt} call"
        assert rc == nat.LITHO_OK, (tag, rc)
        assert launches == case.launches, (tag, launches, case.launches)
        rep = a.report(case.outs)
        assert rep.clean, f"{tag}: {rep}"
        diff = {nm: d[:8] for nm, d in ((nm, differing(a[nm], want)) for nm, want in case.outs.items()) if d}
        assert not diff, f"{tag}: output words that differ from the reference (name: byte offsets) {diff}"
    print(f"{case.entry} {case.shape} {case.variant}, {label}{', side stream' if side is not None else ''}: guards intact / "
          f"outputs fully written / bits equal" + (f" / {case.launches} launches" if case.launches is not None else "")
          + ", twice")


def run(nat, dev, case, side=None):
    t0 = time.perf_counter()
    todo = case.alignments() if side is None else case.alignments()[:1]
    for label, mods in todo:
        check(nat, dev, case, label, mods, side)
    print(f"   {len(todo)} arenas, two calls each: {1e3 * (time.perf_counter() - t0):.0f} ms")


# ---- inputs, made once per shape -------------------------------------------------------------------------------------------------
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def guard_bytes(n):
    return (n * n + n + 4) * 4


def image_of(dev, shape, seed=0, top=3.0):
    """An intensity-like volume [B,D,n,n] in [0, top) with a negative and a NaN cell where n > 1."""
    n, D, B = shape

    def make():
        v = np.random.default_rng(1000 * n + 10 * D + B + seed).uniform(0.0, top, (B, D, n, n)).astype(np.float32)
        if n > 1:
            v[0, 0, 0, 1] = -0.5
            v[B - 1, D - 1, n - 1, n - 2] = np.nan
        return torch.from_numpy(v).to(dev)
    return memo(("image", shape, seed, top), make)


def slowness_of(dev, shape):
    """Slowness log-uniform over three decades with the four kinds of wall where n > 1."""
    n, D, B = shape

    def make():
        s = (10.0 ** np.random.default_rng(77 * n + D + B).uniform(-3.0, 0.0, (B, D, n, n))).astype(np.float32)
        if n > 1:
            s[0, 0, 0, 1], s[0, D - 1, n - 1, n - 2], s[B - 1, 0, 1, 0], s[B - 1, D - 1, n // 2, n // 2] = np.nan, 0.0, -1.0, np.inf
        return torch.from_numpy(s).to(dev)
    return memo(("slowness", shape), make)


def walls_of(s):
    return ~(torch.isfinite(s) & (s > 0))


def uniform_of(dev, key, shape4, lo=-1.0, hi=1.0):
    def make():
        seed = sum(ord(c) for c in key) + 13 * int(np.prod(shape4)) + shape4[-1]
        return torch.from_numpy(np.random.default_rng(seed).uniform(lo, hi, shape4).astype(np.float32)).to(dev)
    return memo(("uniform", key, tuple(shape4), lo, hi), make)


def arrival_of(L, dev, shape):
    """(T, launches) of the wrapper, the reference of litho_develop_time and an input of what follows it."""
    return memo(("T", shape), lambda: L.developmentTime(slowness_of(dev, shape), THICK, H, returnLaunches=True))


def cotangent_of(dev, shape):
    """dl/dT: uniform in (-1, 1), NaN on the walls."""
    n, D, B = shape

    def make():
        g = uniform_of(dev, "gradT", (B, D, n, n)).clone()
        g[walls_of(slowness_of(dev, shape))] = float("nan")
        return g
    return memo(("gradT", shape), make)


def mack_of(L):
    return L.MackResist(C=0.9, rMax=120.0, rMin=0.05, q=5.0, mTh=0.4, surfaceRate=0.25, surfaceDepth=30.0)


def car_of(L, D, k_quench):
    """Both species diffuse, half as far vertically; the smallest stable step count on the (H, THICK / D) grid is 5."""
    sigma = math.sqrt(4.5 / (2.0 / (H * H) + 0.25 / ((THICK / D) ** 2)))
    r = L.ChemicallyAmplifiedResist(C=1.0, quencher=0.3, kAmp=0.05, kQuench=k_quench, kLoss=0.02, acidDiffusionLength=sigma,
                                    quencherDiffusionLength=0.4 * sigma, verticalScale=0.5, bakeTime=BAKE, mack=mack_of(L))
    assert r.minSteps(THICK, D, H) == 5
    return r


def floats(values):
    return (ctypes.c_float * len(values))(*values)


# ---- the twelve entries ----------------------------------------------------------------------------------------------------------
def film_case(L, nat, dev, pn, variant):
    layers, sub, res = FO.STACKS["L3"]
    stack = L.FilmStack(layers, sub, res)
    planes, D = (1, 1) if variant == "D 1" else (2, 17)
    depths = [0.37 * stack.thickness] if D == 1 else stack.depths(D)
    defocus = None if D == 1 else [50.0, -30.0]
    rng = np.random.default_rng(pn)
    P = torch.from_numpy((rng.standard_normal((planes, pn, pn)) + 0.1 + 1j * rng.standard_normal((planes, pn, pn))).astype(np.complex64)).to(dev)
    want = memo(("film", pn, variant), lambda: L.filmPupils(P if planes > 1 else P[0], NA, stack, depths, WL, N0, True, defocus=defocus))
    want = want.reshape(planes, D, 6, pn, pn)
    lay = (ctypes.c_double * (3 * len(layers)))(*[v for layer in layers for v in layer])
    zd = (ctypes.c_double * D)(*depths)
    zf = (ctypes.c_double * planes)(*defocus) if defocus else None

    def call(p, st):
        return nat.lib().litho_film_pupils(p["pupil"], planes, pn, NA, N0, 1, lay, len(layers), sub[0], sub[1], res, zd, D, zf, WL,
                                           p["out"], st)
    return Case("litho_film_pupils", (pn, D, planes), variant, [("pupil", P)], {"out": want}, call, (pn * pn + pn + 4) * 8, mod=8)


DIFFUSIONS = {"lateral only": (1.2, 0.0), "vertical only": (0.0, 0.45), "both": (1.2, 0.45), "neither": (0.0, 0.0)}


def diffuse_case(L, nat, dev, shape, variant):
    n, D, B = shape
    sxy_nm, sz_nm = DIFFUSIONS[variant][0] * H, DIFFUSIONS[variant][1] * (THICK / D)
    sxy, sz = float(sxy_nm) / H, float(sz_nm) / (THICK / D)                    # as latentDiffusion forms them
    passes = (2 if sxy > 0 else 0) + (1 if sz > 0 else 0)
    V = image_of(dev, shape, top=4.0)
    want = memo(("diffuse", shape, variant), lambda: L.latentDiffusion(V, THICK, H, sxy_nm, sz_nm))

    def call(p, st):
        return nat.lib().litho_latent_diffuse(p["image"], B, D, n, sxy, sz, p["out"], p["work"], p["work_bytes"], st)
    work = V.numel() * 4 if passes >= 2 else 0
    return Case("litho_latent_diffuse", shape, f"{variant} ({passes} passes)", [("image", V)], {"out": want}, call, guard_bytes(n),
                work_bytes=work, volumes=["image", "out"] + (["work"] if work else []))


def rate_case(L, nat, dev, shape, variant):
    n, D, B = shape
    doses, resist, V = DOSES[variant], mack_of(L), image_of(dev, shape)
    want = memo(("rate", shape, variant), lambda: L.developmentRate(V, resist, THICK, H, doses))
    g = floats(doses)

    def call(p, st):
        return nat.lib().litho_develop_rate(p["image"], B, D, n, g, len(doses), resist.C, resist.rMax, resist.rMin, resist.q, resist.mTh,
                                            resist.surfaceRate, resist.surfaceDepth, THICK, p["slowness"], st)
    return Case("litho_develop_rate", shape, variant, [("image", V)], {"slowness": want}, call, guard_bytes(n))


def time_case(L, nat, dev, shape, variant):
    n, D, B = shape
    s = slowness_of(dev, shape)
    T, launches = arrival_of(L, dev, shape)
    cap = 1024 if variant == "cap 1024" else launches                         # exactly enough: the smallest flag array, its last used word
    need = int(nat.lib().litho_develop_work_bytes(B, D, n, cap))
    assert need == (4 * cap + 255) // 256 * 256 + s.numel() * 4

    def call(p, st):
        count = ctypes.c_int(-1)
        rc = nat.lib().litho_develop_time(p["slowness"], B, D, n, THICK, H, cap, p["T"], p["work"], p["work_bytes"], ctypes.byref(count), st)
        return rc, count.value
    return Case("litho_develop_time", shape, f"{variant} (max_iterations {cap})", [("slowness", s)], {"T": T}, call, guard_bytes(n),
                work_bytes=need, launches=launches, volumes=["slowness", "T"])


def depth_case(L, nat, dev, shape, variant):
    n, D, B = shape
    T, _ = arrival_of(L, dev, shape)
    t = float(T[torch.isfinite(T)].median())
    want = memo(("depth", shape), lambda: L.developedDepth(T, THICK, t))

    def call(p, st):
        return nat.lib().litho_developed_depth(p["T"], B, D, n, THICK, t, p["depth"], st)
    return Case("litho_developed_depth", shape, variant, [("T", T)], {"depth": want}, call, guard_bytes(n))


def time_vjp_case(L, nat, dev, shape, variant):
    n, D, B = shape
    s, (T, _), g = slowness_of(dev, shape), arrival_of(L, dev, shape), cotangent_of(dev, shape)
    want, launches = memo(("time vjp", shape), lambda: L.developmentTimeGradient(s, T, g, THICK, H, returnLaunches=True))
    cap = 1024 if variant == "cap 1024" else launches
    need = int(nat.lib().litho_develop_vjp_work_bytes(B, D, n, cap))
    assert need == (4 * cap + 255) // 256 * 256 + 5 * s.numel() * 4

    def call(p, st):
        count = ctypes.c_int(-1)
        rc = nat.lib().litho_develop_time_vjp(p["slowness"], p["T"], p["grad_T"], B, D, n, THICK, H, cap, p["grad_slowness"], p["work"],
                                              p["work_bytes"], ctypes.byref(count), st)
        return rc, count.value
    return Case("litho_develop_time_vjp", shape, f"{variant} (max_iterations {cap})", [("slowness", s), ("T", T), ("grad_T", g)],
                {"grad_slowness": want}, call, guard_bytes(n), work_bytes=need, launches=launches,
                volumes=["slowness", "T", "grad_T", "grad_slowness"])


def rate_vjp_case(L, nat, dev, shape, variant):
    n, D, B = shape
    doses, resist, V = DOSES[variant], mack_of(L), image_of(dev, shape)

    def cotangent():
        gs = uniform_of(dev, "gradS" + variant, (len(doses) * B, D, n, n)).clone()
        gs[torch.isnan(L.developmentRate(V, resist, THICK, H, doses))] = float("nan")      # NaN on the walls
        return gs
    gs = memo(("rate vjp in", shape, variant), cotangent)
    want = memo(("rate vjp", shape, variant), lambda: L.developmentRateGradient(V, resist, THICK, H, doses, gs))
    g = floats(doses)

    def call(p, st):
        return nat.lib().litho_develop_rate_vjp(p["x"], B, D, n, g, len(doses), resist.C, resist.rMax, resist.rMin, resist.q, resist.mTh,
                                                resist.surfaceRate, resist.surfaceDepth, THICK, p["grad_slowness"], p["grad_x"], st)
    return Case("litho_develop_rate_vjp", shape, variant, [("x", V), ("grad_slowness", gs)], {"grad_x": want}, call, guard_bytes(n))


def expose_case(peb, nat, dev, shape, variant):
    n, D, B = shape
    doses, V = DOSES[variant], image_of(dev, shape)
    want = memo(("expose", shape, variant), lambda: peb.exposeAcid(V, 0.9, doses))
    g = floats(doses)

    def call(p, st):
        return nat.lib().litho_peb_expose(p["image"], B, D, n, g, len(doses), 0.9, p["acid"], st)
    return Case("litho_peb_expose", shape, variant, [("image", V)], {"acid": want}, call, guard_bytes(n))


def bake_case(L, peb, nat, dev, shape, S, spl, quench):
    n, D, B = shape
    r = car_of(L, D, 2.0 if quench == "finite" else float("inf"))

    def acid():
        h0 = uniform_of(dev, "h0", (B, D, n, n), 0.0, 1.0).clone()
        if n > 1:
            h0[B - 1, D // 2, n // 2, 1] = float("nan")
        return h0
    h0 = memo(("bake in", shape), acid)
    want = memo(("bake", shape, S, quench), lambda: peb.bakeAcid(h0, r, THICK, H, steps=S, stepsPerLaunch=0)[:3])
    need = int(nat.lib().litho_peb_work_bytes(B, D, n))
    assert need == 2 * h0.numel() * 4

    def call(p, st):
        return nat.lib().litho_peb_bake(p["acid_in"], B, D, n, THICK, H, r.quencher, r.kQuench, r.kLoss, r.acidDiffusionLength,
                                        r.quencherDiffusionLength, r.verticalScale, r.bakeTime, S, spl, p["acid"], p["quencher"],
                                        p["acid_dose"], p["work"], p["work_bytes"], st)
    return Case("litho_peb_bake", shape, f"S {S}, steps_per_launch {spl}, {quench} quench", [("acid_in", h0)],
                {"acid": want[0], "quencher": want[1], "acid_dose": want[2]}, call, guard_bytes(n), work_bytes=need,
                volumes=["acid_in", "acid", "quencher", "acid_dose"])


def peb_rate_case(L, peb, nat, dev, shape, variant):
    n, D, B = shape
    r, a = car_of(L, D, 2.0), image_of(dev, shape, seed=5, top=80.0)
    m, slow = memo(("peb rate", shape), lambda: peb.amplifiedRate(a, r, THICK))
    mk = r.mack
    outs = {"slowness": slow, "inhibitor": m} if variant == "with inhibitor" else {"slowness": slow}

    def call(p, st):
        return nat.lib().litho_peb_rate(p["acid_dose"], B, D, n, r.kAmp, mk.rMax, mk.rMin, mk.q, mk.mTh, mk.surfaceRate, mk.surfaceDepth,
                                        THICK, p["slowness"], p.get("inhibitor"), st)
    return Case("litho_peb_rate", shape, variant, [("acid_dose", a)], outs, call, guard_bytes(n))


COTANGENTS = {"grad_acid": (True, False, False), "grad_quencher": (False, True, False), "grad_acid_dose": (False, False, True),
              "all three": (True, True, True)}


def bake_vjp_case(L, peb, nat, dev, shape, c, which, q_in):
    n, D, B = shape
    S, r = 5, car_of(L, D, 2.0)
    h0 = uniform_of(dev, "h0 vjp", (B, D, n, n), 0.0, 1.0)
    cot = [uniform_of(dev, nm, (B, D, n, n)) if on else None for nm, on in zip(("gh", "gq", "ga"), COTANGENTS[which])]
    want = memo(("bake vjp", shape, which), lambda: peb.bakeGradient(h0, r, THICK, H, cot[0], cot[1], cot[2], steps=S))
    need = int(nat.lib().litho_peb_vjp_work_bytes(B, D, n, S, c))
    assert need == (2 * (-(-S // c) - 1) + 2 * c + 8) * h0.numel() * 4
    names = ("grad_acid", "grad_quencher", "grad_acid_dose")
    ins = [("acid_in", h0)] + [(nm, t) for nm, t in zip(names, cot) if t is not None]
    outs = {"grad_acid_in": want[0], "grad_quencher_in": want[1]} if q_in else {"grad_acid_in": want[0]}

    def call(p, st):
        return nat.lib().litho_peb_bake_vjp(p["acid_in"], B, D, n, THICK, H, r.quencher, r.kQuench, r.kLoss, r.acidDiffusionLength,
                                            r.quencherDiffusionLength, r.verticalScale, r.bakeTime, S, c, p.get("grad_acid"),
                                            p.get("grad_quencher"), p.get("grad_acid_dose"), p["grad_acid_in"], p.get("grad_quencher_in"),
                                            p["work"], p["work_bytes"], st)
    return Case("litho_peb_bake_vjp", shape, f"S 5, checkpoint_every {c} ({-(-S // c)} segments), {which}, grad_quencher_in "
                f"{'given' if q_in else 'NULL'}", ins, outs, call, guard_bytes(n), work_bytes=need,
                volumes=[nm for nm, _ in ins] + list(outs))


def expose_vjp_case(peb, nat, dev, shape, variant):
    n, D, B = shape
    doses, V = DOSES[variant], image_of(dev, shape)

    def cotangent():
        ga = uniform_of(dev, "gradAcid" + variant, (len(doses) * B, D, n, n)).clone()
        ga[torch.isnan(peb.exposeAcid(V, 0.9, doses))] = float("nan")          # NaN where the acid is: the walls to be
        return ga
    ga = memo(("expose vjp in", shape, variant), cotangent)
    want = memo(("expose vjp", shape, variant), lambda: peb.exposeAcidGradient(V, 0.9, doses, ga))
    g = floats(doses)

    def call(p, st):
        return nat.lib().litho_peb_expose_vjp(p["image"], B, D, n, g, len(doses), 0.9, p["grad_acid"], p["grad_image"], st)
    return Case("litho_peb_expose_vjp", shape, variant, [("image", V), ("grad_acid", ga)], {"grad_image": want}, call, guard_bytes(n))


# ---- a-e: every entry, shape, variant and alignment ------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["D 1", "D 17"])
@pytest.mark.parametrize("pn", [16, 30])
def test_film_pupils(L, nat, dev, pn, variant):
    run(nat, dev, film_case(L, nat, dev, pn, variant))


@pytest.mark.parametrize("variant", list(DIFFUSIONS))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_latent_diffuse(L, nat, dev, shape, variant):
    run(nat, dev, diffuse_case(L, nat, dev, shape, variant))


@pytest.mark.parametrize("variant", list(DOSES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_develop_rate(L, nat, dev, shape, variant):
    run(nat, dev, rate_case(L, nat, dev, shape, variant))


@pytest.mark.parametrize("variant", ["cap 1024", "cap exact"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_develop_time(L, nat, dev, shape, variant):
    run(nat, dev, time_case(L, nat, dev, shape, variant))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_developed_depth(L, nat, dev, shape):
    run(nat, dev, depth_case(L, nat, dev, shape, "median arrival time"))


@pytest.mark.parametrize("variant", ["cap 1024", "cap exact"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_develop_time_vjp(L, nat, dev, shape, variant):
    run(nat, dev, time_vjp_case(L, nat, dev, shape, variant))


@pytest.mark.parametrize("variant", list(DOSES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_develop_rate_vjp(L, nat, dev, shape, variant):
    run(nat, dev, rate_vjp_case(L, nat, dev, shape, variant))


@pytest.mark.parametrize("variant", list(DOSES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_peb_expose(peb, nat, dev, shape, variant):
    run(nat, dev, expose_case(peb, nat, dev, shape, variant))


BAKES = [(shape, S, spl, quench) for shape in SHAPES for S in (5, 7) for spl in (0, 2, 4) if fits(shape[1], spl)
         for quench in ("finite", "instantaneous")]


@pytest.mark.parametrize("shape,S,spl,quench", BAKES, ids=[f"{ids(b[0])}-S{b[1]}-spl{b[2]}-{b[3]}" for b in BAKES])
def test_peb_bake(L, peb, nat, dev, shape, S, spl, quench):
    run(nat, dev, bake_case(L, peb, nat, dev, shape, S, spl, quench))


@pytest.mark.parametrize("variant", ["with inhibitor", "without inhibitor"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_peb_rate(L, peb, nat, dev, shape, variant):
    run(nat, dev, peb_rate_case(L, peb, nat, dev, shape, variant))


@pytest.mark.parametrize("q_in", [True, False], ids=["q_in", "no_q_in"])
@pytest.mark.parametrize("which", list(COTANGENTS))
@pytest.mark.parametrize("c", [2, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_peb_bake_vjp(L, peb, nat, dev, shape, c, which, q_in):
    run(nat, dev, bake_vjp_case(L, peb, nat, dev, shape, c, which, q_in))


@pytest.mark.parametrize("variant", list(DOSES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_peb_expose_vjp(peb, nat, dev, shape, variant):
    run(nat, dev, expose_vjp_case(peb, nat, dev, shape, variant))


def test_the_bakes_cover_what_fits():
    """Every D takes steps_per_launch 0; 2 and 4 wherever the header's LDS formula fits 160 KiB: all but D = 29."""
    for n, D, B in SHAPES:
        got = sorted({spl for shape, _, spl, _ in BAKES if shape == (n, D, B)})
        assert got == ([0] if D == 29 else [0, 2, 4]), (D, got)


# ---- f: a refused call launches nothing ------------------------------------------------------------------------------------------
def multi_launch_cases(L, peb, nat, dev, shape):
    return [time_case(L, nat, dev, shape, "cap 1024"), time_vjp_case(L, nat, dev, shape, "cap 1024"),
            bake_case(L, peb, nat, dev, shape, 5, 0, "finite"), bake_vjp_case(L, peb, nat, dev, shape, 2, "all three", True)]


@pytest.mark.parametrize("which", range(4), ids=["develop_time", "develop_time_vjp", "peb_bake", "peb_bake_vjp"])
def test_a_refused_workspace_launches_nothing(L, peb, nat, dev, which):
    case = multi_launch_cases(L, peb, nat, dev, ONE_SHAPE)[which]
    for label, mods, nbytes, expected in (("workspace at 8 mod 16", {"work": 8}, case.work_bytes, nat.E_ARG),
                                          ("workspace one byte short", {}, case.work_bytes - 1, nat.E_WORKSPACE)):
        a = case.arena(dev, mods, work_bytes=nbytes)
        assert a.ptr("work") % 16 == mods.get("work", 0) and a.bufs["work"].nbytes == nbytes
        rc, launches = invoke(nat, dev, case, a)
        assert rc == expected, (case.entry, label, rc)
        assert launches in (None, 0)
        untouched = all(a.still_poison(nm) for nm in list(case.outs) + ["work"])
        rep = a.report(case.outs)
        print(f"{case.entry} {case.shape}, {label}: return code {rc}; outputs and workspace {'still poison' if untouched else 'TOUCHED'}; "
              f"guards {'intact' if not rep.guards else rep.guards[:4]}")
        assert untouched and not rep.guards and not rep.inputs


# ---- g: side streams -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4), ids=["develop_time", "develop_time_vjp", "peb_bake", "peb_bake_vjp"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_multi_launch_entries_on_a_side_stream(L, peb, nat, dev, side, shape, which):
    run(nat, dev, multi_launch_cases(L, peb, nat, dev, shape)[which], side)


def test_single_launch_entries_on_a_side_stream(L, peb, nat, dev, side):
    s = ONE_SHAPE
    for case in (film_case(L, nat, dev, 30, "D 17"), diffuse_case(L, nat, dev, s, "both"), rate_case(L, nat, dev, s, "three doses"),
                 depth_case(L, nat, dev, s, "median arrival time"), rate_vjp_case(L, nat, dev, s, "three doses"),
                 expose_case(peb, nat, dev, s, "three doses"), peb_rate_case(L, peb, nat, dev, s, "with inhibitor"),
                 expose_vjp_case(peb, nat, dev, s, "three doses")):
        run(nat, dev, case, side)


# ---- the harness bites -----------------------------------------------------------------------------------------------------------
def test_the_harness_reports_a_write_outside_a_buffer(L, nat, dev):
    """A correct call, then two ordinary torch assignments inside the arena: one element just behind the output, one just in front
    of the workspace.  No kernel is made to misbehave; the report must name both places."""
    case = time_case(L, nat, dev, ONE_SHAPE, "cap 1024")
    a = case.arena(dev)
    rc, _ = invoke(nat, dev, case, a)
    assert rc == nat.LITHO_OK and a.report(case.outs).clean
    T, w = a.bufs["T"], a.bufs["work"]
    a.bytes[T.end:T.end + 4].view(torch.float32)[0] = 1.0                      # 0x3f800000: every byte differs from 0xFF
    a.bytes[w.start - 4:w.start].view(torch.int32)[0] = 0
    rep = a.report(case.outs)
    print(f"planted: one fp32 behind T, one int32 in front of the workspace; reported: {rep}")
    assert rep.guards == [("T", T.nbytes + i) for i in range(4)] + [("work", -4 + i) for i in range(4)]
    assert not rep.inputs and not rep.unwritten and not rep.clean
    a["T"].view(torch.int32)[1, 2, 16, 16] = -1                                # and an output element put back to poison
    assert a.report(case.outs).unwritten == [("T", 4 * ((1 * 3 + 2) * 17 * 17 + 16 * 17 + 16))]
