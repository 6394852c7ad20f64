"""Where the layout, metrology and contour kernels read and write (csrc/layout.hip, optics.hip's k_measure_cd, metrology.hip,
contour.hip): seven entry points through the raw C ABI with every device buffer of a call -- inputs, outputs, workspace -- inside
one guarded, poisoned arena (tests/arena.py, itself checked by tests/test_arena_cpu.py).  These are the project's gather and
scatter kernels: their addresses come from polygon edges (k = (int)ceil(...)), from site coordinates (floorf(px)) and from mask
words (base + prefix + popc), not from a tile index.  The numerical tests (test_gpu_layout.py, test_gpu_coverage.py,
test_gpu_resist.py, test_gpu_epe.py, test_gpu_contour.py) go through the Python wrappers, which take outputs and workspaces from
torch.empty: an overrun lands in allocator slack, a stale workspace already holds the answer, a read one row past the image
returns a plausible float, and an output element nobody wrote looks like zero.

The reference of every case is a CPU restatement, never the wrapper (several of these shapes are pinned nowhere else):
contour_oracle.trace; epe_oracle and resist_oracle.measure_cd for samples, classification and the chosen interval / run, finished
here in NumPy float32 in the header's order of operations (the oracles finish in float64 for their tolerances; the family is
specified bit for bit); oracle.layout_oracle.rasterize_edges; coverage_oracle.coverage; np.fmin / np.fmax over float32 products.
Every comparison is of bit patterns, on integer views.

Per case (entry, shape, variant, alignment):
  a  return code LITHO_OK, every output equal to the reference bit for bit; for the contour pair also every byte of the workspace:
     mask words, prefixes, bases, totals and the copied offsets, restated from the oracle's inside map (contour_tables), and the
     padding word behind an odd number of images still poison;
  b  no guard byte and no input byte changed;
  c  no output element still holds the poison where the reference does not -- and no reference element IS the poison pattern
     (asserted when the case is made: NaN results are the canonical quiet NaN 0x7fc00000, `next` >= 0, geometry 0 / 1, counts
     >= 0, coverage in [0, 1]), so this is never vacuous;
  d  the same call once more into the used arena, NOT re-poisoned: same bits;
  e  alignments: every buffer 16-byte aligned; every fp32, int32 and int16 buffer at 4 mod 16; one buffer at a time at 4, 8 and
     12 mod 16 (float64 edges, int64 counts and the contour workspace, which must be 8-byte aligned: at 8 only).  The full sweep
     runs on one variant of every shape, "aligned" and "all at 4" on every variant;
  f  the same call on a side stream (no graph capture).
Refused calls return their code and leave every output and workspace byte poison: contour count and emit with the workspace at 4
and 12 mod 16 (LITHO_E_ARG) and one byte short (LITHO_E_WORKSPACE), litho_rasterize_edges one byte short, coverage with one byte
less than one band row.  Emit with offsets that disagree with the counted total of one image returns OK, leaves that image's
slice poison and writes the others in full.  litho_contour_count alone leaves the offsets, xy and next poison and everything else as
restated, in a fresh arena and in one that holds a whole count + emit.

The arena is 0xFF: NaN as fp32 / fp64, -1 as int16 / int32 / int64.  A guard is one plane + one row + 4 elements of the call's
largest buffer, at least 256 bytes, in front of and behind every buffer: [planes, n, n] images give (n n + n + 4) floats (an EPE
or CD table [gains, planes, S, 3] or [.., G, 5] gives 3 S + 3 + 4 or 5 G + 5 + 4 floats where that is more); the
rasteriser's [pn][pn + 1] and the coverage band's [rows s][pn s + 1] delta arrays are their own plane, one row pn + 1 or pn s + 1
words; the contour workspace's plane is one image's mask record, (n + 1) 2 W 64-bit words, its row 2 W words.  Workspaces are exactly
what *_work_bytes returns; for coverage exactly the bytes of 1 band row, of 3 (the last band shorter wherever pn % 3 != 0) and
of pn.

Shapes, the smallest at which each mechanism exists:
  contour count + emit   n 1, 2 (no interior; every vertex on a virtual edge), 63 (n + 1 = 64 fills one mask word), 64 (one bit in a
                         second word), 127, 128 (the same for the third word); n + 1 no multiple of 4 leaves idle waves in the last
                         workgroup; planes 1, 3; 1 and 3 gains everywhere, 64 distinct gains (linspace(0.4, 1.6, 64)) at n 64 and 65
                         with 2 planes: gain gi lives in lane gi and in bit gi of the carry; both tones; seeded_stack images
                         (saddles, products equal to T, NaN, +-inf); one stack without any crossing (emit: NULL outputs, no launch)
  litho_measure_epe      n 1 (no cell), 2, 3, 126; S 1, 3, 4 (one full workgroup), 5, 257; range 0.5, 31.5, 32 px: K 1, 63, 64 (at 64
                         lane 63 reads a 65th sample); planes 1, 3; gains 1, 3, 64; corners with outward normals, sites outside, NaN / inf
  litho_measure_cd       n 1, 2, 64, 65, 130, 200, both axes; gauges at column 0 and n - 1, on features 1, 64, 65, 129 and n wide (the
                         outward scan takes a second and a third 64-sample chunk and reaches both borders), beside features, and
                         invalid ones (row -1, row n, column -1, column n, axis 2); gains 1, 3, 64; planes 1, 3
  envelope               n 1, 15, 16, 17 (n n around one 256-thread workgroup); planes 1, 3; gains 1, 64; a NaN sample
  litho_rasterize_edges  pn 1, 2, 255, 256, 257, 300 (columns per thread 1 -> 2, trailing threads without a column); 0 (edges NULL), 1,
                         255, 256, 257 edges (one k_raster_edges workgroup, exactly, one thread more); horizontals, NaN, +-inf, polygons
                         out of the window on all four sides (k clips to 0 and to pn), one wholly outside
  coverage               (pn, s) (1,1) (1,16) (5,2) (64,1) (130,2) (33,4) (65,8) (64,16) (65,16): every S, whole and ragged 64-pixel
                         steps, one and several; the same edge lists, one polygon taller than the window (more than 128 sub-rows: several
                         k_cov_edges chunks)

The harness is shown to fail: after a correct contour call one fp32 is planted behind xy, one int32 in front of the workspace and one
`next` element is put back to all-ones, by plain torch assignments; each is reported at its byte offset.

Observed on an MI355X (LABNOTES.md, "Memory discipline of the layout, metrology and contour entries"): 147 tests, 593 cases in 1899
arenas of two calls each, all of them "guards intact / outputs fully written / bits equal"; NOTHING FOUND -- no guard or input
byte moved, no output element was left unwritten, no result depended on what the arena held before, no misaligned call differed
from the aligned one, and every image of the 64-gain calls has the oracle's bits (the EPE and CD tables too: the device's fp32
division, like the tracer's, is NumPy's).  The eight refused calls returned LITHO_E_ARG / LITHO_E_WORKSPACE with outputs and
workspace still poison.  Cases, arenas and the time in the arenas per entry (set-up, two calls, two reports each):
    litho_contour_count + emit    54 cases   270 arenas  0.80 s     litho_dose_focus_envelope   17 cases  177 arenas  0.17 s
    litho_measure_epe            361 cases   901 arenas  0.73 s     litho_rasterize_edges       32 cases  140 arenas  0.13 s
    litho_measure_cd              99 cases   305 arenas  0.25 s     litho_rasterize_coverage    30 cases  106 arenas  0.16 s
The whole file takes 9.9 s (9.1 and 9.3 s in two earlier runs), 2.2 s of it in the arenas and the rest in the CPU restatements; the slowest tests are the two 64-gain
contour cases (1.1 s each: 128 images through contour_oracle.trace), then 0.3 s (the first call of the process; EPE at S = 257)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import contour_oracle as CO
import coverage_oracle as VO
import epe_oracle as EO
import resist_oracle as RO
from arena import POISON, Arena, Buf, differing, poison_of, words
from oracle import layout_oracle as LO
from test_gpu_contour import seeded_stack
from test_gpu_epe import seeded_sites

pytestmark = pytest.mark.gpu

F = np.float32
T = 0.5
PS = 25.0
GAINS = {1: (1.0,), 3: (1.0, 0.5, 0.8), 64: tuple(float(g) for g in np.linspace(0.4, 1.6, 64).astype(F))}
CANONICAL_NAN = 0x7FC00000
STATS = {}                                                                     # entry -> [cases, arenas, seconds]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    assert _native.lib().litho_target_arch() == b"gfx950"
    return _native


@pytest.fixture(scope="module")
def side(dev):
    return torch.cuda.Stream(dev)


@pytest.fixture(scope="module", autouse=True)
def totals():
    yield
    for entry, (cases, arenas, seconds) in STATS.items():
        print(f"\n{entry:28s} {cases:5d} cases in {arenas:5d} arenas of two calls each, {seconds:6.2f} s", end="")
    print()


# ---- a call, described once and run in many arenas -------------------------------------------------------------------------------
def sane(name, t):
    """Assertion c's other half: the reference holds no element that IS the poison pattern, and no NaN but the canonical one."""
    w = words(t)
    assert not bool((w == poison_of(w)).any()), f"{name}: a reference element equals the poison pattern"
    if t.dtype == torch.float32:
        nan = torch.isnan(t).reshape(-1)
        assert bool((w[nan] == CANONICAL_NAN).all()), f"{name}: a reference NaN that is not 0x7fc00000"
    elif not t.dtype.is_floating_point:
        assert bool((t >= 0).all()), f"{name}: a negative count, index or pixel"


class Case:
    """ins: [(name, CPU tensor)]; outs: {name: reference CPU tensor} in the order of the arena; call(p, stream) -> rc, p = {buffer
    name: c_void_p}, p["work_bytes"] = the workspace's size; work_mods: the offsets mod 16 the entry accepts for its workspace
    besides 0; work_want: the workspace's expected bytes (uint8 CPU tensor) where the entry's layout is restated."""

    def __init__(self, entry, shape, variant, ins, outs, call, guard, work_bytes=0, work_mods=(4, 8, 12), work_want=None, holes=False):
        self.entry, self.shape, self.variant, self.ins, self.outs, self.call = entry, shape, variant, ins, outs, call
        self.guard, self.work_bytes, self.work_mods, self.work_want = max(256, int(guard)), int(work_bytes), work_mods, work_want
        for nm, t in outs.items():
            if not holes:                                                      # (holes: a reference that leaves elements poison on purpose)
                sane(f"{entry} {shape} {variant} {nm}", t)

    def arena(self, dev, mods=None, work_bytes=None):
        mods = mods or {}
        bufs = [Buf(nm, "in", t.dtype, t.shape, mods.get(nm, 0)) for nm, t in self.ins]
        bufs += [Buf(nm, "out", t.dtype, t.shape, mods.get(nm, 0)) for nm, t in self.outs.items()]
        wb = self.work_bytes if work_bytes is None else work_bytes
        if wb:
            bufs.append(Buf("work", "work", torch.uint8, (wb,), mods.get("work", 0)))
        a = Arena(bufs, self.guard, dev)
        for nm, t in self.ins:
            a.fill(nm, t.to(dev))
        a.seal()
        return a

    def movable(self):
        """[(buffer, the offsets mod 16 it may take besides 0)]: 4, 8, 12 for elements of 2 and 4 bytes, 8 for those of 8."""
        out = [(nm, (8,) if t.element_size() == 8 else (4, 8, 12)) for nm, t in self.ins + list(self.outs.items())]
        return out + ([("work", self.work_mods)] if self.work_bytes else [])

    def alignments(self, full=True):
        """(label, {buffer: offset mod 16}): aligned, every 2- and 4-byte buffer at 4, then one buffer at a time."""
        out = [("aligned", {}), ("all at 4 mod 16", {nm: 4 for nm, ok in self.movable() if 4 in ok})]
        if full:
            out += [(f"{nm} at {m} mod 16", {nm: m}) for nm, ok in self.movable() for m in ok]
        return out


def invoke(nat, dev, case, a, side=None, call=None):
    p = {nm: ctypes.c_void_p(a.ptr(nm)) for nm in a.bufs}
    p.setdefault("work", None)
    p["work_bytes"] = a.bufs["work"].nbytes if "work" in a.bufs else 0
    call = call or case.call
    with torch.cuda.device(dev):
        if side is None:
            rc = call(p, nat.stream_ptr(dev))
        else:
            cur = torch.cuda.current_stream(dev)
            assert side.cuda_stream != cur.cuda_stream
            side.wait_stream(cur)                                              # the inputs were copied in on the current stream
            with torch.cuda.stream(side):
                assert nat.stream_ptr(dev).value == side.cuda_stream
                rc = call(p, nat.stream_ptr(dev))
            cur.wait_stream(side)
    torch.cuda.synchronize(dev)
    return rc


def verdict(case, a, tag):
    """Assertions a-c on the arena as it stands."""
    rep = a.report(case.outs)
    assert rep.clean, f"{tag}: {rep}"
    diff = {nm: d[:8] for nm, d in ((nm, differing(a[nm], want)) for nm, want in case.outs.items()) if d}
    assert not diff, f"{tag}: output elements that differ from the reference (name: byte offsets) {diff}"
    if case.work_want is not None:
        d = differing(a["work"], case.work_want)
        assert not d, f"{tag}: workspace bytes that differ from the restated layout {d[:8]}"


def check(nat, dev, case, label, mods=None, side=None, work_bytes=None):
    """Assertions a-d of one case in one arena."""
    a = case.arena(dev, mods, work_bytes)
    for nm, m in (mods or {}).items():
        assert a.ptr(nm) % 16 == m
    for attempt in ("first", "second"):
        rc = invoke(nat, dev, case, a, side)
        tag = f"{case.entry} {case.shape} {case.variant}, {label}, {attempt} call"
        assert rc == nat.LITHO_OK, (tag, rc)
        verdict(case, a, tag)
    return a


def run(nat, dev, case, side=None, full=True):
    t0 = time.perf_counter()
    todo = case.alignments(full) if side is None else case.alignments(False)[:1]
    for label, mods in todo:
        check(nat, dev, case, label + (", side stream" if side is not None else ""), mods, side)
    s = STATS.setdefault(case.entry, [0, 0, 0.0])
    s[0], s[1], s[2] = s[0] + 1, s[1] + len(todo), s[2] + time.perf_counter() - t0
    print(f"{case.entry} {case.shape} {case.variant}{', side stream' if side is not None else ''}: {len(todo)} arenas, two calls "
          f"each, guards intact / outputs fully written / bits equal: {1e3 * (time.perf_counter() - t0):.0f} ms")


_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def floats(values):
    return (ctypes.c_float * len(values))(*values)


def tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def plane_guard(n):
    return (n * n + n + 4) * 4


# ---- contours --------------------------------------------------------------------------------------------------------------------
def contour_stack(n, planes, exposed):
    """[planes, n, n]: seeded_stack where it has room for its special samples; written out below that."""
    def make():
        if n == 1:
            u = np.array([[[0.75 if exposed else 0.25]], [[0.5]], [[np.nan]]], dtype=F)
        elif n == 2:
            u = np.array([[[0.75, 0.25], [0.25, 0.75]], [[0.5, np.inf], [np.nan, -np.inf]], [[1.0, 0.1], [0.2, 0.3]]], dtype=F)    # a saddle first
        else:
            u = seeded_stack(n, 3, 4000 + n)
        return u
    return memo(("stack", n, exposed if n == 1 else None), make)[:planes]


def traced(n, p, gain, exposed):
    return memo(("trace", n, p, gain, exposed), lambda: CO.trace(contour_stack(n, 3, exposed)[p], gain, T, exposed))


def contour_layout(n, images):
    """Byte offsets of the five sub-arrays of the contour workspace, as the header describes them: uint64 masks [images][n + 1][2 W],
    int64 offsets [images + 1], int32 prefixes [images][n + 1][2 W], int32 bases [images][n + 1][2], int32 totals [images], rounded
    up to 8."""
    W = (n + 1 + 63) // 64
    rec = (n + 1) * 2 * W
    offs = images * rec * 8
    pref = offs + (images + 1) * 8
    base = pref + images * rec * 4
    total = base + images * (n + 1) * 2 * 4
    return dict(W=W, rec=rec, offs=offs, pref=pref, base=base, total=total, bytes=(total + images * 4 + 7) // 8 * 8)


def contour_tables(inside):
    """One image's (mask uint64 [n + 1][2 W], prefix int32 [n + 1][2 W], base int32 [n + 1][2], total) from its inside map: record
    R = r + 1 holds the crossed H edges of row r (bit e = c + 1) and the crossed V edges between rows r and r + 1 (bit c)."""
    n = inside.shape[0]
    W = (n + 1 + 63) // 64
    ext = np.zeros((n + 2, n + 2), dtype=bool)
    ext[1:-1, 1:-1] = inside
    bits = np.zeros((n + 1, 2, 64 * W), dtype=bool)
    bits[1:, 0, :n + 1] = ext[1:-1, :-1] != ext[1:-1, 1:]
    bits[:, 1, :n] = ext[:-1, 1:-1] != ext[1:, 1:-1]
    bits = bits.reshape(n + 1, 2, W, 64)
    mask = np.bitwise_or.reduce(bits.astype(np.uint64) << np.arange(64, dtype=np.uint64), axis=-1)
    pop = bits.sum(axis=-1).astype(np.int64)
    pref = np.cumsum(pop, axis=2) - pop
    tot = pop.sum(axis=2).reshape(-1)                                          # record by record: H total, V total
    base = np.cumsum(tot) - tot
    return mask.reshape(n + 1, 2 * W), pref.reshape(n + 1, 2 * W).astype(np.int32), base.reshape(n + 1, 2).astype(np.int32), int(tot.sum())


def contour_case(nat, n, planes, n_gains, exposed, offsets=None, flat=False):
    gains = GAINS[n_gains]
    images = planes * n_gains
    u = np.full((planes, n, n), 0.1 if exposed else 2.0, dtype=F) if flat else contour_stack(n, planes, exposed)
    ts = [CO.trace(u[p], g, T, exposed) if flat else traced(n, p, g, exposed) for g in gains for p in range(planes)]     # image = gain * planes + plane
    counts = np.array([len(t["next"]) for t in ts], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) if offsets is None else np.asarray(offsets(counts), dtype=np.int64)
    written = [int(offs[i + 1] - offs[i]) == int(counts[i]) for i in range(images)]
    V = int(offs[-1])
    lay = contour_layout(n, images)
    need = int(nat.lib().litho_contour_work_bytes(n, planes, n_gains)) if nat is not None else lay["bytes"]
    assert need == lay["bytes"]
    outs = {"counts": tensor(counts)}
    if V:
        xy = np.full((V, 2), -1, dtype=np.int32).view(F)                       # an image whose offsets disagree stays poison
        nxt = np.full(V, -1, dtype=np.int32)
        for i, t in enumerate(ts):
            if written[i] and counts[i]:
                xy[offs[i]:offs[i + 1]], nxt[offs[i]:offs[i + 1]] = t["xy"], t["next"]
        outs.update(xy=tensor(xy), next=tensor(nxt))
    tables = [contour_tables(t["inside"]) for t in ts]
    assert [tb[3] for tb in tables] == counts.tolist()                         # the restated workspace agrees with the oracle's count
    work = np.full(need, POISON, dtype=np.uint8)
    work[:lay["offs"]] = np.concatenate([tb[0].reshape(-1) for tb in tables]).view(np.uint8)
    if V:
        work[lay["offs"]:lay["pref"]] = offs.view(np.uint8)
    work[lay["pref"]:lay["base"]] = np.concatenate([tb[1].reshape(-1) for tb in tables]).view(np.uint8)
    work[lay["base"]:lay["total"]] = np.concatenate([tb[2].reshape(-1) for tb in tables]).view(np.uint8)
    work[lay["total"]:lay["total"] + 4 * images] = counts.astype(np.int32).view(np.uint8)
    g = floats(gains)

    def count(p, st):
        return nat.lib().litho_contour_count(p["image"], planes, n, g, n_gains, T, int(exposed), p["work"], p["work_bytes"], p["counts"], st)

    def emit(p, st):
        return nat.lib().litho_contour_emit(p["image"], planes, n, g, n_gains, T, int(exposed), p["work"], p["work_bytes"], offs.ctypes.data,
                                            p.get("xy"), p.get("next"), st)

    def call(p, st):
        return count(p, st) or emit(p, st)
    guard = max(plane_guard(n), (lay["rec"] + 2 * lay["W"] + 4) * 8)
    case = Case("litho_contour_count + emit", (n, planes, n_gains), f"exposed {int(exposed)}" + (", no crossing" if flat else ""),
                [("image", tensor(u))], outs, call, guard, work_bytes=need, work_mods=(8,), work_want=tensor(work), holes=offsets is not None)
    if offsets is None and not flat:                                           # c is not vacuous: what the oracle must show
        saddles = sum(sum(t["saddles"]) for t in ts)
        assert V > 0 and (n < 63 or saddles > 0), (V, saddles)
    case.count, case.emit, case.traces, case.offs, case.counts = count, emit, ts, offs, counts
    return case


# Both tones at every n with 1 and 3 gains.  With 64 gains the oracle's trace is what costs (128 images a case, over a second), so
# the tone alternates with n instead of doubling the two cases: it flips a comparison and moves no address.
CONTOURS = [(n, planes, g, ex) for n in (1, 2, 63, 64, 127, 128) for planes in (1, 3) for g in (1, 3) for ex in (1, 0)]
CONTOURS += [(64, 2, 64, 1), (65, 2, 64, 0)]


@pytest.mark.parametrize("n,planes,n_gains,exposed", CONTOURS, ids=[f"n{c[0]}-p{c[1]}-g{c[2]}-ex{c[3]}" for c in CONTOURS])
def test_contour_count_and_emit(nat, dev, n, planes, n_gains, exposed):
    case = contour_case(nat, n, planes, n_gains, bool(exposed))
    if n_gains == 64:
        ins = [t["inside"] for t in case.traces]
        assert len(set(GAINS[64])) == 64 and all(c > 0 for c in case.counts.tolist())          # distinct gains, a crossing in every image
        assert all(not np.array_equal(ins[62 * planes + p], ins[63 * planes + p]) for p in range(planes))     # gains 62 and 63 differ
        assert not np.array_equal(ins[62], ins[63]) and not np.array_equal(case.traces[62]["next"], case.traces[63]["next"])    # images 62, 63
    run(nat, dev, case, full=(planes, n_gains) in ((3, 3), (2, 64)))


@pytest.mark.parametrize("exposed", [1, 0])
def test_contour_without_a_crossing(nat, dev, exposed):
    """counts are zero, emit returns OK with NULL outputs before any launch: the workspace keeps what count left, its offsets poison."""
    case = contour_case(nat, 9, 2, 3, bool(exposed), flat=True)
    assert case.offs.tolist() == [0] * 7 and set(case.outs) == {"counts"}
    run(nat, dev, case)


@pytest.mark.parametrize("n,planes,n_gains,exposed", [(64, 3, 3, 1), (65, 2, 64, 0)])
def test_contour_count_alone(nat, dev, n, planes, n_gains, exposed):
    """litho_contour_count by itself writes counts and four of the workspace's five sub-arrays: the offsets (emit's copy), xy and
    next stay poison, everything else is the restated layout -- also when the arena already holds a whole count + emit."""
    case = contour_case(nat, n, planes, n_gains, bool(exposed))
    lay = contour_layout(n, planes * n_gains)
    want = case.work_want.clone()
    want[lay["offs"]:lay["pref"]] = POISON
    a = case.arena(dev)
    for attempt in ("first", "second"):
        assert invoke(nat, dev, case, a, call=case.count) == nat.LITHO_OK
        rep = a.report(case.outs)
        assert not rep.guards and not rep.inputs and {nm for nm, _ in rep.unwritten} == {"xy", "next"}, str(rep)
        assert a.still_poison("xy") and a.still_poison("next") and not differing(a["counts"], case.outs["counts"])
        assert not differing(a["work"], want), attempt
    assert invoke(nat, dev, case, a) == nat.LITHO_OK                            # count + emit, then count again: the offsets stay emit's
    verdict(case, a, "count + emit after count alone")
    assert invoke(nat, dev, case, a, call=case.count) == nat.LITHO_OK
    verdict(case, a, "count alone into the used arena")


def test_contour_emit_with_offsets_of_another_image(nat, dev):
    """The second of three images is given one vertex too few: emit returns OK, leaves that image's slice of xy and next poison and
    writes the other two in full, at the offsets it was given."""
    def one_short(counts):
        c = counts.copy()
        c[1] -= 1
        return np.concatenate([[0], np.cumsum(c)])
    case = contour_case(nat, 64, 3, 1, True, offsets=one_short)
    lo, hi = int(case.offs[1]), int(case.offs[2])
    assert hi - lo == case.counts[1] - 1 > 0 and bool((case.outs["next"][lo:hi] == -1).all()) and bool((case.outs["next"][hi:] >= 0).all())
    a = case.arena(dev)
    for attempt in ("first", "second"):
        assert invoke(nat, dev, case, a) == nat.LITHO_OK
        rep = a.report(case.outs)
        assert not rep.guards and not rep.inputs and not rep.unwritten, str(rep)
        assert not differing(a["xy"], case.outs["xy"]) and not differing(a["next"], case.outs["next"]) and not differing(a["work"], case.work_want)
        assert bool((words(a["next"])[lo:hi] == -1).all()) and bool((words(a["xy"])[2 * lo:2 * hi] == -1).all())


# ---- edge placement error --------------------------------------------------------------------------------------------------------
def epe_image(n):
    return memo(("epe image", n), lambda: np.random.default_rng(600 + n).random((3, n, n)).astype(F))


def epe_sites(n, S):
    """S rows of test_gpu_epe.py's site list: its last 14 (corners with outward normals, outside, NaN, inf) first, then axis-aligned
    and seeded ones; the short lists take one of each kind."""
    pool = seeded_sites(max(n, 2), 300, 700 + n)
    special, axis, free = pool[-14:], pool[300:340], pool[:300]
    if S >= 54:
        return np.concatenate([special, axis, free[:S - 54]])
    inner = np.array([[0.5 * (n - 1), 0.5 * (n - 1), 1.0, 0.0], [0.25 * (n - 1), 0.5 * (n - 1), -0.6, 0.8]], dtype=F)
    pick = np.concatenate([inner[:1], special[3:4], special[9:10], inner[1:], special[7:8]])     # inside, corner, NaN, inside, outside
    return np.ascontiguousarray(pick[:S])


def epe_reference(img, sites, gains, exposed, range_px):
    """fp32 [n_gains, planes, S, 3]: the interval epe_oracle.measure_epe chose, its position and slope in the header's fp32 order;
    held to the oracle's float64 value by the bound of test_gpu_epe.py."""
    table, cond = EO.measure_epe(img, sites, gains, T, exposed, range_px, PS)
    v, _, t = EO.samples(img, sites, range_px)
    K = (v.shape[-1] - 1) // 2
    T32, ps, h, nan = F(T), F(PS), F(0.5), F(np.nan)
    out = np.full(table.shape, nan, dtype=F)
    for gi, gain in enumerate(gains):
        u = v * F(gain)
        found = ~np.isnan(table[gi, ..., 2])
        pick = np.where(found, np.rint(2.0 * np.nan_to_num(table[gi, ..., 2])) + K, 0).astype(np.int64)
        a = np.take_along_axis(u, pick[..., None], axis=-1)[..., 0]
        b = np.take_along_axis(u, pick[..., None] + 1, axis=-1)[..., 0]
        tk = t[pick]
        with np.errstate(divide="ignore", invalid="ignore"):
            ts = tk + h * ((T32 - a) / (b - a))
            epe, ils = ts * ps, np.abs(b - a) / ((h * ps) * T32)
        assert epe.dtype == F and ils.dtype == F and tk.dtype == F
        out[gi, ..., 0], out[gi, ..., 1], out[gi, ..., 2] = np.where(found, epe, nan), np.where(found, ils, nan), np.where(found, tk, nan)
        tol = 2.0 ** -22 * (np.abs(table[gi, ..., 2]) + 0.5 * cond[gi]) * PS
        assert (np.abs(out[gi, ..., 0].astype(np.float64) - table[gi, ..., 0])[found] <= tol[found]).all()
    return out


def epe_case(nat, n, S, range_px, planes, n_gains, exposed):
    gains = GAINS[n_gains]
    img, sites = epe_image(n)[:planes], epe_sites(n, S)
    want = epe_reference(img, sites, gains, exposed, range_px)
    g = floats(gains)

    def call(p, st):
        return nat.lib().litho_measure_epe(p["image"], planes, n, p["sites"], S, g, n_gains, T, int(exposed), range_px, PS, p["out"], st)
    return Case("litho_measure_epe", (n, S), f"range {range_px}, {planes} planes, {n_gains} gains, exposed {int(exposed)}",
                [("image", tensor(img)), ("sites", tensor(sites))], {"out": tensor(want)}, call, max(plane_guard(n), (3 * S + 3 + 4) * 4))


@pytest.mark.parametrize("S", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("n", [1, 2, 3, 126])
def test_measure_epe(nat, dev, n, S):
    finite = nans = 0
    for i, (range_px, planes, n_gains) in enumerate((r, p, g) for r in (0.5, 31.5, 32.0) for p in (1, 3) for g in (1, 3, 64)):
        case = epe_case(nat, n, S, range_px, planes, n_gains, exposed=bool((i + S) % 2))
        rows = torch.isnan(case.outs["out"][..., 2])
        finite, nans = finite + int((~rows).sum()), nans + int(rows.sum())
        run(nat, dev, case, full=(range_px, planes, n_gains) == (32.0, 3, 3))
    print(f"n {n}, S {S}: {finite} rows with a crossing, {nans} without")
    assert nans > 0 and (finite > 0) == (n >= 2)                                # the table holds both kinds (n = 1 has no cell: NaN only)


# ---- critical dimension on cut lines ---------------------------------------------------------------------------------------------
def cd_layout(n, axis, exposed):
    """(image [3, n, n], gauges [(row, col, axis)], widths wanted): rows that carry one run of inside samples each -- 1 wide at column
    0 and at column n - 1, 64 wide from column 0 and up to column n - 1, 65 and 129 wide, and the whole row -- on a seeded
    background that is outside at every gain; gauges at both ends and in the middle of every run, just beside it, on an empty
    row at columns 0 and n - 1, and outside the grid.  axis 1: the same, transposed."""
    def make():
        rng = np.random.default_rng(900 + n)
        img = rng.uniform(0.05, 0.3, (3, n, n)).astype(F)
        runs = [(1, 0), (1, n - 1), (64, 0), (64, n - 64), (65, (n - 65) // 2), (129, 0), (129, n - 129), (n, 0)]
        runs = [(w, s) for w, s in runs if w <= n and s >= 0]
        gauges = []
        for i, (w, s) in enumerate(runs):
            r = (1 + 3 * i) if n >= 32 else i % n
            img[:, r, :] = rng.uniform(0.05, 0.3, (3, n)).astype(F)           # (a later run on the same row of a tiny grid replaces it)
            img[:, r, s:s + w] = rng.uniform(0.7, 0.95, (3, w)).astype(F)
            gauges += [(r, s, 0), (r, s + w - 1, 0), (r, s + w // 2, 0)] + [(r, c, 0) for c in (s - 1, s + w) if 0 <= c < n]
        empty = n - 1 if n >= 32 else None
        gauges += [(empty, 0, 0), (empty, n - 1, 0)] if empty else []
        gauges += [(-1, 0, 0), (n, 0, 0), (0, -1, 0), (0, n, 0), (0, 0, 2)]
        return img, gauges, sorted({w for w, _ in runs})
    img, gauges, widths = memo(("cd layout", n), make)
    if not exposed:
        img = (F(1.0) - img).astype(F)
    if axis == 1:
        img, gauges = np.ascontiguousarray(img.transpose(0, 2, 1)), [(c, r, a if a == 2 else 1) for r, c, a in gauges]
    return img, gauges, widths


def cd_reference(img, gauges, gains, exposed):
    """fp32 [n_gains, planes, G, 5]: the run resist_oracle.measure_cd found, its edges and slopes in the header's fp32 order."""
    table, runs, _ = RO.measure_cd(img, gauges, gains, T, exposed, PS)
    n = img.shape[-1]
    T32, ps, nan = F(T), F(PS), F(np.nan)
    out = np.full(table.shape, nan, dtype=F)
    for gi, gain in enumerate(gains):
        for p in range(img.shape[0]):
            for k, (row, col, axis) in enumerate(gauges):
                if np.isnan(table[gi, p, k, 0]):
                    continue                                                   # outside the grid: five NaN
                lo, hi = (int(x) for x in runs[gi, p, k])
                if lo < 0:
                    out[gi, p, k, 0] = 0
                    continue
                u = (img[p, row, :] if axis == 0 else img[p, :, col]) * F(gain)
                x_lo, x_hi = F(-0.5), F(n) - F(0.5)
                if lo > 0:
                    a, b = u[lo - 1], u[lo]
                    x_lo, out[gi, p, k, 3] = F(lo - 1) + (T32 - a) / (b - a), np.abs(b - a) / (T32 * ps)
                if hi < n - 1:
                    a, b = u[hi], u[hi + 1]
                    x_hi, out[gi, p, k, 4] = F(hi) + (T32 - a) / (b - a), np.abs(b - a) / (T32 * ps)
                out[gi, p, k, :3] = (x_hi - x_lo) * ps, x_lo, x_hi
                assert abs(float(out[gi, p, k, 0]) - table[gi, p, k, 0]) <= 1e-4 * PS * max(1.0, n / 64)     # the same quantity
    return out, runs


def cd_case(nat, n, axis, planes, n_gains, exposed):
    gains = GAINS[n_gains]
    img, gauges, widths = cd_layout(n, axis, exposed)
    img = img[:planes]
    want, runs = memo(("cd", n, axis, planes, n_gains, exposed), lambda: cd_reference(img, gauges, gains, exposed))
    gi = int(np.argmin(np.abs(np.array(gains) - 1.0)))                         # the gain next to 1: the runs are as they were laid out
    seen = set((runs[gi, 0, :, 1] - runs[gi, 0, :, 0] + 1)[runs[gi, 0, :, 0] >= 0].tolist())
    assert set(widths) <= seen, (widths, seen)                                  # every run width is there, plane 0
    assert bool((want[gi, 0, :, 0] == 0).any()) == (n > 1) and bool(np.isnan(want[gi, 0, -5:]).all())    # beside a run; invalid gauges
    if n >= 130:                                                               # gauges at both ends of the 129-wide run: three chunks
        assert 129 in seen and (0, n - 1) in {(int(lo), int(hi)) for lo, hi in runs[gi, 0]}
    g, G = floats(gains), len(gauges)

    def call(p, st):
        return nat.lib().litho_measure_cd(p["image"], planes, n, p["gauges"], G, g, n_gains, T, int(exposed), PS, p["out"], st)
    return Case("litho_measure_cd", (n, axis), f"{planes} planes, {n_gains} gains, exposed {int(exposed)}",
                [("image", tensor(img)), ("gauges", tensor(np.array(gauges, dtype=np.int32)))], {"out": tensor(want)}, call, max(plane_guard(n), (5 * G + 5 + 4) * 4))


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 64, 65, 130, 200])
def test_measure_cd(nat, dev, n, axis):
    combos = [(1, 1), (3, 3), (1, 64), (3, 1), (1, 3)] + ([(3, 64)] if n == 65 else [])
    for i, (planes, n_gains) in enumerate(combos):
        for exposed in ((True, False) if i < 3 else (bool((i + axis) % 2),)):
            run(nat, dev, cd_case(nat, n, axis, planes, n_gains, exposed), full=(planes, n_gains, exposed) == (3, 3, True))


# ---- dose-focus envelope ---------------------------------------------------------------------------------------------------------
def envelope_case(nat, n, planes, n_gains):
    gains = GAINS[n_gains]
    u = np.random.default_rng(50 + n).uniform(-0.5, 2.0, (3, n, n)).astype(F)[:planes].copy()
    u[0, n // 2, n // 3] = np.nan                                              # alone (1 plane): NaN out; among others: skipped
    prod = np.stack([CO.products(u[p], g) for p in range(planes) for g in gains])
    lo, hi = np.fmin.reduce(prod, axis=0), np.fmax.reduce(prod, axis=0)
    assert bool(np.isnan(lo[n // 2, n // 3])) == (planes == 1) and int(np.isnan(lo).sum()) == int(planes == 1)
    g = floats(gains)

    def call(p, st):
        return nat.lib().litho_dose_focus_envelope(p["image"], planes, n, g, n_gains, p["lo"], p["hi"], st)
    return Case("litho_dose_focus_envelope", (n, planes, n_gains), "a NaN sample", [("image", tensor(u))], {"lo": tensor(lo), "hi": tensor(hi)},
                call, plane_guard(n))


@pytest.mark.parametrize("n_gains", [1, 64])
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_dose_focus_envelope(nat, dev, n, planes, n_gains):
    run(nat, dev, envelope_case(nat, n, planes, n_gains))


# ---- rasteriser and area coverage ------------------------------------------------------------------------------------------------
X0, Y0, PIXEL = 10.0, -20.0, 8.0


def edge_list(pn, ne):
    """Exactly `ne` edges [ne, 4] fp64 in the window [X0, X0 + pn PIXEL] x [Y0, Y0 + pn PIXEL]: counter-clockwise rectangles that stick
    out of it on each of the four sides (the crossing column clips to 0 and to pn), one wholly outside, one narrow and taller than
    the window, a NaN, a +inf and a -inf edge, and a many-cornered polygon that fills the count; horizontals in every rectangle.
    One edge: a single upward one through the whole window."""
    span = pn * PIXEL
    if ne == 0:
        return np.zeros((0, 4))
    if ne == 1:
        return np.array([[X0 + 0.37 * span, Y0 - 0.5 * span, X0 + 0.61 * span, Y0 + 1.5 * span]])

    def rect(xa, ya, xb, yb):
        q = np.array([[xa, ya], [xb, ya], [xb, yb], [xa, yb]])
        return np.concatenate([q, np.roll(q, -1, axis=0)], axis=1)
    parts = [rect(-0.31, 0.21, 0.42, 0.52), rect(0.63, 0.33, 1.3, 0.71), rect(0.22, -0.4, 0.44, 0.31), rect(0.55, 0.62, 0.83, 1.5),
             rect(1.2, 1.2, 1.6, 1.7), rect(0.47, -0.2, 0.53, 1.2)]
    k = ne - 27
    assert k >= 3
    ang = 2 * np.pi * (np.arange(k) + 0.25) / k
    rad = 0.3 + 0.17 * np.cos(5 * ang)
    q = np.stack([0.5 + rad * np.cos(ang), 0.48 + rad * np.sin(ang)], axis=1)
    parts.append(np.concatenate([q, np.roll(q, -1, axis=0)], axis=1))
    e = np.concatenate(parts) * span + np.array([X0, Y0, X0, Y0])
    bad = np.array([[np.nan, Y0 + 0.1 * span, X0 + 0.5 * span, Y0 + 0.9 * span], [X0 + 0.2 * span, np.inf, X0 + 0.2 * span, Y0 + 0.3 * span],
                    [X0 + 0.1 * span, Y0 + 0.2 * span, -np.inf, Y0 + 0.4 * span]])
    e = np.concatenate([e[:11], bad[:1], e[11:200], bad[1:], e[200:]])
    assert e.shape == (ne, 4) and int((e[:, 1] == e[:, 3]).sum()) >= 12
    return np.ascontiguousarray(e)


def raster_case(nat, pn, ne):
    edges = edge_list(pn, ne)
    want = memo(("raster", pn, ne), lambda: LO.rasterize_edges(edges, pn, X0, Y0, PIXEL))
    assert set(np.unique(want).tolist()) <= {0, 1} and want.dtype == np.int16
    if ne >= 255 and pn >= 2:
        assert 0 < int(want.sum()) < pn * pn and want[:, 0].any() and want[:, -1].any() and want[0].any() and want[-1].any()
    need = pn * (pn + 1) * 4
    assert nat is None or int(nat.lib().litho_rasterize_work_bytes(pn)) == need

    def call(p, st):
        return nat.lib().litho_rasterize_edges(p.get("edges"), ne, pn, X0, Y0, PIXEL, p["work"], p["work_bytes"], p["geometry"], st)
    ins = [("edges", tensor(edges))] if ne else []
    return Case("litho_rasterize_edges", (pn, ne), "edges NULL" if not ne else "mixed edges", ins, {"geometry": tensor(want)}, call,
                need + (pn + 1 + 4) * 4, work_bytes=need)


@pytest.mark.parametrize("ne", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("pn", [1, 2, 255, 256, 257, 300])
def test_rasterize_edges(nat, dev, pn, ne):
    run(nat, dev, raster_case(nat, pn, ne), full=ne in (0, 257))


COVERAGE = [(1, 1), (1, 16), (5, 2), (64, 1), (130, 2), (33, 4), (65, 8), (64, 16), (65, 16)]


def coverage_case(nat, pn, s, band, ne=257):
    edges = edge_list(pn, ne)
    want = memo(("coverage", pn, s, ne), lambda: VO.coverage(edges, pn, X0, Y0, PIXEL, s))
    if ne == 257:
        assert pn < 33 or (float(want.max()) == 1.0 and float(want.min()) == 0.0 and (s == 1 or bool(((want > 0) & (want < 1)).any())))
        tall = np.nanmax(np.where(np.isfinite(edges).all(axis=1), np.abs(edges[:, 3] - edges[:, 1]), 0.0)) / (PIXEL / s)
        assert tall > pn * s and (pn * s <= 128 or tall > 128)                  # an edge through every sub-row: every k_cov_edges chunk
    need = band * s * (pn * s + 1) * 4
    assert nat is None or int(nat.lib().litho_rasterize_coverage_work_bytes(pn, s, band)) == need

    def call(p, st):
        return nat.lib().litho_rasterize_coverage(p.get("edges"), ne, pn, X0, Y0, PIXEL, s, p["work"], p["work_bytes"], p["coverage"], st)
    ins = [("edges", tensor(edges))] if ne else []
    bands = -(-pn // band)
    return Case("litho_rasterize_coverage", (pn, s), f"{ne} edges, {band} band rows ({bands} bands, the last of {pn - (bands - 1) * band})",
                ins, {"coverage": tensor(want)}, call, need + (pn * s + 1 + 4) * 4, work_bytes=need)


@pytest.mark.parametrize("pn,s", COVERAGE, ids=[f"{pn}-{s}" for pn, s in COVERAGE])
def test_rasterize_coverage(nat, dev, pn, s):
    for band in sorted({1, min(3, pn), pn}):
        run(nat, dev, coverage_case(nat, pn, s, band), full=band == min(3, pn) and pn * s <= 520)
    if (pn, s) == (33, 4):
        for ne in (0, 1, 255, 256):
            run(nat, dev, coverage_case(nat, pn, s, 3, ne), full=False)


# ---- refused calls launch nothing ------------------------------------------------------------------------------------------------
def refused(nat, dev, case, label, expected, mods=None, work_bytes=None, call=None):
    a = case.arena(dev, mods, work_bytes)
    rc = invoke(nat, dev, case, a, call=call)
    touched = [nm for nm in list(case.outs) + ["work"] if not a.still_poison(nm)]
    rep = a.report(case.outs)
    print(f"{case.entry} {case.shape}, {label}: return code {rc}; outputs and workspace {'still poison' if not touched else touched}")
    assert rc == expected and not touched and not rep.guards and not rep.inputs, (label, rc, touched, str(rep))


@pytest.mark.parametrize("which", ["count", "emit"])
def test_a_refused_contour_workspace_launches_nothing(nat, dev, which):
    case = contour_case(nat, 64, 3, 3, True)
    call = getattr(case, which)
    for mod in (4, 12):
        refused(nat, dev, case, f"{which}, workspace at {mod} mod 16", nat.E_ARG, mods={"work": mod}, call=call)
    refused(nat, dev, case, f"{which}, workspace one byte short", nat.E_WORKSPACE, work_bytes=case.work_bytes - 1, call=call)


def test_a_refused_raster_workspace_launches_nothing(nat, dev):
    case = raster_case(nat, 257, 257)
    refused(nat, dev, case, "workspace one byte short", nat.E_WORKSPACE, work_bytes=case.work_bytes - 1)
    case = coverage_case(nat, 33, 4, 1)
    refused(nat, dev, case, "less than one band row", nat.E_WORKSPACE, work_bytes=case.work_bytes - 1)


# ---- f: side streams -------------------------------------------------------------------------------------------------------------
def test_every_entry_on_a_side_stream(nat, dev, side):
    for case in (contour_case(nat, 64, 3, 3, True), contour_case(nat, 65, 2, 64, False), epe_case(nat, 126, 257, 32.0, 3, 64, True),
                 cd_case(nat, 130, 1, 3, 3, True), envelope_case(nat, 17, 3, 64), raster_case(nat, 257, 257), raster_case(nat, 2, 0),
                 coverage_case(nat, 65, 16, 3), coverage_case(nat, 130, 2, 1), coverage_case(nat, 64, 1, 64)):
        run(nat, dev, case, side)


# ---- the harness bites -----------------------------------------------------------------------------------------------------------
def test_the_harness_reports_a_write_outside_a_buffer(nat, dev):
    """A correct call, then ordinary torch assignments inside the arena: one fp32 just behind xy, one int32 just in front of the
    workspace, one element of next put back to all-ones.  No kernel is made to misbehave; the report must name the three places."""
    case = contour_case(nat, 64, 3, 3, True)
    a = case.arena(dev)
    assert invoke(nat, dev, case, a) == nat.LITHO_OK and a.report(case.outs).clean
    xy, w = a.bufs["xy"], a.bufs["work"]
    a.bytes[xy.end:xy.end + 4].view(torch.float32)[0] = 1.0                    # 0x3f800000: every byte differs from 0xFF
    a.bytes[w.start - 4:w.start].view(torch.int32)[0] = 0
    rep = a.report(case.outs)
    print(f"planted: one fp32 behind xy, one int32 in front of the workspace; reported: {rep}")
    assert rep.guards == [("xy", xy.nbytes + i) for i in range(4)] + [("work", -4 + i) for i in range(4)]
    assert not rep.inputs and not rep.unwritten and not rep.clean
    a["next"][1234] = -1
    rep = a.report(case.outs)
    print(f"planted: next[1234] all-ones; reported: {rep}")
    assert rep.unwritten == [("next", 4 * 1234)] and differing(a["next"], case.outs["next"]) == [4 * 1234]
