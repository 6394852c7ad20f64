"""Where the Abbe engine reads and writes inside its workspace (csrc/abbe_engine.hip, engine_kernels.hpp, wave_kernels.hpp):
litho_abbe_accumulate_opts / _weighted / _counted / _planned through the raw C ABI, every device buffer of a call -- maskFT, pupil,
shifts, weights, count_dev, `out`, the workspace -- inside ONE guarded, poisoned arena (tests/arena.py), and the device held to what
litho_abbe_plan_dry_run DECLARES for the call, byte range by byte range.  tests/test_planner_cpu.py proves that the declared
regions are disjoint and inside litho_abbe_workspace_bytes without ever seeing a kernel; the numerical GPU tests run the kernels
on torch.empty workspaces, where a row written past its T share, a slab nobody counted or a read one mask row outside maskFT
lands in allocator slack.  Here the two meet.

Per call (`run` below), with options.poison left at 0 -- the arena's 0xFF is the poison: NaN as fp32, -1 as int32:
  1  no guard byte and no input byte changed; guards are one plane + one row + one pack of the call's largest plane (complex64);
  2  `out` (role "inout", prefilled with a finite, non-zero, non-constant pattern) equals prefill + oracle.abbe_oracle.abbe_raw
     within helpers.TOL_IMAGE_MAX / TOL_IMAGE_L2; from run size 2048 up (value-pinned by test_gpu_abbe.py / test_gpu_planner.py;
     the fp32 reference would take longer than the test) it equals bit for bit the same call on a torch.empty workspace outside
     any arena; every pixel is finite;
  3  ints [0, 14) of the workspace's plan region equal the words `host_words` computes from the test's own inputs (support box,
     shift extents, S, edge supports on the natural box of the grid the call runs at, corner flag), ints [32, 42) of a split call
     the host's split words; THESE words go into the dry run;
  4  the dry run's general, variant, coarse, natural_box, wave_y, xkind, batch, planes_in_flight, groups, xchunk equal
     litho_abbe_last_plan for the part that ran last; run_size is held through the launched box: litho_abbe_last_plan carries the
     box of the grid that RAN, whose first row is the host's first row + (run_size - pn) / 2 (general mode: pn rows);
  5  touched_outside("workspace", ranges) is empty, ranges = plan, twtab, twtab2, slab_used, ic_used, chat_used, gam_used, T_used,
     recon_T_used, embed_M / P / O of the present parts, list_a, list_b, split_counts of a split, and plan_scratch (the
     planning launch's partial extrema at the head of the own-size T region; absent from a call planned from a record);
  6  T_used is batch x planes in flight whatever S is.  accumulate_chunk places item (plane q, point s) of a batch of nb points
     at T + (q nb + s) t_point, contiguously from the head of T for every number of planes in flight (the plane stride is nb,
     not the planned batch), so a call never writes past min(planes in flight, planes) x min(batch, S) items: every byte of
     T_used behind that (and behind the other tenants of the head of T: reconstruction, split counts, planning scratch) is
     still 0xFF.  Asserted for every case, planes_in_flight > 1 included;
  7  the same call again into the used arena, `out` re-filled, nothing re-poisoned: the same bits;
  8  maskFT, pupil and out at 8 mod 16, shifts and weights at 4 mod 16: the aligned call's bits;
  9  one case of every group also runs on a side stream;
 10  litho_abbe_last_kernels names the case's `xk` / `yk` for the part that ran last, character for character (the spelling
     bench.py matches against rocprofv3's): the table recorded on an MI355X, which the launch layer may not change.

The case list is fixed (CASES); test_every_case_plans_as_stated (no GPU) holds every entry to its comment through the dry run.
Pupils are disks with defocus computed here in float64 (support k^2 <= (pn/4)^2, as the reference's r <= 1; one sample on each
edge of the natural box), a wide box (rows and columns 10 .. 250) and a square with set corners; masks are seeded complex noise;
source lists are a handful of strided points of the 0.4 - 0.8 annulus, shifted where a case wants wrapping.

The entries without a dry run -- litho_abbe_field, litho_mask_spectrum, litho_mask_spectrum_complex (pn 16, 64, 200, 256, 512; an
epsilon that pads and one that crops) -- get the same arena and assertions 1, 2, 7, 8, and for 5 the regions read off
abbe_engine.hip (transform_call below), references and bounds from tests/spectrum_oracle.py; litho_source_compact / _weighted run
with a scratch of exactly pn + 1 int32 and lists of exactly `capacity` entries, bit for bit, the entries beyond S still poison.
Refused calls (a workspace one byte short of the own grid's regions, a null pointer, N < pn) leave `out` as sealed and the workspace
poison.  The harness is shown to fail on the device: planted writes are reported at their offsets, and each of T_used, slab_used,
ic_used, embed_O, list_b, plan_scratch and twtab2 shortened by one 256-byte block (here, not in the library) makes assertion 5 fail.

Found by this file (LABNOTES.md, "Where the Abbe engine reads and writes inside its workspace", with the times on an MI355X): no
kernel writes outside its region; the dry run did not declare the planning scratch, nor twtab2 for a call that may go coarse but
plans direct.  Both are declared now (plan_dry_run.cpp) and kept as cases."""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

from arena import POISON, Arena, Buf, differing
from helpers import TOL_IMAGE_L2, TOL_IMAGE_MAX, rel_l2, rel_max

INT_MAX, INT_MIN = 2**31 - 1, -2**31
X_FAMILIES = ("k_xpass_abbe", "k_xpass_rect", "k_xpass_split", "k_xpass")
Y_FAMILIES = ("k_ypass_rect", "k_ypass_coop_dma", "k_ypass_wave", "k_ypass_pair", "k_ypass_acc")
KERNELS = {}                                                                   # case name -> (x-pass, y-pass) of the last part
TIMES = {}
DRY_FIELDS = (("general", "general"), ("variant", "variant"), ("coarse", "coarse_grid"), ("natural_box", "natural_box"), ("wave_y", "wave_ypass"),
              ("xkind", "fused_xpass"), ("batch", "batch"), ("planes_in_flight", "planes_in_flight"), ("groups", "groups_per_plane"),
              ("xchunk", "xchunk"))
PART_REGIONS = ("plan", "twtab", "twtab2", "slab_used", "ic_used", "chat_used", "gam_used", "T_used", "recon_T_used", "embed_M", "embed_P",
                "embed_O")


class Case:
    """One call.  `expect`: what the comment of the case says about its plan, as fields of the dry run's last part (or of the
    result: run_size, split, parts)."""

    def __init__(self, name, pn, N, opts=None, S=5, planes=1, pupil="disk", src="annular", entry="opts", ws="full", side=False, **expect):
        self.name, self.pn, self.N, self.opts, self.S, self.planes = name, pn, N, dict(opts or {}), S, planes
        self.pupil, self.src, self.entry, self.ws, self.side, self.expect = pupil, src, entry, ws, side, expect


SMALL = {"coarse": 2, "batch": 1, "groups": 1}
CASES = [
    # run size below 256: radix-16 kernels, T tile 4
    Case("16-16", 16, 16, S=3, variant=0, tile=4, wave_y=0, xk="k_xpass_abbe<4, 0, true, 1, 1>", yk="k_ypass_acc<4, 0, true>"),
    Case("16-32", 16, 32, S=3, variant=1, tile=4, wave_y=0, xk="k_xpass_abbe<5, 1, true, 1, 1>", yk="k_ypass_acc<5, 1, true>"),
    Case("16-64", 16, 64, S=3, variant=2, tile=4, wave_y=0, side=True, xk="k_xpass_abbe<6, 2, true, 1, 1>", yk="k_ypass_acc<6, 2, true>"),
    Case("30-64 generic", 30, 64, S=4, variant=-1, tile=4, wave_y=0, xk="k_xpass_abbe<6, -1, false, 1, 1>", yk="k_ypass_acc<6, -1, false>"),
    Case("64-128", 64, 128, S=7, variant=1, tile=4, wave_y=0, xk="k_xpass_abbe<7, 1, true, 1, 1>", yk="k_ypass_acc<7, 1, true>"),
    # run size 256, N 512
    Case("256 default", 256, 512, variant=1, coarse=0, wave_y=1, tile=8, xkind=1, xk="k_xpass_abbe<9, 1, true, 1, 1>", yk="k_ypass_rect<9, 8, false, 1>"),   # 5 points: below the coarse threshold
    Case("256 coarse 2", 256, 512, {"coarse": 2}, coarse=1, wave_y=1, xkind=1, side=True, xk="k_xpass_abbe<8, 0, true, 1, 1>", yk="k_ypass_rect<8, 8, true, 1>"),
    Case("256 coarse 2 gcombine 0", 256, 512, {"coarse": 2, "gcombine": 0}, coarse=1, wave_y=1, xk="k_xpass_abbe<8, 0, true, 1, 1>", yk="k_ypass_rect<8, 8, true, 1>"),
    Case("256 w64 0", 256, 512, {"coarse": 0, "w64": 0}, coarse=0, wave_y=0, variant=1, tile=4, xk="k_xpass_abbe<9, 1, true, 1, 1>", yk="k_ypass_acc<9, 1, true>"),
    Case("256 tile 4", 256, 512, {"coarse": 0, "tile": 4}, coarse=0, wave_y=0, tile=4, xk="k_xpass_abbe<9, 1, true, 1, 1>", yk="k_ypass_acc<9, 1, true>"),
    Case("256 rowpairs", 256, 512, {"coarse": 0, "rowpairs": 1}, coarse=0, wave_y=1, tile=8, xk="k_xpass_abbe<9, 1, true, 1, 1>", yk="k_ypass_rect<9, 8, false, 1>"),
    Case("256 w64x", 256, 512, {"coarse": 0, "w64x": 1}, coarse=0, tile=4, xk="k_xpass_abbe<9, 1, true, 1, 1>", yk="k_ypass_acc<9, 1, true>"),
    Case("256 force_generic", 256, 512, {"coarse": 0, "force_generic": 1}, coarse=0, variant=-1, wave_y=0, xkind=0, xk="k_xpass_abbe<9, -1, false, 1, 1>", yk="k_ypass_acc<9, -1, false>"),
    Case("256 force_general", 256, 512, {"force_general": 1}, general=1, variant=-1, coarse=0, xkind=0, xk="k_xpass<9, 1, litho::AbbeLoader>", yk="k_ypass_acc<9, -1, false>"),
    Case("256 wrapping list", 256, 512, src="wrap", general=1, variant=-1, split=0, xk="k_xpass<9, 1, litho::AbbeLoader>", yk="k_ypass_acc<9, -1, false>"),   # general mode by itself
    Case("256 wide pupil", 256, 512, pupil="wide", src="tiny", general=0, natural_box=0, variant=-1, wave_y=0, coarse=0, xk="k_xpass_abbe<9, -1, false, 1, 1>", yk="k_ypass_acc<9, -1, false>"),   # shifts of at most 5
    Case("256 square corners", 256, 512, {"coarse": 2}, pupil="square", coarse=0, natural_box=1, wave_y=1, xk="k_xpass_abbe<9, 1, true, 1, 1>", yk="k_ypass_rect<9, 8, false, 1>"),
    # small geometry at 256: what makes assertion 5 sharp (5.5 MiB declared of 293.5)
    Case("256 small fold", 256, 512, SMALL, S=70, coarse=1, batch=1, groups=1, xk="k_xpass_abbe<8, 0, true, 1, 1>", yk="k_ypass_rect<8, 8, true, 1>"),   # the slabs fold after 64 batches
    Case("256 small ragged planes", 256, 512, {"coarse": 2, "batch": 2, "groups": 2, "plane_chunk": 2}, S=7, planes=3, coarse=1, batch=2,
         planes_in_flight=2, side=True, xk="k_xpass_abbe<8, 0, true, 1, 1>", yk="k_ypass_rect<8, 8, true, 1>"),
    Case("256 small ragged xchunk", 256, 512, {"coarse": 0, "batch": 3, "xchunk": 2}, S=7, coarse=0, batch=3, xchunk=2, xk="k_xpass_abbe<9, 1, true, 1, 1>", yk="k_ypass_rect<9, 8, false, 1>"),
    # other run sizes and the remaining kernel families
    Case("256-256", 256, 256, variant=0, wave_y=1, xk="k_xpass_abbe<8, 0, true, 1, 1>", yk="k_ypass_rect<8, 8, true, 1>"),
    Case("512-512", 512, 512, S=3, variant=0, wave_y=1, xk="k_xpass_abbe<9, 0, true, 1, 1>", yk="k_ypass_rect<9, 8, true, 1>"),
    Case("512 rect", 512, 1024, {"coarse": 0}, S=3, coarse=0, xkind=3, wave_y=1, xk="k_xpass_rect<10, false>", yk="k_ypass_rect<10, 8, false, 1>"),
    Case("512 xrect 0", 512, 1024, {"coarse": 0, "xrect": 0}, S=3, coarse=0, xkind=1, wave_y=1, xk="k_xpass_abbe<10, 1, true, 1, 1>", yk="k_ypass_rect<10, 8, false, 1>"),
    Case("512 rect 0", 512, 1024, {"coarse": 0, "rect": 0}, S=3, coarse=0, wave_y=1, xk="k_xpass_rect<10, false>", yk="k_ypass_wave<10, 8, false>"),
    Case("1024 coarse 2", 1024, 2048, {"coarse": 2}, S=12, coarse=1, xchunk=12, xk="k_xpass_abbe<10, 0, true, 1, 1>", yk="k_ypass_rect<10, 8, true, 2>"),
    Case("2048 coarse 2", 2048, 4096, {"coarse": 2}, S=2, coarse=1, wave_y=1, xk="k_xpass_abbe<11, 0, true, 1, 1>", yk="k_ypass_rect<11, 8, true, 2>"),
    Case("2048 coarse 0", 2048, 4096, {"coarse": 0}, S=2, coarse=0, wave_y=1, xkind=1, side=True, xk="k_xpass_abbe<12, 1, true, 1, 1>", yk="k_ypass_wave<12, 8, false>"),
    # launches no other case names: k_xpass_rect with every bin kept, k_ypass_rect's combined groups on the direct path, k_xpass_w64
    Case("512-512 xrect 2", 512, 512, {"xrect": 2}, S=3, variant=0, xkind=3, wave_y=1, xk="k_xpass_rect<9, true>", yk="k_ypass_rect<9, 8, true, 1>"),
    Case("512 rect groups 2", 512, 1024, {"coarse": 0, "groups": 2}, S=4, coarse=0, xkind=3, wave_y=1, groups=2, xk="k_xpass_rect<10, false>", yk="k_ypass_rect<10, 8, false, 2>"),
    Case("2048 coarse 0 w64x", 2048, 4096, {"coarse": 0, "w64x": 1}, S=2, coarse=0, xkind=0, wave_y=1, tile=4, xk="k_xpass_w64<12>", yk="k_ypass_wave<12, 4, false>"),
    # embedded sizes
    Case("200 embedded", 200, 512, SMALL, run_size=256, coarse=1, embedded=1, xk="k_xpass_abbe<8, 0, true, 1, 1>", yk="k_ypass_rect<8, 8, true, 1>"),
    Case("300 embedded", 300, 1024, {"coarse": 2}, S=3, run_size=512, coarse=1, embedded=1, xk="k_xpass_abbe<9, 0, true, 1, 1>", yk="k_ypass_rect<9, 8, true, 1>"),
    Case("200 wrapping list", 200, 512, src="wrap", run_size=256, part_size=200, general=1, embedded=0, xk="k_xpass<9, 1, litho::AbbeLoader>", yk="k_ypass_acc<9, -1, false>"),   # refuses the embedding
    Case("200 embed 0", 200, 512, {"embed": 0}, run_size=200, variant=-1, embedded=0, xk="k_xpass_abbe<9, -1, false, 1, 1>", yk="k_ypass_acc<9, -1, false>"),
    Case("200 own-size workspace", 200, 512, ws="own", run_size=200, variant=-1, embedded=0, xk="k_xpass_abbe<9, -1, false, 1, 1>", yk="k_ypass_acc<9, -1, false>"),
    # split lists: part 0 keeps the fast path, part 1 runs general mode
    Case("256 split", 256, 512, {"split": 2, "coarse": 2, "batch": 4, "groups": 2}, S=20, src="partial", split=1, parts=2, general=1, side=True, xk="k_xpass<9, 1, litho::AbbeLoader>", yk="k_ypass_acc<9, -1, false>"),
    Case("200 split embedded", 200, 512, {"split": 2, "coarse": 2, "batch": 4, "groups": 2}, S=20, src="partial", split=1, parts=2, general=1,
         run_size=256, part_size=200, part0_size=256, xk="k_xpass<9, 1, litho::AbbeLoader>", yk="k_ypass_acc<9, -1, false>"),
    # the other entries, three representative plans each
    Case("weighted 256 coarse", 256, 512, SMALL, S=6, entry="weighted", coarse=1, xk="k_xpass_abbe<8, 0, true, 1, 1, float const*>", yk="k_ypass_rect<8, 8, true, 1>"),
    Case("weighted 64", 64, 128, S=6, entry="weighted", variant=1, xk="k_xpass_abbe<7, 1, true, 1, 1, float const*>", yk="k_ypass_acc<7, 1, true>"),
    Case("weighted 200 embedded", 200, 512, SMALL, S=6, entry="weighted", run_size=256, xk="k_xpass_abbe<8, 0, true, 1, 1, float const*>", yk="k_ypass_rect<8, 8, true, 1>"),
    Case("counted 256 coarse", 256, 512, SMALL, S=6, entry="counted", coarse=1, xk="k_xpass_abbe<8, 0, true, 1, 1>", yk="k_ypass_rect<8, 8, true, 1>"),
    Case("counted 30", 30, 64, S=4, entry="counted", variant=-1, xk="k_xpass_abbe<6, -1, false, 1, 1>", yk="k_ypass_acc<6, -1, false>"),
    Case("counted 200 embedded", 200, 512, SMALL, S=6, entry="counted", run_size=256, xk="k_xpass_abbe<8, 0, true, 1, 1>", yk="k_ypass_rect<8, 8, true, 1>"),
    Case("planned 256 coarse", 256, 512, SMALL, S=6, entry="planned", coarse=1, xk="k_xpass_abbe<8, 0, true, 1, 1>", yk="k_ypass_rect<8, 8, true, 1>"),
    Case("planned 64", 64, 128, S=6, entry="planned", variant=1, xk="k_xpass_abbe<7, 1, true, 1, 1>", yk="k_ypass_acc<7, 1, true>"),
    Case("planned 256 split", 256, 512, {"split": 2, "coarse": 2, "batch": 4, "groups": 2}, S=20, src="partial", entry="planned", split=1,
         parts=2, xk="k_xpass<9, 1, litho::AbbeLoader>", yk="k_ypass_acc<9, -1, false>"),
    # the weighted x-pass siblings no other name-asserting test reaches: k_xpass_rect (both FULL values) and the general x-pass
    Case("weighted 512 rect", 512, 1024, {"coarse": 0}, S=3, entry="weighted", coarse=0, xkind=3, wave_y=1, xk="k_xpass_rect<10, false, float const*>", yk="k_ypass_rect<10, 8, false, 1>"),
    Case("weighted 512-512 xrect 2", 512, 512, {"xrect": 2}, S=3, entry="weighted", variant=0, xkind=3, wave_y=1, xk="k_xpass_rect<9, true, float const*>", yk="k_ypass_rect<9, 8, true, 1>"),
    Case("weighted 64 wrapping list", 64, 128, S=6, src="wrap", entry="weighted", general=1, variant=-1, split=0, xk="k_xpass<7, 1, litho::AbbeLoaderW>", yk="k_ypass_acc<7, -1, false>"),
]
# 4096^2: two points and a 5 GiB workspace; the four calls run in turn in ONE arena (and one more with the other alignment)
BIG = [Case("4096 coarse 2 coopdma 1", 4096, 8192, {"coarse": 2, "coopdma": 1}, S=2, coarse=1, tile=16, wave_y=1, xk="k_xpass_abbe<12, 0, true, 1, 1>", yk="k_ypass_coop_dma<12, 4>"),
       Case("4096 coarse 2 coopdma 0", 4096, 8192, {"coarse": 2, "coopdma": 0}, S=2, coarse=1, tile=16, wave_y=1, xk="k_xpass_abbe<12, 0, true, 1, 1>", yk="k_ypass_coop<12, 4>"),
       Case("4096 coarse 0", 4096, 8192, {"coarse": 0}, S=2, coarse=0, xkind=2, wave_y=1, xk="k_xpass_split<13>", yk="k_ypass_pair<13, 8>"),
       Case("4096 coarse 0 weighted", 4096, 8192, {"coarse": 0}, S=2, entry="weighted", coarse=0, xkind=2, wave_y=1, xk="k_xpass_split<13, float const*>", yk="k_ypass_pair<13, 8>")]
BY_NAME = {c.name: c for c in CASES + BIG}
assert len(BY_NAME) == len(CASES) + len(BIG)


# ---- the inputs of a case, on the CPU: the dry-run check needs no device ---------------------------------------------------------
_INPUTS = {}


def disk_pupil(pn, plane):
    k = (np.arange(pn) - pn // 2) / (pn / 4.0)
    r2 = k[:, None] ** 2 + k[None, :] ** 2
    return np.where(r2 <= 1.0, np.exp(1j * math.pi * (0.35 + 0.2 * plane) * (2.0 * r2 - 1.0)), 0.0).astype(np.complex64)


def annulus_points(pn, K, sin=0.4, sout=0.8):
    """K strided points of the annulus (K None: all of them), as (dy, dx), in row-major order."""
    R = pn / 4.0
    d = np.arange(pn) - pn // 2
    rr = np.hypot(d[:, None], d[None, :])
    pts = np.argwhere((rr >= sin * R) & (rr <= sout * R)) - pn // 2           # row-major, as litho_source_compact writes them
    if K is None:
        return pts.astype(np.int32)
    assert len(pts) >= K, (pn, len(pts))
    return pts[(np.arange(K) * len(pts)) // K].astype(np.int32)


def inputs(case):
    """(maskFT [pn, pn] c64, pupil [planes, pn, pn] c64, shifts [S, 2] int32, weights [S] fp32) as CPU tensors, made once."""
    key = (case.pn, case.planes, case.pupil, case.src, case.S)
    if key not in _INPUTS:
        pn, c, h = case.pn, case.pn // 2, case.pn // 4
        gen = torch.Generator().manual_seed(1000 * pn + case.S)
        mft = torch.polar(0.5 + torch.rand(pn, pn, generator=gen), 6.2831853 * torch.rand(pn, pn, generator=gen)).to(torch.complex64)
        if case.pupil == "disk":
            pupil = torch.from_numpy(np.stack([disk_pupil(pn, p) for p in range(case.planes)]))
        else:
            lo, hi = (10, 250) if case.pupil == "wide" else (c - h, c + h)
            pupil = torch.zeros(case.planes, pn, pn, dtype=torch.complex64)
            n = hi - lo + 1
            pupil[:, lo:hi + 1, lo:hi + 1] = torch.polar(0.5 + 0.5 * torch.rand(case.planes, n, n, generator=gen),
                                                         6.2831853 * torch.rand(case.planes, n, n, generator=gen)).to(torch.complex64)
        sh = annulus_points(pn, case.S, 0.03, 0.078) if case.src == "tiny" else annulus_points(pn, case.S)
        if case.src == "wrap":
            sh[:, 0] += 2 * h                                                  # dy in [1.2 h, 2.8 h]: every point wraps the disk's box
        elif case.src == "partial":
            sh[:, 1] += h // 2                                                 # dx in [-0.3 h, 1.3 h]: the points beyond h - 1 wrap
        weights = (0.5 + torch.rand(case.S, generator=gen)).to(torch.float32)
        weights[case.S // 2] = 0.0
        _INPUTS[key] = (mft, pupil, torch.from_numpy(sh), weights)
    return _INPUTS[key]


def host_words(pupil, shifts, pn, pe):
    """The 14 plan words and the split's ten words, from the inputs (k_plan_gather / k_plan_finish / k_split_* restated)."""
    nz = (pupil != 0).any(0).numpy()
    rows, cols = np.flatnonzero(nz.any(1)), np.flatnonzero(nz.any(0))
    sh = shifts.numpy().astype(np.int64)
    w = [int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1]), int(sh[:, 0].min()), int(sh[:, 0].max()), int(sh[:, 1].min()),
         int(sh[:, 1].max()), len(sh)]
    edges = [e for e in (pn // 2 - pe // 4, pn // 2 + pe // 4) if 0 <= e < pn]
    er = np.flatnonzero(nz[:, edges].any(1)) if edges else np.array([], dtype=int)
    ec = np.flatnonzero(nz[edges, :].any(0)) if edges else np.array([], dtype=int)
    w += [int(er[0]), int(er[-1])] if len(er) else [INT_MAX, INT_MIN]
    w += [int(ec[0]), int(ec[-1])] if len(ec) else [INT_MAX, INT_MIN]
    w.append(int(any(nz[r, c] for r in edges for c in edges)))
    wraps = (w[0] + sh[:, 0] < 0) | (w[1] + sh[:, 0] > pn - 1) | (w[2] + sh[:, 1] < 0) | (w[3] + sh[:, 1] > pn - 1)
    sw = [int((~wraps).sum()), int(wraps.sum())]
    for part in (sh[~wraps], sh[wraps]):
        sw += [int(part[:, 0].min()), int(part[:, 0].max()), int(part[:, 1].min()), int(part[:, 1].max())] if len(part) else [INT_MAX, INT_MIN] * 2
    return w, sw, wraps


class Planned:
    """What the dry run says about a case, from host-computed words."""

    def __init__(self, nat, case, cus=256):
        pn, N = case.pn, case.N
        mft, pupil, shifts, weights = inputs(case)
        size, emb = ctypes.c_size_t(0), ctypes.c_int(0)
        assert nat.lib().litho_abbe_workspace_bytes(pn, N, ctypes.byref(size)) == 0
        assert nat.lib().litho_abbe_embedded_size(pn, N, ctypes.byref(emb)) == 0
        self.full_bytes = size.value
        own = nat.plan_dry_run(pn, N, case.planes, [0, pn - 1, 0, pn - 1, 0, 0, 0, 0, 1] + [INT_MAX, INT_MIN] * 2 + [0], options={"embed": 0})
        self.own_bytes = own.part[0].T_region.end                              # the regions of the call's own size only
        self.ws_bytes = self.own_bytes if case.ws == "own" else self.full_bytes
        self.pe = emb.value if case.opts.get("embed", 1) and self.ws_bytes == self.full_bytes else pn
        self.words, sw, self.wraps = host_words(pupil, shifts, pn, self.pe)
        nowrap = not self.wraps.any()
        # (a weighted list is never split; the others when options.split says so: 2 = always)
        may_split = case.entry != "weighted" and not nowrap and not case.opts.get("force_general", 0) and (case.opts.get("split", 1) >= 2 or case.S >= 256)
        self.sw = sw if may_split else None
        self.dry = nat.plan_dry_run(pn, N, case.planes, self.words, self.sw, options=case.opts, cus=cus,
                                    workspace_bytes=0 if case.ws == "full" else self.ws_bytes)
        assert self.dry.status == 0 and self.dry.workspace_bytes == self.full_bytes and self.dry.run_size == self.pe, (case.name, self.dry.status)
        self.parts = [p for p in self.dry.part if p.present]
        self.last = self.parts[-1]

    def ranges(self, planning=True):
        out = {}
        for i, p in enumerate(self.parts):
            for name in PART_REGIONS:
                r = getattr(p, name)
                if r.bytes:
                    out[f"{name}[{i}]"] = (r.offset, r.bytes)
        if self.dry.split:
            for name in ("list_a", "list_b", "split_counts"):
                r = getattr(self.dry, name)
                out[name] = (r.offset, r.bytes)
        if planning:
            out["plan_scratch"] = (self.dry.plan_scratch.offset, self.dry.plan_scratch.bytes)
        return out


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    assert _native.lib().litho_target_arch() == b"gfx950"
    return _native


# ---- no GPU: the case list plans as its comments say -----------------------------------------------------------------------------
def test_every_case_plans_as_stated(nat):
    seen = []
    for case in CASES + BIG:
        pl = Planned(nat, case)
        last, exp = pl.last, dict(case.expect)
        assert pl.dry.split == exp.pop("split", 0) and len(pl.parts) == exp.pop("parts", 1), case.name
        assert pl.dry.run_size == exp.pop("run_size", case.pn), (case.name, pl.dry.run_size)
        assert last.run_size == exp.pop("part_size", pl.dry.run_size), (case.name, last.run_size)
        assert pl.parts[0].run_size == exp.pop("part0_size", pl.parts[0].run_size), case.name
        exp.pop("xk", None), exp.pop("yk", None)                               # the kernels of the last part: held on the device (check_call)
        embedded = exp.pop("embedded", None)
        if embedded is not None:
            assert (pl.parts[0].embed_M.bytes > 0) == bool(embedded), case.name
        for k, v in exp.items():
            assert getattr(last, k) == v, (case.name, k, getattr(last, k), v)
        if pl.dry.split:
            assert pl.parts[0].general == 0 and pl.parts[1].general == 1 and 0 < pl.sw[0] < case.S, (case.name, pl.sw)
        # the planning scratch: at the head of the own-size T region, inside the workspace the call passes, clear of the lists
        scratch, own = pl.dry.plan_scratch, nat.plan_dry_run(case.pn, case.N, case.planes, pl.words, pl.sw, options=dict(case.opts, embed=0))
        assert scratch.offset == own.part[0].T_region.offset and 0 < scratch.bytes and scratch.end <= own.part[0].T_region.end <= pl.ws_bytes
        assert scratch.bytes == ((case.pn + 7) // 8 * case.planes + 1) * 64 and (not pl.dry.split or scratch.end <= pl.dry.list_a.offset)
        total = sum(n for _, n in pl.ranges().values())
        seen.append((case.name, last.run_size, last.variant, last.coarse, last.wave_y, last.xkind, last.batch, last.groups, last.tile, total,
                     pl.ws_bytes))
    for row in seen:
        print("%-30s run %5d variant %2d coarse %d wave_y %d xkind %d batch %5d groups %3d tile %2d declares %11d of %11d bytes" % row)
    # the small geometry is what makes the byte check sharp: a few MiB declared of 293.5
    small = Planned(nat, BY_NAME["256 small fold"])
    assert sum(n for _, n in small.ranges().values()) < 8 << 20 and small.ws_bytes > 290 << 20
    # the 70-point case folds its slabs once in mid-run (after 64 batches) and goes a second round
    assert small.last.batch == 1 and BY_NAME["256 small fold"].S > 64


# ---- the device ------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def side(dev):
    return torch.cuda.Stream(dev)


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


_REFS = {}


def reference(case):
    """oracle.abbe_raw per plane (weighted: point by point, sum of w_s |E_s|^2 in float64), made once per input set."""
    from oracle import abbe_oracle as O
    key = (case.pn, case.N, case.planes, case.pupil, case.src, case.S, case.entry == "weighted")
    if key not in _REFS:
        mft, pupil, shifts, weights = inputs(case)
        if case.entry == "weighted":
            ref = torch.stack([sum(float(weights[s]) * O.abbe_raw(mft, pupil[p], shifts[s:s + 1], case.N).double() for s in range(case.S))
                               for p in range(case.planes)])
        else:
            ref = torch.stack([O.abbe_raw(mft, pupil[p], shifts, case.N).double() for p in range(case.planes)])
        _REFS[key] = ref
    return _REFS[key]


def prefill(planes, pn):
    i = torch.arange(planes * pn * pn, dtype=torch.float64)
    return (0.5 + (i % 97) / 97.0 + (i % 13) / 64.0).to(torch.float32).reshape(planes, pn, pn)


def make_arena(case, pl, dev, odd=False, capacity=None, ws_bytes=None, weights=False):
    """`weights`: a weights buffer for a case that takes none itself (an arena that a weighted case will run in later)."""
    pn, cap = case.pn, capacity or case.S
    m8, m4 = (8, 4) if odd else (0, 0)
    bufs = [Buf("maskFT", "in", torch.complex64, (pn, pn), m8), Buf("pupil", "in", torch.complex64, (case.planes, pn, pn), m8),
            Buf("shifts", "in", torch.int32, (cap, 2), m4)]
    if case.entry == "weighted" or weights:
        bufs.append(Buf("weights", "in", torch.float32, (cap,), m4))
    if case.entry in ("counted", "planned"):
        bufs.append(Buf("count_dev", "in", torch.int32, (1,), m4))
    bufs += [Buf("out", "inout", torch.float32, (case.planes, pn, pn), m8), Buf("workspace", "work", torch.uint8, (ws_bytes or pl.ws_bytes,), 0)]
    a = Arena(bufs, (pn * pn + pn + 4) * 8, device=dev)
    assert a.ptr("workspace") % 256 == 0 and a.bufs["workspace"].nbytes == (ws_bytes or pl.ws_bytes)
    mft, pupil, shifts, weights = inputs(case)
    a.fill("maskFT", mft.to(dev))
    a.fill("pupil", pupil.to(dev))
    a["shifts"][:case.S].copy_(shifts.to(dev))                                 # (capacity > S: the tail stays poison)
    if "weights" in a.bufs:
        a["weights"][:case.S].copy_(weights.to(dev))
    if "count_dev" in a.bufs:
        a["count_dev"].fill_(case.S)
    a.fill("out", prefill(case.planes, pn).to(dev))
    a.seal()
    return a


def launch(nat, case, ptrs, ws_bytes, capacity, stream, weights="own", record=None):
    """The raw call; ptrs: name -> device address.  Returns (rc, count_host)."""
    lib, cnt = nat.lib(), ctypes.c_int64(-7)
    opts = nat.Options.make(case.opts)
    vp = lambda name: ctypes.c_void_p(ptrs[name]) if ptrs.get(name) else None
    head = (vp("maskFT"), vp("pupil"), case.planes, vp("shifts"), vp("count_dev"), capacity, case.pn, case.N, vp("out"), vp("workspace"),
            ws_bytes, ctypes.c_void_p(stream.cuda_stream))
    rec = ctypes.byref(record) if record is not None else None
    if case.entry == "weighted":
        rc = lib.litho_abbe_accumulate_weighted(*head, rec, ctypes.byref(opts), ctypes.byref(cnt), vp("weights") if weights == "own" else weights)
    elif case.entry == "counted" and not case.opts:
        rc = lib.litho_abbe_accumulate_counted(*head, ctypes.byref(cnt))
    elif case.entry == "planned" and not case.opts and record is not None:
        rc = lib.litho_abbe_accumulate_planned(*head, rec, ctypes.byref(cnt))
    else:
        rc = lib.litho_abbe_accumulate_opts(*head, rec, ctypes.byref(opts), ctypes.byref(cnt))
    return rc, cnt.value


def call_in(nat, a, case, dev, stream=None, capacity=None, **kw):
    stream = stream or torch.cuda.current_stream(dev)
    torch.cuda.synchronize(dev)
    rc, cnt = launch(nat, case, {n: a.ptr(n) for n in a.bufs}, a.bufs["workspace"].nbytes, capacity or case.S, stream, **kw)
    try:
        torch.cuda.synchronize(dev)
    except RuntimeError as e:                                                  # a device fault: nothing more runs on this device
        pytest.exit(f"{case.name}: {e}", returncode=3)
    if rc == nat.E_HIP:
        pytest.exit(f"{case.name}: {nat.lib().litho_last_error().decode()}", returncode=3)
    return rc, cnt


def outside_an_arena(nat, case, pl, dev):
    """The same call on torch tensors and a torch.empty workspace of the same size: what the numerical tests pin."""
    mft, pupil, shifts, weights = inputs(case)
    t = {"maskFT": mft.to(dev), "pupil": pupil.to(dev), "shifts": shifts.to(dev), "weights": weights.to(dev),
         "out": prefill(case.planes, case.pn).to(dev), "workspace": torch.empty(pl.ws_bytes, dtype=torch.uint8, device=dev)}
    torch.cuda.synchronize(dev)
    rc, _ = launch(nat, case, {k: v.data_ptr() for k, v in t.items()}, pl.ws_bytes, case.S, torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0
    return t["out"]


def check_call(nat, a, case, pl, dev, planning=True, last_plan_kind=None, want_bits=None):
    """Assertions 1 - 6 on the arena after one call; returns `out` (a clone)."""
    ws, pn = a["workspace"], case.pn
    rep = a.report({})
    assert rep.clean, f"{case.name}: {rep}"                                                                          # 1
    out = a["out"].clone()
    assert bool(torch.isfinite(out).all()), case.name                                                               # 2
    if want_bits is not None:
        assert differing(out, want_bits) == [], f"{case.name}: bits differ from the reference call"
    elif pl.dry.run_size >= 2048:
        assert differing(out, outside_an_arena(nat, case, pl, dev)) == [], f"{case.name}: bits differ from the call outside an arena"
    else:
        got, ref = out.cpu().double() - a.sealed("out").cpu().double(), reference(case)
        e, l2 = rel_max(got, ref), rel_l2(got, ref)
        print(f"{case.name}: rel-to-max {e:.2e}, rel-L2 {l2:.2e}")
        assert e < TOL_IMAGE_MAX and l2 < TOL_IMAGE_L2, case.name
    if planning:                                                                                                    # 3
        assert ws[:56].view(torch.int32).cpu().tolist() == pl.words, (case.name, ws[:56].view(torch.int32).cpu().tolist(), pl.words)
    if pl.dry.split:
        assert ws[128:168].view(torch.int32).cpu().tolist() == pl.sw, (case.name, ws[128:168].view(torch.int32).cpu().tolist(), pl.sw)
    plan, last = nat.last_plan(), pl.last                                                                            # 4
    for dry_name, plan_name in DRY_FIELDS:
        assert getattr(last, dry_name) == plan[plan_name], (case.name, dry_name, getattr(last, dry_name), plan[plan_name], plan)
    if last.general:
        assert plan["box_rows"] == last.run_size and plan["box_row0"] == 0, (case.name, plan)
    else:
        assert plan["box_row0"] == pl.words[0] + (last.run_size - pn) // 2 and plan["box_rows"] == pl.words[1] - pl.words[0] + 1, (case.name, plan)
    if last_plan_kind is not None:
        assert plan["planned_from_record"] == last_plan_kind, (case.name, plan)
    ranges = pl.ranges(planning)                                                                                     # 5
    touched = a.touched_outside("workspace", ranges.values())
    assert touched == [], f"{case.name}: {len(touched)} bytes outside the declared ranges, first {touched[:4]}, last {touched[-1]}; declared {ranges}"
    head = {}                                                                                                       # 6
    for i, p in enumerate(pl.parts):
        written = min(p.planes_in_flight, case.planes) * min(p.batch, p.source_points) * p.t_item_bytes
        assert written <= p.T_used.bytes
        head[p.T_used.offset] = max(head.get(p.T_used.offset, 0), written, p.recon_T_used.bytes)
    tight = dict(ranges)
    for i, p in enumerate(pl.parts):
        tight[f"T_used[{i}]"] = (p.T_used.offset, head[p.T_used.offset])
        tight.pop(f"recon_T_used[{i}]", None)
    touched = a.touched_outside("workspace", tight.values())
    assert touched == [], f"{case.name}: {len(touched)} bytes of T behind the last item written, first {touched[:4]}"
    KERNELS[case.name] = nat.last_kernels()
    assert KERNELS[case.name] == (case.expect["xk"], case.expect["yk"]), (case.name, KERNELS[case.name])                # 10
    return out


def run(nat, case, dev, cus, side=None, arenas=None):
    """One case: aligned arena (two calls), the other alignment, the side stream.  `arenas`: {odd: arena} to reuse (the 4096 group)."""
    t0 = time.perf_counter()
    pl = Planned(nat, case, cus)
    capacity = case.S + 3 if case.entry in ("counted", "planned") else case.S
    bits = {}
    for odd in (False, True):
        if arenas is not None and odd in arenas:
            a = arenas[odd]
            b = a.bufs["workspace"]
            a.bytes[b.start:b.end].fill_(POISON)
            a.fill("out", a.sealed("out"))
        else:
            a = make_arena(case, pl, dev, odd, capacity, weights=arenas is not None)
            if arenas is not None:
                arenas[odd] = a
        rc, cnt = call_in(nat, a, case, dev, capacity=capacity)
        assert rc == 0 and cnt == case.S, (case.name, rc, cnt, nat.lib().litho_last_error())
        bits[odd] = check_call(nat, a, case, pl, dev, want_bits=bits.get(False))
        if capacity > case.S:                                                  # the tail of the list is poison and stays out of it
            assert bool((a["shifts"][case.S:] == -1).all())
        if odd:
            continue
        a.fill("out", a.sealed("out"))                                                                               # 7
        rc, cnt = call_in(nat, a, case, dev, capacity=capacity)
        assert rc == 0 and a.report({}).clean and differing(a["out"], bits[False]) == [], f"{case.name}: second call into the used arena"
        if case.side:                                                                                               # 9
            a.fill("out", a.sealed("out"))
            rc, cnt = call_in(nat, a, case, dev, stream=side, capacity=capacity)
            assert rc == 0 and a.report({}).clean and differing(a["out"], bits[False]) == [], f"{case.name}: side stream"
    TIMES[case.name] = time.perf_counter() - t0
    return pl, bits[False]


@gpu
@pytest.mark.parametrize("name", [c.name for c in CASES if c.entry == "opts"])
def test_abbe_call_stays_inside_what_the_dry_run_declares(nat, dev, cus, side, name):
    run(nat, BY_NAME[name], dev, cus, side)


@gpu
def test_the_4096_group_in_one_arena(nat, dev, cus, side):
    """k_ypass_coop_dma, k_ypass_coop (tile 16), k_xpass_split<13> + k_ypass_pair<13> and the weighted k_xpass_split<13, float
    const*>: the four calls in turn in ONE 5 GiB arena per alignment (with a weights buffer from the start, for the last of
    them), the workspace re-poisoned and `out` re-filled between them."""
    arenas = {}
    for case in BIG:
        run(nat, case, dev, cus, side, arenas)
    print("4096 group: " + ", ".join(f"{c.name} {TIMES[c.name]:.1f} s" for c in BIG))


@gpu
@pytest.mark.parametrize("name", [c.name for c in CASES if c.entry == "weighted"])
def test_weighted_entry(nat, dev, cus, side, name):
    """Weights inside the arena (one of them 0); w = 1 gives the unweighted call's bits."""
    case = BY_NAME[name]
    pl, _ = run(nat, case, dev, cus, side)
    a = make_arena(case, pl, dev)
    a["weights"].fill_(1.0)
    a.seal()
    rc, _ = call_in(nat, a, case, dev)
    plain = Case(case.name, case.pn, case.N, case.opts, S=case.S, planes=case.planes, pupil=case.pupil, src=case.src)
    b = make_arena(plain, pl, dev)
    rc2, _ = call_in(nat, b, plain, dev)
    assert rc == 0 and rc2 == 0 and a.report({}).clean and b.report({}).clean and differing(a["out"], b["out"]) == [], name


@gpu
@pytest.mark.parametrize("name", [c.name for c in CASES if c.entry == "counted"])
def test_counted_entry(nat, dev, cus, side, name):
    """count_dev inside the arena, capacity = S + 3: the count comes back, the poisoned tail of the list influences nothing
    (the extents among the plan words are those of the first S entries: assertion 3)."""
    run(nat, BY_NAME[name], dev, cus, side)


@gpu
@pytest.mark.parametrize("name", [c.name for c in CASES if c.entry == "planned"])
def test_planned_entry(nat, dev, cus, side, name):
    """A call planned from a filled record: the planning call's bits, the same bytes untouched -- and not even the planning
    scratch or the plan words, which it does not compute again (litho_abbe_last_plan [15] = 1, a split list 3)."""
    case = BY_NAME[name]
    pl, bits = run(nat, case, dev, cus, side)
    capacity = case.S + 3
    a = make_arena(case, pl, dev, capacity=capacity)
    rec = nat.PlanRecord()
    rc, cnt = call_in(nat, a, case, dev, capacity=capacity, record=rec)
    assert rc == 0 and rec.valid == 1 and differing(a["out"], bits) == [] and nat.last_plan()["planned_from_record"] == (2 if pl.dry.split else 0)
    b = a.bufs["workspace"]
    a.bytes[b.start:b.end].fill_(POISON)
    a.fill("out", a.sealed("out"))
    rc, cnt = call_in(nat, a, case, dev, capacity=capacity, record=rec)
    assert rc == 0 and cnt == case.S, (rc, cnt)
    check_call(nat, a, case, pl, dev, planning=False, last_plan_kind=3 if pl.dry.split else 1, want_bits=bits)
    assert bool((a["workspace"][:56] == POISON).all()), "a call planned from a record writes no plan words"


@gpu
def test_every_kernel_family_was_launched(nat):
    """Over the file, every x-pass and y-pass family DESIGN.md section 4 names ran at least once (the table under -s)."""
    names = [c.name for c in CASES + BIG]
    assert [n for n in names if n not in KERNELS] == [], "run the whole file: the cases above fill the table"
    for n in names:
        print(f"{n:30s} {KERNELS[n][0]:44s} {KERNELS[n][1]:34s} {TIMES.get(n, 0):5.1f} s")
    fam = lambda k: k.split("<")[0]
    xs, ys = {fam(KERNELS[n][0]) for n in names}, {fam(KERNELS[n][1]) for n in names}
    assert set(X_FAMILIES) <= xs and set(Y_FAMILIES) <= ys, (sorted(xs), sorted(ys))
    assert "k_ypass_coop" in ys                                                # (coopdma 0: not in section 4's table, run all the same)
    print(f"{len(names)} cases, {sum(TIMES.values()):.1f} s; slowest {max(TIMES, key=TIMES.get)} {max(TIMES.values()):.1f} s")


# ---- refusals: nothing is launched -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("what", ["workspace one byte short", "null maskFT", "null out", "N below pn"])
def test_refused_calls_touch_nothing(nat, dev, cus, what):
    case = Case("refused", 64, 32, S=4) if what == "N below pn" else BY_NAME["64-128"]
    if what == "N below pn":
        pl, ws_bytes = None, 4096
    else:
        pl = Planned(nat, case, cus)
        ws_bytes = pl.own_bytes - 1 if what == "workspace one byte short" else pl.ws_bytes
    a = make_arena(case, pl, dev, ws_bytes=ws_bytes)
    ptrs = {n: a.ptr(n) for n in a.bufs}
    if what.startswith("null"):
        ptrs[what.split()[1]] = 0
    torch.cuda.synchronize(dev)
    rc, _ = launch(nat, case, ptrs, ws_bytes, case.S, torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)
    assert rc == {"workspace one byte short": nat.E_WORKSPACE, "N below pn": nat.E_NSMALL}.get(what, nat.E_ARG), (what, rc)
    assert a.report({}).clean and a.still_poison("workspace") and differing(a["out"], a.sealed("out")) == [], what


# ---- the harness can fail --------------------------------------------------------------------------------------------------------
@gpu
def test_planted_writes_are_reported_where_they_are(nat, dev, cus):
    """After one correct call: one fp32 just behind T_used, one int32 in front of the workspace, by plain torch assignments."""
    case = BY_NAME["256 small ragged xchunk"]
    pl = Planned(nat, case, cus)
    a = make_arena(case, pl, dev)
    rc, _ = call_in(nat, a, case, dev)
    ranges = list(pl.ranges().values())
    assert rc == 0 and a.report({}).clean and a.touched_outside("workspace", ranges) == []
    end = pl.last.T_used.end
    assert end + 4 <= pl.ws_bytes and all(not (o <= end < o + n) for o, n in ranges)
    a["workspace"][end:end + 4].view(torch.float32)[0] = 1.0
    assert a.touched_outside("workspace", ranges) == [end, end + 1, end + 2, end + 3]      # 1.0f = 00 00 80 3F: no byte of it is 0xFF
    b = a.bufs["workspace"]
    a.bytes[b.start - 4:b.start].view(torch.int32)[0] = 0
    assert a.report({}).guards == [("workspace", -4), ("workspace", -3), ("workspace", -2), ("workspace", -1)]


@gpu
@pytest.mark.parametrize("name, region", [("256 small ragged xchunk", "T_used[0]"), ("256 small fold", "slab_used[0]"), ("256 small fold", "ic_used[0]"),
                                          ("200 embedded", "embed_O[0]"), ("256 split", "list_b"),
                                          # the two regions the dry run did not declare before this file existed
                                          ("200 embedded", "plan_scratch"), ("256 default", "twtab2[0]")])
def test_a_declared_range_one_block_short_is_noticed(nat, dev, cus, name, region):
    """Assertion 5 can fail: the same ranges with ONE of them shortened by its last 256-byte block (in this test's copy, not in
    the library) no longer cover what the call wrote."""
    case = BY_NAME[name]
    pl = Planned(nat, case, cus)
    a = make_arena(case, pl, dev)
    rc, _ = call_in(nat, a, case, dev)
    ranges = pl.ranges()
    assert rc == 0 and a.touched_outside("workspace", ranges.values()) == []
    off, n = ranges[region]
    ranges[region] = (off, n - 256)
    touched = a.touched_outside("workspace", ranges.values())
    assert touched and off + n - 256 <= touched[0] and touched[-1] < off + n, (region, touched[:4])


# ---- the workspace entries without a dry run: litho_abbe_field, litho_mask_spectrum, litho_mask_spectrum_complex ------------------
# What each may touch, read off abbe_engine.hip (abbe_field, mask_setup, mask_spectrum*), at the offsets of the own-size layout
# (a dry run of the same (pn, N) with the embedding off):
#   field     plan ints [0, 15) (the planning words and the weight flag) and [16, 18) (the (0, 0) shift); the table; the head of T:
#             the planning scratch, then ONE item of the pupil's box in 4-column tiles, ceil(pn / 4) 4 rows float2
#   spectra   the table; the scaled image in the slab region, 4 ns^2 (int16 entry) or 8 ns^2 bytes; ONE item of T,
#             ceil(pn / 4) 4 (j1 - j0) float2, [j0, j1) the frame samples that hold image samples
SMALL_SIZES = [(16, 32), (64, 128), (200, 512), (256, 512), (512, 1024)]
EPS_PADS, EPS_CROPS = 1.0363, 1.035                                            # epsilon, and epsilon pn / N: ns < N padded, ns > N cropped


def own_layout(nat, pn, N):
    d = nat.plan_dry_run(pn, N, 1, [0, pn - 1, 0, pn - 1, 0, 0, 0, 0, 1] + [INT_MAX, INT_MIN] * 2 + [0], options={"embed": 0})
    size = ctypes.c_size_t(0)
    assert d.status == 0 and nat.lib().litho_abbe_workspace_bytes(pn, N, ctypes.byref(size)) == 0
    return d.part[0], size.value


def transform_call(nat, dev, side, entry, pn, N, eps=None):
    import spectrum_oracle as SO
    lay, ws_bytes = own_layout(nat, pn, N)
    if eps == EPS_CROPS:
        eps = EPS_CROPS * N / pn
    lib, seed = nat.lib(), SO.case_seed(pn, N, 7)
    tile_cols = (pn + 3) // 4 * 4
    if entry == "field":
        P, M = torch.from_numpy(disk_pupil(pn, 1)), SO.complex_gaussian(pn, seed)
        ins = {"pf": P, "maskFT": M}
        ref, norm = SO.field_f64(P.to(SO.C128) * M.to(SO.C128), pn, N), SO.fro((P, M))
        rows = int((P != 0).any(1).sum())
        ranges = [(lay.plan.offset, 60), (lay.plan.offset + 64, 8), (lay.twtab.offset, N * 8),
                  (lay.T_region.offset, max(((pn + 7) // 8 + 1) * 64, tile_cols * rows * 8))]
        fn = lambda a, st: lib.litho_abbe_field(a.ptr("pf"), a.ptr("maskFT"), pn, N, a.ptr("result"), a.ptr("workspace"), ws_bytes, st)
    else:
        x = SO.pm1_mask(pn, seed) if entry == "int16" else SO.complex_map(pn, seed)
        ins = {"mask": x}
        scaled = SO.scaled_image(x, eps)
        ns = scaled.shape[0]
        pW, j0, j1 = SO.frame_window(ns, N)
        assert (ns < N) == (eps == EPS_PADS) and ns != N and j1 - j0 == min(ns, N)
        ref, norm = SO.spectrum_f64(scaled, pn, N), SO.fro(scaled)
        ranges = [(lay.twtab.offset, N * 8), (lay.slab_region.offset, ns * ns * (4 if entry == "int16" else 8)),
                  (lay.T_region.offset, tile_cols * (j1 - j0) * 8)]
        f = lib.litho_mask_spectrum if entry == "int16" else lib.litho_mask_spectrum_complex
        fn = lambda a, st: f(a.ptr("mask"), pn, eps, N, a.ptr("result"), a.ptr("workspace"), ws_bytes, st)
    bits = {}
    for odd in (False, True):
        bufs = [Buf(k, "in", v.dtype, v.shape, (8 if v.is_complex() else 4) if odd else 0) for k, v in ins.items()]
        bufs += [Buf("result", "out", torch.complex64, (pn, pn), 8 if odd else 0), Buf("workspace", "work", torch.uint8, (ws_bytes,))]
        a = Arena(bufs, (pn * pn + pn + 4) * 8, device=dev)
        for k, v in ins.items():
            a.fill(k, v.to(dev))
        a.seal()
        want = {"result": ref.to(torch.complex64)}
        for stream in [torch.cuda.current_stream(dev)] * 2 + ([side] if not odd else []):       # 7: the second call into the used arena
            torch.cuda.synchronize(dev)
            rc = fn(a, ctypes.c_void_p(stream.cuda_stream))
            torch.cuda.synchronize(dev)
            rep = a.report(want)
            assert rc == 0 and rep.clean, f"{entry} {pn} {N} {eps}: rc {rc}, {rep}"                                      # 1
            got = a["result"].clone()
            assert differing(got, bits.setdefault("first", got)) == [], f"{entry} {pn} {N} {eps}: bits differ (odd {odd}, {stream})"   # 7, 8
        err = SO.err_norm(got.cpu(), ref, norm)                                                                         # 2
        if not odd:
            print(f"{entry} pn {pn} N {N} eps {eps}: err_norm {err:.3e}, bound {SO.bound(N):.3e}")
        assert err <= SO.bound(N) and bool(torch.isfinite(torch.view_as_real(got)).all())
        touched = a.touched_outside("workspace", ranges)                                                                 # 5
        assert touched == [], f"{entry} {pn} {N} {eps}: {len(touched)} bytes outside {ranges}: first {touched[:4]}, last {touched[-1]}"


@gpu
@pytest.mark.parametrize("pn, N", SMALL_SIZES)
def test_field_entry(nat, dev, side, pn, N):
    transform_call(nat, dev, side, "field", pn, N)


@gpu
@pytest.mark.parametrize("eps", [EPS_PADS, EPS_CROPS])
@pytest.mark.parametrize("entry", ["int16", "complex"])
@pytest.mark.parametrize("pn, N", SMALL_SIZES)
def test_mask_spectrum_entries(nat, dev, side, pn, N, entry, eps):
    transform_call(nat, dev, side, entry, pn, N, eps)


# ---- litho_source_compact / _weighted: scratch of exactly pn + 1 int32, lists of exactly `capacity` entries -----------------------
@gpu
@pytest.mark.parametrize("sync", [True, False])
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("pn", [16, 30, 256])
def test_source_compact_entries(nat, dev, side, pn, weighted, extra, sync):
    """Shifts and weights bit for bit (row-major order), the entries beyond S still poison, scratch = the raw row counts and the
    total in scratch[pn] (the two-launch form used up to pn 4096 leaves the counts raw)."""
    lib = nat.lib()
    pts = annulus_points(pn, None)
    S, cap = len(pts), len(pts) + extra
    src = torch.zeros(pn, pn, dtype=torch.float32 if weighted else torch.int64)
    vals = 0.25 + (torch.arange(S) % 7).to(torch.float32) / 8.0
    at = torch.from_numpy(pts.astype(np.int64)) + pn // 2
    src[at[:, 0], at[:, 1]] = vals if weighted else 1
    want = {"shifts": torch.full((cap, 2), -1, dtype=torch.int32), "scratch": torch.cat([src.ne(0).sum(1), torch.tensor([S])]).to(torch.int32)}
    want["shifts"][:S] = torch.from_numpy(pts)
    if weighted:
        want["weights"] = torch.full((cap,), -1, dtype=torch.int32).view(torch.float32)
        want["weights"][:S] = vals
    for odd in (False, True):
        bufs = [Buf("src", "in", src.dtype, (pn, pn), (8 if src.dtype == torch.int64 else 4) if odd else 0),
                Buf("shifts", "out", torch.int32, (cap, 2), 4 if odd else 0), Buf("scratch", "out", torch.int32, (pn + 1,), 4 if odd else 0)]
        if weighted:
            bufs.append(Buf("weights", "out", torch.float32, (cap,), 4 if odd else 0))
        a = Arena(bufs, (pn * pn + pn + 4) * 8, device=dev)
        a.fill("src", src.to(dev))
        a.seal()
        for stream in [torch.cuda.current_stream(dev)] * 2 + [side]:
            cnt = ctypes.c_int64(-7)
            host = ctypes.byref(cnt) if sync else None
            torch.cuda.synchronize(dev)
            if weighted:
                rc = lib.litho_source_compact_weighted(a.ptr("src"), pn, a.ptr("shifts"), a.ptr("weights"), cap, a.ptr("scratch"), host,
                                                       ctypes.c_void_p(stream.cuda_stream))
            else:
                rc = lib.litho_source_compact(a.ptr("src"), pn, a.ptr("shifts"), cap, a.ptr("scratch"), host, ctypes.c_void_p(stream.cuda_stream))
            torch.cuda.synchronize(dev)
            rep = a.report(want)
            assert rc == 0 and cnt.value == (S if sync else -7) and rep.clean, (rc, cnt.value, str(rep))
            for k, v in want.items():
                assert differing(a[k], v) == [], (k, pn, weighted, extra, sync, odd)
