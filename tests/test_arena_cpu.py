"""tests/arena.py can fail: the layout it promises and every kind of damage it is there to report, on CPU tensors (no GPU)."""
import pytest
import torch

from arena import POISON, Arena, Buf, differing, words

N, D = 5, 2
GUARD = (N * N + N + 4) * 4                                                    # one plane + one row + one pack, in bytes: 136


def make(mod_x=0, mod_y=0, mod_w=0, work_bytes=100):
    a = Arena([Buf("x", "in", torch.float32, (D, N, N), mod_x), Buf("y", "out", torch.float32, (D, N, N), mod_y),
               Buf("work", "work", torch.uint8, (work_bytes,), mod_w)], GUARD)
    x = torch.arange(D * N * N, dtype=torch.float32).reshape(D, N, N) + 1.0
    a.fill("x", x)
    a.seal()
    return a, x


def answer(a, x):
    """What a correct call would do: y = 2 x, and scribble over all of the workspace."""
    a["y"].copy_(2.0 * x)
    a["work"].fill_(0x11)
    return {"y": 2.0 * x}


@pytest.mark.parametrize("mod", [0, 4, 8, 12])
def test_offsets_and_guard_sizes(mod):
    a, x = make(mod_x=mod, mod_y=(mod + 4) % 16, mod_w=mod)
    assert a.guard == 256 and a.guard >= GUARD                                  # 136 bytes rounded up to 256
    assert a.bytes.data_ptr() % 256 == 0 and bool((a.bytes[:a.bufs["x"].start] == POISON).all())
    for name, m in (("x", mod), ("y", (mod + 4) % 16), ("work", mod)):
        b = a.bufs[name]
        assert a.ptr(name) % 16 == m and a.ptr(name) == a.bytes.data_ptr() + b.start
        assert b.end - b.start == b.nbytes == a[name].numel() * a[name].element_size()
        assert a.leading_guard(name) >= a.guard and a.trailing_guard(name) >= a.guard
    assert a.bufs["x"].end <= a.bufs["y"].start - a.guard and a.size - a.bufs["work"].end >= a.guard
    assert torch.equal(a["x"], x) and a.still_poison("y") and a.still_poison("work")
    assert words(a["y"]).dtype == torch.int32 and bool((words(a["y"]) == -1).all()) and bool(torch.isnan(a["y"]).all())
    rep = a.report(answer(a, x))
    assert rep.clean and not a.still_poison("y"), str(rep)


def test_a_complex_buffer_at_8_mod_16():
    a = Arena([Buf("p", "in", torch.complex64, (3, 4), 8), Buf("q", "out", torch.complex64, (3, 4), 8)], 64)
    assert a.ptr("p") % 16 == 8 and a.ptr("q") % 16 == 8 and a["q"].dtype == torch.complex64
    assert bool(torch.isnan(torch.view_as_real(a["q"])).all())
    p = torch.complex(torch.arange(12.0).reshape(3, 4), torch.ones(3, 4))
    a.fill("p", p)
    a.seal()
    a["q"].copy_(p)
    a["q"].view(torch.float32).reshape(-1)[5] = float("nan")                    # one real part written as an ordinary NaN
    a["q"].view(torch.int32).reshape(-1)[7] = -1                                # one imaginary part left as poison
    want = p.clone()
    torch.view_as_real(want).reshape(-1)[5] = float("nan")
    rep = a.report({"q": want})
    assert rep.unwritten == [("q", 28)] and not rep.guards and not rep.inputs, str(rep)


@pytest.mark.parametrize("mod", [0, 12])
def test_a_flipped_byte_is_reported_where_it_is(mod):
    a, x = make(mod_x=mod, mod_y=mod)
    want = answer(a, x)
    y, w = a.bufs["y"], a.bufs["work"]
    a.bytes[y.start - 1] = 0                                                   # the last byte in front of y
    a.bytes[y.end] = 7                                                         # the first byte behind y
    a.bytes[w.start - 100] = 1                                                 # inside the guard in front of the workspace
    a.bytes[a.size - 1] = 2                                                    # the last byte of the arena
    a.bytes[a.bufs["x"].start + 9] ^= 0x40                                     # an input byte
    rep = a.report(want)
    assert rep.guards == [("y", -1), ("y", y.nbytes), ("work", -100), ("work", a.size - 1 - w.start)], str(rep)
    assert rep.inputs == [("x", 9)] and rep.unwritten == [] and not rep.clean


def test_a_byte_in_front_of_the_first_buffer():
    a, x = make()
    want = answer(a, x)
    a.bytes[0] = 0
    assert a.report(want).guards == [("x", -a.guard)]


def test_an_output_element_left_as_poison_is_reported_and_a_nan_result_is_not():
    a, x = make(mod_y=4)
    want = answer(a, x)
    nan_other_payload = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)[0]
    want["y"][1, 2, 3] = float("nan")                                          # the reference: the canonical NaN, 0x7fc00000
    a["y"][1, 2, 3] = nan_other_payload                                        # the call: a NaN of another payload -- written
    a["y"].view(torch.int32)[0, 4, 1] = -1                                     # never written: still 0xFFFFFFFF
    rep = a.report(want)
    assert rep.unwritten == [("y", 4 * (4 * N + 1))] and not rep.guards and not rep.inputs, str(rep)
    # as floats the two could not be told apart: both are NaN, and neither equals the reference
    assert bool(torch.isnan(a["y"][1, 2, 3])) and bool(torch.isnan(a["y"][0, 4, 1]))
    # bitwise comparison sees both, and only those
    assert differing(a["y"], want["y"]) == [4 * (4 * N + 1), 4 * (N * N + 2 * N + 3)]
    want["y"][1, 2, 3] = nan_other_payload
    assert differing(a["y"], want["y"]) == [4 * (4 * N + 1)]
    # where the reference itself holds the poison pattern, an equal word is no finding
    want["y"].view(torch.int32)[0, 4, 1] = -1
    assert a.report(want).clean and differing(a["y"], want["y"]) == []


@pytest.mark.parametrize("nbytes", [1, 100, 256, 4 * 50 + 256])
def test_a_workspace_of_exact_size(nbytes):
    a, x = make(work_bytes=nbytes)
    w = a.bufs["work"]
    assert a["work"].numel() == nbytes and w.end - w.start == nbytes and a["work"].dtype == torch.uint8
    want = answer(a, x)                                                        # writes every byte of the workspace
    assert a.report(want).clean
    a.bytes[w.end] = 0x11                                                      # one byte more than was asked for
    assert a.report(want).guards == [("work", nbytes)]


WIDTHS = {"int16 of odd length": (torch.int16, (7, 7), 4), "int64": (torch.int64, (9,), 8), "float64": (torch.float64, (5, 4), 8)}


@pytest.mark.parametrize("kind", list(WIDTHS))
def test_elements_of_two_and_eight_bytes(kind):
    """The dtypes of the geometry family: int16 [pn, pn] with odd pn (98 bytes: no multiple of 4), int64 counts, float64 edges.
    A flipped guard byte, a changed input and an unwritten element are each reported at their byte offset, the last element of
    the odd-length buffer included; the poison is all-ones at every width."""
    dtype, shape, mod = WIDTHS[kind]
    size = torch.empty((), dtype=dtype).element_size()
    count = int(torch.tensor(shape).prod())
    a = Arena([Buf("x", "in", dtype, shape, mod), Buf("y", "out", dtype, shape, mod), Buf("tail", "out", torch.int16, (3,), 4)], 64)
    assert a.ptr("x") % 16 == mod and a.ptr("y") % 16 == mod and a.bufs["y"].nbytes == count * size and a.bufs["tail"].nbytes == 6
    assert (count * size) % 4 == (2 if dtype == torch.int16 else 0)
    x = (torch.arange(count, dtype=torch.float64).reshape(shape) * 3.0 + 1.0).to(dtype)
    a.fill("x", x)
    a.seal()
    assert words(a["y"]).dtype == {2: torch.int16, 8: torch.int64}[size] and bool((words(a["y"]) == -1).all())
    assert bool(torch.isnan(a["y"]).all()) if dtype.is_floating_point else bool((a["y"] == -1).all())
    want = {"y": x + x, "tail": torch.tensor([1, 0, 1], dtype=torch.int16)}
    assert a.report(want).unwritten == [("y", size * i) for i in range(count)] + [("tail", 2 * i) for i in range(3)]
    a["y"].copy_(want["y"])
    a["tail"].copy_(want["tail"])
    assert a.report(want).clean and differing(a["y"], want["y"]) == [] and differing(a["tail"], want["tail"]) == []
    y = a.bufs["y"]
    a.bytes[y.end] = 0                                                         # the first byte behind y: for int16 [7, 7] at byte 98
    a.bytes[y.start - 3] ^= 0x01                                               # in front of it
    a.bytes[a.bufs["x"].start + size * (count - 1) + size - 1] ^= 0x80        # the last byte of the last input element
    a["y"].view(-1).view({2: torch.int16, 8: torch.int64}[size])[count - 1] = -1     # the last element left as poison
    a["tail"][2] = -1                                                          # and the odd one behind a 4-byte boundary
    rep = a.report(want)
    assert rep.guards == [("y", -3), ("y", y.nbytes)] and rep.inputs == [("x", size * count - 1)], str(rep)
    assert rep.unwritten == [("y", size * (count - 1)), ("tail", 4)] and not rep.clean, str(rep)
    assert differing(a["y"], want["y"]) == [size * (count - 1)] and differing(a["tail"], want["tail"]) == [4]
    # half of an 8-byte element still poison is a written element (its bits differ from the reference, which differing() reports)
    if size == 8:
        a["y"].view(-1).view(torch.int32)[0] = -1
        assert a.report(want).unwritten == [("y", size * (count - 1)), ("tail", 4)] and differing(a["y"], want["y"])[0] == 0
    # where the reference itself is all-ones, an equal element is no finding
    want["tail"][2] = -1
    assert a.report(want).unwritten == [("y", size * (count - 1))]


def test_an_eight_byte_element_starts_at_0_or_8():
    with pytest.raises(AssertionError):
        Buf("e", "in", torch.float64, (4,), 4)
    with pytest.raises(AssertionError):
        Buf("c", "out", torch.int64, (4,), 12)
    assert Buf("g", "out", torch.int16, (3,), 12).nbytes == 6


def test_nothing_launched_leaves_everything_poison():
    a, x = make(mod_w=8)
    assert a.ptr("work") % 16 == 8
    assert a.still_poison("y") and a.still_poison("work") and a.report({"y": 2.0 * x}).unwritten[0] == ("y", 0)
    a["work"][3] = 0
    assert not a.still_poison("work")


# ---- a workspace whose call declares which bytes it may use -----------------------------------------------------------------------
RANGES = [(256, 512), (1024, 256)]                                             # [256, 768) and [1024, 1280) of a 2000-byte workspace


def declared(work_bytes=2000):
    a, x = make(work_bytes=work_bytes)
    w = a["work"]
    for off, n in RANGES:                                                      # a correct call: writes inside its ranges only
        w[off:off + n] = 0x11
    return a, x


def test_touched_outside_a_clean_case():
    a, x = declared()
    assert a.touched_outside("work", RANGES) == [] and a.touched_outside("work", list(reversed(RANGES))) == []
    assert a.touched_outside("work", RANGES + [(0, 0)]) == []                 # an absent region (0 bytes) declares nothing
    assert a.touched_outside("work", [RANGES[0]]) == list(range(1024, 1280))   # the harness can fail: a range withheld
    assert a.touched_outside("work", [(256, 511), RANGES[1]]) == [767]         # ... or shortened by one byte


@pytest.mark.parametrize("where, at", [("just before a range", 255), ("just after a range", 768), ("between two ranges", 900),
                                       ("just before the second range", 1023), ("just after the last range", 1280),
                                       ("the first byte", 0), ("the last byte", 1999)])
def test_touched_outside_one_planted_byte(where, at):
    a, x = declared()
    a["work"][at] = 0
    assert a.touched_outside("work", RANGES) == [at], where
    a["work"][at] = POISON                                                     # the poison value itself written there: not seen, by design
    assert a.touched_outside("work", RANGES) == []


def test_touched_outside_overlapping_ranges_and_a_whole_buffer():
    a, x = declared()
    a["work"][700:1100] = 0x22
    assert a.touched_outside("work", [(256, 512), (600, 500), (1024, 256)]) == []
    assert a.touched_outside("work", [(0, 2000)]) == [] and a.touched_outside("work", []) == list(range(256, 1280))
    with pytest.raises(AssertionError):
        a.touched_outside("work", [(1900, 101)])                               # a range that leaves the buffer
    with pytest.raises(AssertionError):
        a.touched_outside("x", RANGES)                                         # only a workspace has declared ranges


def test_an_accumulated_buffer_is_guarded_and_sealed_but_left_to_the_caller():
    """Role "inout": the prefill is kept by seal(), a change of the buffer is neither "input changed" nor "never written" --
    whether it was written at all is for the caller to see by comparing values -- and its guards are watched like any other."""
    a = Arena([Buf("x", "in", torch.float32, (4,)), Buf("acc", "inout", torch.float32, (3, 3), 8), Buf("w", "work", torch.uint8, (64,))], 64)
    pre = torch.arange(9, dtype=torch.float32).reshape(3, 3) * 0.5 + 1.0
    a.fill("x", torch.ones(4))
    a.fill("acc", pre)
    a.seal()
    assert a.ptr("acc") % 16 == 8 and a.leading_guard("acc") >= 64 and a.trailing_guard("acc") >= 64
    assert a.report({}).clean and torch.equal(a.sealed("acc"), pre) and torch.equal(a.sealed("x"), torch.ones(4))
    a["acc"].add_(2.0)                                                         # the call accumulates: no finding
    a["acc"].view(torch.int32)[1, 1] = -1                                      # even an element that IS the poison pattern is the caller's
    rep = a.report({})
    assert rep.clean, str(rep)
    assert torch.equal(a.sealed("acc"), pre) and differing(a["acc"], pre + 2.0) == [16]
    b = a.bufs["acc"]
    a.bytes[b.end] = 0
    a.bytes[b.start - 1] = 0
    a["x"][2] = 5.0
    rep = a.report({})
    assert rep.guards == [("acc", -1), ("acc", b.nbytes)] and [n for n, _ in rep.inputs] == ["x"] * len(rep.inputs) and rep.inputs
    assert all(8 <= off < 12 for _, off in rep.inputs) and not rep.unwritten


def test_comparisons_in_chunks(monkeypatch):
    """The scans walk the arena CHUNK bytes at a time: findings on both sides of a chunk border, reported once each."""
    import arena
    monkeypatch.setattr(arena, "CHUNK", 100)
    a, x = declared()
    for at in (99, 100, 199, 900, 1999):
        a["work"][at] = 3
    assert a.touched_outside("work", RANGES) == [99, 100, 199, 900, 1999]
    assert not a.still_poison("work") and a.still_poison("y")
    a.bytes[a.size - 1] = 0
    assert a.report({"y": 2.0 * x}).guards == [("work", a.size - 1 - a.bufs["work"].start)]
