"""A guarded, poisoned arena for calls through the raw C ABI: every device buffer of ONE call -- inputs, outputs and the
workspace -- lies in a single uint8 allocation, so that what a kernel reads or writes outside a buffer is seen.

    poison      every byte of the arena is 0xFF before the inputs are copied in: as fp32 or complex64 that is a NaN (a read outside
                a buffer contaminates the result instead of looking plausible), as int32 it is -1 (a flag word that nobody
                initialised reads as "changed").
    guards      in front of and behind every buffer lie at least `guard_bytes` bytes of poison, rounded up to 256: the caller
                passes one plane + one row + one pack of the call's volume, (n n + n + 4) elements, the farthest a one-off error in
                a plane, row or pack index can reach.
    alignment   a buffer starts `mod` bytes (0, 4, 8 or 12) past a 16-byte boundary; the arena asserts data_ptr() % 16 == mod.
    exact sizes a buffer is exactly as long as it was asked for -- a workspace exactly what its *_work_bytes function returned --
                and the next byte is guard.

After the call `report(reference)` lists, as (buffer name, byte offset from the start of that buffer): every guard byte that
changed (a negative offset lies in front of the buffer, one >= its size behind it; a byte between two buffers goes to the nearer
one), every input byte that changed, and every 4-byte word of an output that still holds the poison pattern where the reference
result does not.  All comparisons are of bit patterns, through uint8 or int32 views: a result may hold NaN (walls) and a NaN
never equals itself as a float.  A buffer that is accumulated into has the role "inout": filled, sealed and guarded, but left
to the caller to compare (sealed(name) is what it held).  For a workspace whose call declares WHICH bytes it may use,
touched_outside(name, ranges) lists the bytes outside those ranges that no longer hold the poison.  Every comparison runs on the
arena's own device, in runs of at most CHUNK bytes.  Works on CPU tensors as well (tests/test_arena_cpu.py)."""
import torch

POISON = 0xFF
POISON_WORD = -1                                                               # all-ones as int16, int32 or int64
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}       # the integer view of an element, by its width
ROLES = ("in", "out", "work", "inout")
CHUNK = 1 << 28                                                                # bytes compared at a time: a workspace may be 5 GiB


class Buf:
    """One buffer of the call: `role` "in" (must not change), "out" (must be written completely), "work" (scratch: its
    contents are nobody's business, its borders are) or "inout" (accumulated into: filled, sealed and guarded like an input, but
    exempt from the input-unchanged and the never-written scans -- the caller compares its values); `mod` = the start offset in bytes modulo 16, a multiple of the element
    size (an 8-byte element starts at 0 or 8)."""

    def __init__(self, name, role, dtype, shape, mod=0):
        assert role in ROLES and mod in (0, 4, 8, 12), (name, role, mod)
        self.name, self.role, self.dtype, self.shape, self.mod = name, role, dtype, tuple(int(v) for v in shape), mod
        count = 1
        for v in self.shape:
            count *= v
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.nbytes = count * self.itemsize
        assert self.nbytes > 0 and mod % min(self.itemsize, 16) == 0, (name, self.nbytes, dtype, mod)
        self.start = self.end = None


def words(t):
    """The bit patterns of a tensor, element by element, as a flat integer tensor of the element's width: uint8 (1 byte), int16
    (int16), int32 (fp32, int32; complex64 as its real parts) or int64 (fp64, int64; complex128 as its real parts)."""
    t = t.contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    t = t.reshape(-1)
    bits = _BITS[t.element_size()]
    return t if t.dtype == bits else t.view(bits)


def poison_of(w):
    """The poison pattern as an element of words()' dtype: 0xFF for bytes, -1 (all-ones) for the signed widths."""
    return POISON if w.dtype == torch.uint8 else POISON_WORD


def differing(a, b):
    """Byte offsets of the elements (of a's own width) in which a and b differ as bit patterns; a shape mismatch is an error."""
    wa, wb = words(a), words(b.to(a.device))
    assert wa.shape == wb.shape and wa.dtype == wb.dtype, (tuple(a.shape), tuple(b.shape))
    step = wa.element_size()
    return [step * i for i in (wa != wb).nonzero().flatten().cpu().tolist()]


class Report:
    """What report() found; each entry is (buffer name, byte offset from the start of that buffer)."""

    def __init__(self, guards, inputs, unwritten):
        self.guards, self.inputs, self.unwritten = guards, inputs, unwritten

    @property
    def clean(self):
        return not (self.guards or self.inputs or self.unwritten)

    def __str__(self):
        def some(items):
            return f"{len(items)}: {items[:8]}{' ...' if len(items) > 8 else ''}"
        return f"guard bytes changed {some(self.guards)}; input bytes changed {some(self.inputs)}; output elements never written {some(self.unwritten)}"


class Arena:
    def __init__(self, bufs, guard_bytes, device="cpu"):
        self.bufs = {b.name: b for b in bufs}
        assert len(self.bufs) == len(bufs), "buffer names must differ"
        self.guard = (int(guard_bytes) + 255) // 256 * 256
        assert self.guard >= 256
        at = 0
        for b in bufs:                                                         # [guard][mod][buffer][pad to 256] ... [guard]
            b.start = at + self.guard + b.mod
            b.end = b.start + b.nbytes
            at = (b.end + 255) // 256 * 256
        self.size = at + self.guard
        raw = torch.full((self.size + 256,), POISON, dtype=torch.uint8, device=device)
        shift = -raw.data_ptr() % 256
        self.bytes = raw[shift:shift + self.size]
        assert self.bytes.data_ptr() % 256 == 0 and shift % 16 == 0
        for b in bufs:
            assert self[b.name].data_ptr() % 16 == b.mod, (b.name, self[b.name].data_ptr() % 16, b.mod)
        # the guards, as (start, end) byte runs of the arena between its buffers; no mask is built: the comparisons below run run
        # by run and buffer by buffer on the arena's own device (a workspace of 5 GiB would need as much again per mask, and
        # a mask built on the CPU would have to be copied there)
        self._gaps, at = [], 0
        for b in bufs:
            self._gaps.append((at, b.start))
            at = b.end
        self._gaps.append((at, self.size))
        self._sealed = None

    def __getitem__(self, name):
        """The buffer as a tensor of its own dtype and shape, a view of the arena."""
        b = self.bufs[name]
        return self.bytes[b.start:b.end].view(b.dtype).view(b.shape)

    def ptr(self, name):
        return self[name].data_ptr()

    def leading_guard(self, name):
        """Bytes of poison between this buffer and the one in front of it (or the start of the arena)."""
        b = self.bufs[name]
        return b.start - max([o.end for o in self.bufs.values() if o.end <= b.start], default=0)

    def trailing_guard(self, name):
        b = self.bufs[name]
        return min([o.start for o in self.bufs.values() if o.start >= b.end], default=self.size) - b.end

    def fill(self, name, value):
        """Copy an input in (bit for bit: same dtype, same shape)."""
        view = self[name]
        assert value.dtype == view.dtype and tuple(value.shape) == tuple(view.shape), (name, value.dtype, tuple(value.shape))
        view.copy_(value)

    def seal(self):
        """Remember the arena as it is now, inputs in place: what report() compares the inputs with."""
        self._sealed = {b.name: self.bytes[b.start:b.end].clone() for b in self.bufs.values() if b.role in ("in", "inout")}

    def _locate(self, positions):
        """(name, offset) per arena byte position: inside a buffer that buffer, outside the nearer one."""
        out = []
        for p in positions:
            best = None
            for b in self.bufs.values():
                dist = 0 if b.start <= p < b.end else (b.start - p if p < b.start else p - b.end + 1)
                if best is None or dist < best[0]:
                    best = (dist, b)
            out.append((best[1].name, p - best[1].start))
        return out

    def _where(self, lo, hi, other=None):
        """Arena byte positions in [lo, hi) that differ from the poison -- or from `other`, a tensor of hi - lo bytes."""
        out = []
        for a in range(lo, hi, CHUNK):
            b = min(hi, a + CHUNK)
            bad = self.bytes[a:b] != (POISON if other is None else other[a - lo:b - lo])
            if bool(bad.any()):
                out += [a + i for i in bad.nonzero().flatten().cpu().tolist()]
        return out

    def sealed(self, name):
        """The buffer as seal() found it ("in" and "inout" buffers), in its own dtype and shape."""
        b = self.bufs[name]
        return self._sealed[name].view(b.dtype).view(b.shape)

    def touched_outside(self, name, ranges):
        """For a "work" buffer and `ranges` = [(offset, bytes), ...] relative to its start: the byte offsets of the buffer that lie
        outside every range and no longer hold the poison, in ascending order."""
        b = self.bufs[name]
        assert b.role == "work", (name, b.role)
        out, at = [], 0
        for off, n in sorted((int(o), int(n)) for o, n in ranges if n > 0):
            assert 0 <= off and off + n <= b.nbytes, (name, off, n, b.nbytes)
            if off > at:
                out += self._where(b.start + at, b.start + off)
            at = max(at, off + n)
        if at < b.nbytes:
            out += self._where(b.start + at, b.end)
        return [p - b.start for p in out]

    def still_poison(self, name):
        """True when every byte of the buffer is still 0xFF: nothing was launched on it."""
        b = self.bufs[name]
        return not self._where(b.start, b.end)

    def report(self, reference):
        """`reference`: {output name: the tensor the output is expected to equal}; every "out" buffer needs one."""
        assert self._sealed is not None, "seal() the arena after the inputs are in"
        cur = self.bytes
        guards = self._locate([p for lo, hi in self._gaps for p in self._where(lo, hi)])
        inputs = self._locate([p for b in self.bufs.values() if b.role == "in" for p in self._where(b.start, b.end, self._sealed[b.name])])
        unwritten = []
        for b in self.bufs.values():
            if b.role != "out":
                continue
            got, want = words(self[b.name]), words(reference[b.name].to(cur.device))
            assert got.shape == want.shape and got.dtype == want.dtype, (b.name, tuple(got.shape), tuple(want.shape), got.dtype, want.dtype)
            left = (got == poison_of(got)) & (want != poison_of(got))
            unwritten += [(b.name, got.element_size() * i) for i in left.nonzero().flatten().cpu().tolist()]
        return Report(guards, inputs, unwritten)
