"""Guard-banded, poisoned buffers for the memory-contract tests (test_memory_contract_cpu.py / _gpu.py).

`guarded` puts a tensor between two guard bands, `ExactScratch` stands in for `ops.scratch` and hands every wrapper a workspace
of exactly the size it asked for, filled with a pattern of the test's choice.  Both work on CPU and device tensors alike: the
harness tests itself on the CPU.

The arena of one buffer is  [front guard | payload | back guard]:

* with shift = s the payload starts s elements of its dtype past the 256-byte boundary instead of on it (an operand that is
  not 16-byte aligned: tests/alignment.py); the elements between the boundary and the payload belong to the front guard;
* the guards, and the padding columns of a strided payload (ld > shape[-1]), hold the 32-bit word GUARD_WORD.  Read as
  float32 or float64 it is a NaN, read as int32 / int64 it is negative: a kernel that reads past an input's extent and lets
  the value reach a result shows in the comparison of results, a kernel that writes there shows in `check()`;
* the payload holds POISON (a NaN of another bit pattern for floating types, a negative number for integers, 0xC3 bytes for
  uint8) until somebody writes it: `all_written()` finds what a kernel left out.

The back guard is max(1 MiB, payload bytes): 1 MiB is the floor of `ops.scratch`, so an overrun that lands silently inside the
shared scratch in the rest of the suite lands inside the test's own arena here.  The front guard is 64 KiB.

`guarded_far` is the sibling for row pitches of gigabytes (tests/far_pitch.py): a back guard of 1 MiB, a front guard of the
caller's choice, and a `check()` that reads the arena in place, piece by piece (GuardedFar below).
"""
import torch

GUARD_WORD = -23131                      # 0xFFFFA5A5: NaN as f32 and (doubled) as f64, negative as int32 / int64
FRONT_GUARD = 64 << 10
BACK_GUARD_MIN = 1 << 20
ALIGN = 256

# dtype -> (integer dtype of the same width, poison value in it)
_POISON = {
    torch.float32: (torch.int32, 0x7FC5A5A5),                          # a quiet NaN with a payload
    torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5),
    torch.int32: (torch.int32, -0x5A5A5A5B),
    torch.int64: (torch.int64, -0x5A5A5A5A5A5A5A5B),
    torch.uint8: (torch.uint8, 0xC3),
}

FILL_FF, FILL_00, FILL_HUGE = "ff", "00", "7f7fffff"
FILLS = (FILL_FF, FILL_00, FILL_HUGE)


def _itemsize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _pattern_arena(nbytes, device):
    """A uint8 tensor of at least nbytes + ALIGN bytes that repeats GUARD_WORD from its first byte."""
    words = (nbytes + ALIGN + 3) // 4
    return torch.full((words,), GUARD_WORD, dtype=torch.int32, device=device).view(torch.uint8)


class Guarded:
    """Handle of one guarded buffer: `.view` is the tensor to hand to a kernel."""

    def __init__(self, shape, dtype, device, ld=None, front=FRONT_GUARD, back=None, poison=True, shift=0):
        shape = tuple(int(s) for s in shape)
        assert len(shape) >= 1 and all(s >= 0 for s in shape)
        self.shape, self.dtype, self.device = shape, dtype, torch.device(device)
        cols = shape[-1]
        self.ld = cols if ld is None else int(ld)
        assert self.ld >= cols and (ld is None or len(shape) == 2), "a leading dimension goes with a 2-D payload"
        size = _itemsize(dtype)
        rows = 1
        for s in shape[:-1]:
            rows *= s
        self.rows, self.cols = rows, cols
        n_elem = 0 if rows == 0 or cols == 0 else (rows - 1) * self.ld + cols
        self.nbytes = n_elem * size
        assert front % 4 == 0 and front >= 0
        self.front = front
        self.shift = int(shift)
        assert 0 <= self.shift * size < ALIGN, "a shift is a few whole elements"
        self.back = max(BACK_GUARD_MIN, self.nbytes) if back is None else int(back)
        total = front + self.nbytes + self.back + self.shift * size
        self.arena = _pattern_arena(total, device)
        # the payload starts `shift` elements past the first 256-byte aligned address at or after `front` bytes into the arena
        self.off = front + (-(self.arena.data_ptr() + front)) % ALIGN + self.shift * size
        self.view = self._view_of(self.arena)
        assert self.view.data_ptr() % ALIGN == self.shift * size
        if poison and self.view.numel():
            idt, val = _POISON[dtype]
            self._int_view(self.arena).fill_(val)

    # -- views of an arena-shaped byte tensor
    def _flat(self, arena):
        return arena[self.off:self.off + self.nbytes].view(self.dtype)

    def _view_of(self, arena):
        flat = self._flat(arena)
        if self.rows == 0 or self.cols == 0:
            return flat.new_empty(self.shape)
        if len(self.shape) == 1:
            return flat
        if self.ld == self.cols:
            return flat.view(self.shape)
        return flat.as_strided(self.shape, (self.ld, 1))

    def _int_view(self, arena):
        idt, _ = _POISON[self.dtype]
        v = self._view_of(arena)
        return v if idt == self.dtype else v.view(idt)

    # -- checks
    def check(self, what="buffer"):
        """Every guard byte and every padding element is as it was made; else names the first damaged byte offset
        relative to the start of the payload (negative: in the front guard)."""
        got = self.arena.clone()
        want = _pattern_arena(self.arena.numel() - ALIGN, self.device)[:self.arena.numel()]
        assert want.numel() == got.numel()
        if self.view.numel():
            self._int_view(got).zero_()
            self._int_view(want).zero_()
        bad = (got != want).nonzero()
        if bad.numel():
            first = int(bad[0]) - self.off
            where = ("the front guard" if first < 0 else "the back guard" if first >= self.nbytes else "a padding column")
            raise AssertionError(f"{what}: {bad.numel()} guard bytes damaged, the first at byte offset {first} from the payload "
                                 f"start ({where}; payload {self.nbytes} bytes, shape {self.shape}, ld {self.ld}, {self.dtype})")

    def all_written(self, what="buffer"):
        """No element of the payload still holds the poison."""
        if not self.view.numel():
            return
        _, val = _POISON[self.dtype]
        left = (self._int_view(self.arena) == val).reshape(-1).nonzero()
        if left.numel():
            raise AssertionError(f"{what}: {left.numel()} of {self.view.numel()} elements were never written, the first at "
                                 f"flat index {int(left[0])} (shape {self.shape}, {self.dtype})")


def guarded(shape, dtype, device, ld=None, front=FRONT_GUARD, back=None, shift=0):
    """-> (view, handle): a poisoned tensor of `shape` (row pitch `ld` when given) between two guard bands, its first
    element `shift` elements past a 256-byte boundary."""
    h = Guarded(shape, dtype, device, ld=ld, front=front, back=back, shift=shift)
    return h.view, h


def guarded_copy(t, ld=None, front=FRONT_GUARD, back=None, shift=0):
    """-> (view, handle): the values of `t` in a guarded arena of its own (an input: what surrounds it reads as NaN / negative)."""
    v, h = guarded(t.shape, t.dtype, t.device, ld=ld, front=front, back=back, shift=shift)
    v.copy_(t)
    return v, h


FAR_BACK = 1 << 20
FAR_PIECE = 64 << 20                     # 32-bit words per piece of GuardedFar.check: 256 MiB read, a 64 MiB mask, one count


class GuardedFar:
    """`Guarded` for a 2-D payload whose row pitch is gigabytes (tests/far_pitch.py): [front guard | row 0 | gap | row 1 | ...
    | back guard], the first element on a 256-byte boundary.  The arena is filled with GUARD_WORD by one fill; only the
    payload rows are touched afterwards (the poison, or an input's values).  The back guard is 1 MiB, not the payload's
    extent, and `check()` reads the arena where it lies, FAR_PIECE words at a time: no clone, no copy to the host beyond one
    count per piece, and a 64 MiB mask as its only temporary (the far-pitch tests allow themselves 1 GiB).

    `front` is at least FRONT_GUARD.  The far-pitch table asks for more: an offset that a kernel truncated to 32 bits lands
    inside the arena by construction; one it sign-extended from 32 bits lands up to 2 GiB (a byte offset) or up to
    2^31 elements (an element index) in front of the base, and the front guard is sized to hold it."""

    def __init__(self, rows, cols, dtype, device, ld, front=FRONT_GUARD, poison=True, backing=None):
        rows, cols, ld, front = int(rows), int(cols), int(ld), int(front)
        size = _itemsize(dtype)
        assert rows >= 1 and cols >= 1 and ld >= cols and size in (4, 8), (rows, cols, ld, dtype)
        assert front >= FRONT_GUARD and front % ALIGN == 0
        self.shape, self.dtype, self.device = (rows, cols), dtype, torch.device(device)
        self.rows, self.cols, self.ld, self.size = rows, cols, ld, size
        self.front, self.back, self.shift = front, FAR_BACK, 0
        self.nbytes = ((rows - 1) * ld + cols) * size
        total = front + self.nbytes + self.back
        n_words = (total + ALIGN + 3) // 4
        if backing is None:
            self.words = torch.full((n_words,), GUARD_WORD, dtype=torch.int32, device=device)
        else:                            # the caller's memory (an int32 tensor it reuses from arena to arena): the same one fill
            assert backing.dtype == torch.int32 and backing.dim() == 1 and backing.numel() >= n_words and backing.device.type == self.device.type
            self.words = backing[:n_words]
            self.words.fill_(GUARD_WORD)
        self.arena = self.words.view(torch.uint8)
        self.off = front + (-(self.arena.data_ptr() + front)) % ALIGN
        self.view = self.arena[self.off:self.off + self.nbytes].view(dtype).as_strided((rows, cols), (ld, 1))
        assert self.view.data_ptr() % ALIGN == 0
        if poison:
            self._int_view().fill_(_POISON[dtype][1])

    def arena_bytes(self):
        return self.arena.numel()

    def _int_view(self):
        idt, _ = _POISON[self.dtype]
        return self.view if idt == self.dtype else self.view.view(idt)

    def _row_words(self, r):
        """[lo, hi): the 32-bit words of the arena that payload row r occupies."""
        lo = (self.off + r * self.ld * self.size) // 4
        return lo, lo + self.cols * self.size // 4

    def _where(self, word):
        byte = word * 4 - self.off
        if byte < 0:
            return byte, "the front guard"
        if byte >= self.nbytes:
            return byte, "the back guard"
        return byte, f"the gap after row {byte // (self.ld * self.size)}"

    def check(self, what="buffer", piece=FAR_PIECE):
        """Every byte in front of, between and behind the payload rows is as it was made; else names the first damaged byte
        offset relative to the start of the payload (negative: in the front guard)."""
        n = self.words.numel()
        pitch = self.ld * self.size // 4
        first_row_word = self.off // 4
        counts, pieces = [], []
        for s in range(0, n, piece):
            e = min(n, s + piece)
            bad = self.words[s:e] != GUARD_WORD
            # the payload rows that meet [s, e)
            r0 = max(0, (s - first_row_word - self.cols * self.size // 4) // pitch)
            for r in range(r0, self.rows):
                lo, hi = self._row_words(r)
                if lo >= e:
                    break
                if hi > s:
                    bad[max(lo, s) - s:min(hi, e) - s] = False
            counts.append(bad.sum())
            pieces.append(s)
            del bad
        counts = torch.stack(counts).cpu()
        total = int(counts.sum())
        if total:
            s = pieces[int(counts.nonzero()[0])]
            e = min(n, s + piece)
            bad = self.words[s:e] != GUARD_WORD
            for r in range(self.rows):
                lo, hi = self._row_words(r)
                if hi > s and lo < e:
                    bad[max(lo, s) - s:min(hi, e) - s] = False
            word = s + int(bad.nonzero()[0])
            byte, where = self._where(word)
            # the damaged word's first differing byte
            got = self.arena[word * 4:word * 4 + 4].cpu()
            want = torch.tensor([GUARD_WORD], dtype=torch.int32).view(torch.uint8)
            byte += int((got != want).nonzero()[0])
            raise AssertionError(f"{what}: {total} guard words damaged, the first at byte offset {byte} from the payload start "
                                 f"({where}; payload extent {self.nbytes} bytes, shape {self.shape}, ld {self.ld}, {self.dtype})")

    def all_written(self, what="buffer"):
        """No element of the payload rows still holds the poison."""
        _, val = _POISON[self.dtype]
        left = (self._int_view() == val).reshape(-1).nonzero()
        if left.numel():
            i = int(left[0])
            raise AssertionError(f"{what}: {left.numel()} of {self.rows * self.cols} elements were never written, the first at "
                                 f"flat index {i} (row {i // self.cols}, column {i % self.cols}; shape {self.shape}, ld {self.ld}, "
                                 f"{self.dtype})")

    def untouched(self):
        """Every element of the payload rows still holds the poison (a refused call's outputs)."""
        return bool((self._int_view() == _POISON[self.dtype][1]).all())


class FarColumns:
    """Columns [c0, c1) of a GuardedFar payload as an operand of their own: blocks that share one `ld` parameter are column
    slices of one wide matrix, each row [block 0 | block 1 | ...] and then the gap.  `check()` is the arena's (every block
    of the row is payload, whoever writes it); `all_written()` and `untouched()` look at this block's columns only."""

    def __init__(self, parent, c0, c1):
        assert 0 <= c0 < c1 <= parent.cols
        self.parent, self.c0, self.c1 = parent, c0, c1
        self.view = parent.view[:, c0:c1]
        self.dtype, self.shape = parent.dtype, (parent.rows, c1 - c0)

    def _int_view(self):
        return self.parent._int_view()[:, self.c0:self.c1]

    def check(self, what="buffer", piece=FAR_PIECE):
        self.parent.check(what, piece=piece)

    def all_written(self, what="buffer"):
        left = (self._int_view() == _POISON[self.dtype][1]).reshape(-1).nonzero()
        if left.numel():
            i, cols = int(left[0]), self.c1 - self.c0
            raise AssertionError(f"{what}: {left.numel()} of {self.parent.rows * cols} elements were never written, the first at "
                                 f"flat index {i} (row {i // cols}, column {i % cols} of columns [{self.c0}, {self.c1}); ld "
                                 f"{self.parent.ld}, {self.dtype})")

    def untouched(self):
        return bool((self._int_view() == _POISON[self.dtype][1]).all())


def guarded_far(shape, dtype, device, ld, front=FRONT_GUARD, backing=None):
    """-> (view, handle): a poisoned [rows, cols] tensor at the far row pitch `ld`."""
    h = GuardedFar(shape[0], shape[1], dtype, device, ld, front=front, backing=backing)
    return h.view, h


def guarded_far_copy(t, ld, front=FRONT_GUARD, backing=None):
    """-> (view, handle): the values of the 2-D tensor `t` at the far row pitch `ld`, GUARD_WORD everywhere else."""
    h = GuardedFar(t.shape[0], t.shape[1], t.dtype, t.device, ld, front=front, poison=False, backing=backing)
    h.view.copy_(t)
    return h.view, h


class ExactScratch:
    """Stand-in for `ops.scratch` (monkeypatch.setattr(ops, "scratch", ExactScratch(fill))): a request of n bytes returns a
    uint8 view of exactly n bytes (16 when n == 0), 256-byte aligned, inside a guarded arena, and filled with `fill` before
    every call.  Keyed per (device, stream) like ops.scratch, and per size: a stream that asks for the sizes a, b, a gets
    its first arena back, so consecutive kernels do reuse one workspace.  Arenas are never freed while the object lives:
    a kernel queued on a side stream may still be using one."""

    def __init__(self, fill=FILL_FF):
        assert fill in FILLS, fill
        self.fill = fill
        self.arenas = {}                 # (device index, stream, nbytes) -> Guarded
        self.calls = 0

    def _fill(self, v):
        if self.fill == FILL_FF:
            v.fill_(0xFF)
        elif self.fill == FILL_00:
            v.zero_()
        else:
            n4 = v.numel() // 4 * 4
            v[:n4].view(torch.int32).fill_(0x7F7FFFFF)
            v[n4:].fill_(0x7F)

    def __call__(self, nbytes, device):
        from vit_som_amd import _lib
        dev = torch.device(device)
        n = max(int(nbytes), 0) or 16
        self.calls += 1
        if dev.type != "cuda":
            return self._get((0, 0, n), n, dev)
        # allocate and fill on the stream the kernel will run on (ops.on_stream forces launches onto a side stream that
        # is not torch's current one): the fill is then ordered before the kernel and after the workspace's last user
        with torch.cuda.stream(_lib.launch_torch_stream()):
            return self._get((dev.index or 0, _lib.stream(), n), n, dev)

    def _get(self, key, n, dev):
        h = self.arenas.get(key)
        if h is None:
            h = self.arenas[key] = Guarded((n,), torch.uint8, dev, poison=False)
        self._fill(h.view)
        return h.view

    def check(self):
        for key, h in self.arenas.items():
            h.check(f"workspace of {key[2]} bytes (device {key[0]}, stream {key[1]:#x})")
