"""Guard bands and poisoned bodies for kernel outputs.

A kernel test that compares only what a kernel left INSIDE its output tensor cannot see two kinds of bug: a store outside
the tensor (a ragged tail tile that writes one row too many, a scratch query that promises too little) and an element that
was never written (the caching allocator hands back the previous case's result, which has the right size and magnitude).

`Guarded.out(*shape, dtype=...)` allocates one flat backing buffer laid out as  lead | body | trail  and returns the
contiguous body view:
  * both bands are filled with the byte 0xA5 (a finite value in every float format) and compared BITWISE through an integer
    view; a band is at least 256 rows of the body's last dimension (the tallest GEMM tile: a whole overrunning tail tile lands
    in the band, not in somebody else's memory) and at least 64 KiB, rounded up to a multiple of 256 bytes, so the body keeps
    the alignment of the allocation;
  * the body is filled with a NaN of a fixed payload (integer outputs: the byte 0x5A); an element that still holds exactly
    those bits after the launch was never written.

`check()` synchronises, then asserts for every registered buffer that both bands are untouched and that no poison is left in
the body; a failure names the buffer and the (row, column) of the first offending element in the body's layout (rows below 0
are in front of the body, rows >= the body's row count behind it).  Where the contract leaves part of a buffer undefined,
`check(defined=mask_or_index, of=buffer)` restricts the poison check of that buffer to the defined part; the caller states it
from include/ffm_hip.h, never from what the kernel happened to write.

`Guarded.window(rows, ld, col0, cols, dtype=...)` is the same for an operand whose row stride is wider than its rows: the
body is [rows, ld], the tensor handed out is the strided view body[:, col0:col0 + cols], and everything of the body outside
that view is FROZEN - `check()` also asserts that every such element still holds the poison bits, bit for bit, and names the
(row, column) of the first that does not.  A store that spills from a window into the gap between its width and its row
stride lands there, where neither a band nor a value comparison would see it.  `Guarded.window_in(rows, ld, col0, src)` is
the input twin: `src` inside a [rows, ld] tensor of NaN, so that a load that strays out of the window and reaches an
accumulator turns the result NaN.

Every test file defines its own fixture around this class (see `guard_fixture`); the fixture fails at teardown when a
registered buffer was never checked.
"""
import torch

BAND_BYTE = 0xA5
INT_POISON_BYTE = 0x5A
MIN_BAND_BYTES = 64 << 10
BAND_ROWS = 256
ALIGN = 256

# NaNs with a payload no arithmetic produces, as the integer of the same width
_POISON = {torch.float32: 0x7FC5A5A5, torch.float64: 0x7FF85A5A5A5A5A5A, torch.bfloat16: 0x7FDA, torch.float16: 0x7EDA}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _repeat_byte(byte, size):
    """The signed integer of `size` bytes whose every byte is `byte`."""
    v = int.from_bytes(bytes([byte]) * size, "little", signed=False)
    if size > 1 and v >= 1 << (8 * size - 1):
        v -= 1 << (8 * size)
    return v


class _Buf:
    def __init__(self, name, shape, dtype, device):
        self.name, self.shape, self.dtype = name, tuple(shape), dtype
        self.item = torch.empty((), dtype=dtype).element_size()
        self.ld = self.shape[-1] if len(self.shape) >= 2 else 1   # 1-D: 64 KiB bands, offsets as (0, index)
        self.numel = 1
        for s in self.shape:
            self.numel *= s
        band = max(BAND_ROWS * self.ld * self.item, MIN_BAND_BYTES)
        band = (band + ALIGN - 1) // ALIGN * ALIGN
        self.band = band // self.item                     # elements per band (ALIGN is a multiple of every item size)
        self.ints = torch.empty(2 * self.band + self.numel, dtype=_INT_VIEW[self.item], device=device)
        self.band_bits = _repeat_byte(BAND_BYTE, self.item)
        self.poison_bits = _POISON[dtype] if dtype in _POISON else _repeat_byte(INT_POISON_BYTE, self.item)
        self.ints.fill_(self.band_bits)
        self.ints[self.band:self.band + self.numel].fill_(self.poison_bits)
        self.flat = self.ints.view(dtype)                  # the whole backing buffer in the output's dtype
        self.body = self.flat[self.band:self.band + self.numel].view(self.shape)
        self.view = self.body                              # what the caller holds (a window: a strided part of the body)
        self.window = None                                 # (col0, cols): only these columns of the body may change
        self.defined = None
        self.checked = False

    def set_window(self, col0, cols):
        assert len(self.shape) == 2 and 0 <= col0 and cols > 0 and col0 + cols <= self.ld, "a window lies inside its rows"
        self.window = (col0, cols)
        self.view = self.body[:, col0:col0 + cols]

    def rowcol(self, linear):
        """(row, column) in the body's layout of the element `linear` elements after the body's first."""
        return (linear // self.ld, linear % self.ld) if len(self.shape) >= 2 else (0, linear)

    def check(self):
        self.checked = True
        left = self.ints[self.band:self.band + self.numel] == self.poison_bits
        if self.window is not None:                        # (ahead of the bands: a spill reaches the gap of the next row first)
            inside = torch.zeros(self.shape, dtype=torch.bool, device=self.ints.device)
            inside[:, self.window[0]:self.window[0] + self.window[1]] = True
            inside = inside.reshape(-1)
            changed = ~left & ~inside
            if bool(changed.any()):
                first = int(changed.nonzero()[0])
                r, c = self.rowcol(first)
                lo, hi = self.window[0], self.window[0] + self.window[1]
                raise AssertionError(f"'{self.name}' {list(self.shape)}, window columns [{lo}, {hi}): the frozen part outside the window "
                                     f"changed: first at (row {r}, column {c}) of the body's layout, {int(changed.sum())} element(s) in all")
            left = left & inside
        lead, trail = self.ints[:self.band], self.ints[self.band + self.numel:]
        for band, base, where in ((lead, -self.band, "in front of"), (trail, self.numel, "behind")):
            ref = torch.full_like(band, self.band_bits)
            if not torch.equal(band, ref):
                first = int((band != ref).nonzero()[0])
                n = int((band != ref).sum())
                r, c = self.rowcol(base + first)
                raise AssertionError(f"guard band {where} '{self.name}' {list(self.shape)} changed: first at (row {r}, column {c}) "
                                     f"of the body's layout, {n} element(s) in all")
        if self.defined is not None:
            left &= self.defined.reshape(-1)
        if bool(left.any()):
            first = int(left.nonzero()[0])
            r, c = self.rowcol(first)
            raise AssertionError(f"'{self.name}' {list(self.shape)}: element (row {r}, column {c}) was never written "
                                 f"({int(left.sum())} poisoned element(s) left in the defined part)")


class Guarded:
    def __init__(self, device="cuda"):
        self.device = device
        self.bufs = []

    def out(self, *shape, dtype=torch.float32, name=None):
        """A poisoned, contiguous output of `shape` between two guard bands."""
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        b = _Buf(name or f"out{len(self.bufs)}", shape, dtype, self.device)
        self.bufs.append(b)
        return b.body

    def like(self, t, name=None):
        return self.out(*t.shape, dtype=t.dtype, name=name)

    def scratch(self, *shape, dtype=torch.float32, name=None):
        """Scratch whose contents the contract leaves undefined after the call (sized by a query or by the header's formula):
        the bands are guarded, no element of the body has to be written."""
        t = self.out(*shape, dtype=dtype, name=name)
        b = self.bufs[-1]
        b.defined = torch.zeros(b.shape, dtype=torch.bool, device=self.device)
        return t

    def window(self, rows, ld, col0, cols, dtype=torch.float32, name=None):
        """The strided view body[:, col0:col0 + cols] of a poisoned [rows, ld] body between two guard bands.  The window is the
        defined part; the rest of the body is frozen: `check()` fails when any element of it no longer holds the poison bits."""
        b = _Buf(name or f"window{len(self.bufs)}", (rows, ld), dtype, self.device)
        b.set_window(col0, cols)
        self.bufs.append(b)
        return b.view

    def window_in(self, rows, ld, col0, src):
        """An input behind a row stride: `src` [rows, cols] copied into columns col0.. of a [rows, ld] tensor of NaN, viewed as
        that window.  Not registered: nothing is checked on it - a load outside the window shows as NaN in what it feeds."""
        assert src.dim() == 2 and src.shape[0] == rows and col0 + src.shape[1] <= ld and src.dtype.is_floating_point
        body = torch.full((rows, ld), float("nan"), dtype=src.dtype, device=self.device)
        view = body[:, col0:col0 + src.shape[1]]
        view.copy_(src)
        return view

    def record(self, t):
        """The bookkeeping of a tensor this object handed out (tests of the helper reach the backing buffer through it)."""
        for b in self.bufs:
            if b.view.data_ptr() == t.data_ptr() and b.view.shape == t.shape and b.view.stride() == t.stride():
                return b
        raise KeyError("not a tensor from Guarded.out")

    def check(self, defined=None, of=None):
        """Bands untouched and no poison left, for every buffer (with `of`: for that buffer only).  `defined`: a bool mask of
        the body's shape, or an index (slice, tuple of slices, ...) into it - the part the contract defines; it is kept for
        later calls."""
        if self.device != "cpu":
            torch.cuda.synchronize()
        if defined is not None:
            if of is None:
                assert len(self.bufs) == 1, "check(defined=...) needs of=<buffer> when several buffers are registered"
                of = self.bufs[0].body
            b = self.record(of)
            assert b.window is None, "a window is defined as a whole"
            if isinstance(defined, torch.Tensor) and defined.dtype == torch.bool:
                mask = defined.to(self.device).expand(b.shape)
            else:
                mask = torch.zeros(b.shape, dtype=torch.bool, device=self.device)
                mask[defined] = True
            b.defined = mask.contiguous()
        for b in ([self.record(of)] if of is not None else self.bufs):
            b.check()

    def finish(self):
        """Teardown of the fixture: every buffer handed out must have been checked."""
        never = [b.name for b in self.bufs if not b.checked]
        self.bufs = []
        assert not never, f"guarded outputs never checked: {never}"


def guard_fixture(device="cuda"):
    """Body of the per-file fixture:  @pytest.fixture  def g(): yield from guard_fixture()"""
    gd = Guarded(device)
    yield gd
    gd.finish()
