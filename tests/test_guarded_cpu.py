"""tests/guarded.py must be able to fail: every fault it exists to catch, simulated on CPU tensors by writing into the backing
buffer directly, raises and names the buffer and the offset; what the contract leaves undefined does not."""
import pytest
import torch

from tests.guarded import ALIGN, BAND_ROWS, MIN_BAND_BYTES, Guarded, guard_fixture

DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int64]
IDS = ["f32", "bf16", "f16", "i32", "i64"]


@pytest.fixture
def g():
    yield from guard_fixture("cpu")


def _fill(t):
    """What a correct kernel does: every element of the body written."""
    t.copy_(torch.arange(t.numel()).reshape(t.shape).to(t.dtype))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_layout_and_a_clean_run(g, dt):
    M, ld = 37, 24
    t = g.out(M, ld, dtype=dt, name="out")
    b = g.record(t)
    item = t.element_size()
    assert t.shape == (M, ld) and t.is_contiguous() and t.dtype == dt
    assert b.band * item >= max(BAND_ROWS * ld * item, MIN_BAND_BYTES) and (b.band * item) % ALIGN == 0
    assert t.data_ptr() == b.flat.data_ptr() + b.band * item and t.data_ptr() % 16 == 0
    assert b.flat.numel() == 2 * b.band + M * ld
    if dt.is_floating_point:
        assert bool(torch.isnan(t).all()), "the body is poisoned with NaN"
        assert bool(torch.isfinite(b.flat[:b.band].float()).all()), "the bands hold a non-NaN pattern"
    wide = g.out(5, 3072, dtype=dt, name="wide")          # 256 rows of a wide output exceed the 64 KiB floor
    assert g.record(wide).band * item == 256 * 3072 * item
    one = g.out(7, dtype=dt, name="one")
    assert g.record(one).band * item == MIN_BAND_BYTES
    for x in (t, wide, one):
        _fill(x)
    g.check()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_a_write_one_element_after_the_body(g, dt):
    M, ld = 5, 24
    other = g.out(3, dtype=dt, name="other")
    t = g.out(M, ld, dtype=dt, name="victim")
    _fill(t), _fill(other)
    b = g.record(t)
    b.flat[b.band + M * ld] = 1
    with pytest.raises(AssertionError, match=rf"behind 'victim' .*\(row {M}, column 0\)"):
        g.check()


def test_a_write_one_row_after_the_body(g):
    M, ld = 5, 24
    t = g.out(M, ld, dtype=torch.bfloat16, name="rows")
    _fill(t)
    b = g.record(t)
    b.flat[b.band + M * ld + 3:b.band + (M + 1) * ld] = 2.0           # columns 3.. of row M: a tail tile's extra row
    with pytest.raises(AssertionError, match=rf"behind 'rows' .*\(row {M}, column 3\).* {ld - 3} element"):
        g.check()


def test_bands_are_compared_bit_for_bit(g):
    """One flipped sign bit in the band behind a 1-D output trips, and is reported at its index."""
    t = g.out(4, dtype=torch.float32, name="bits")
    _fill(t)
    b = g.record(t)
    b.flat[b.band + 4 + 10] = -b.flat[b.band + 4 + 10]                # same magnitude, other sign bit
    with pytest.raises(AssertionError, match=r"behind 'bits' .*\(row 0, column 14\)"):
        g.check()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_a_write_one_element_before_the_body(g, dt):
    M, ld = 5, 24
    t = g.out(M, ld, dtype=dt, name="front")
    _fill(t)
    b = g.record(t)
    b.flat[b.band - 1] = 1
    with pytest.raises(AssertionError, match=rf"in front of 'front' .*\(row -1, column {ld - 1}\)"):
        g.check()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_a_body_element_left_unwritten(g, dt):
    M, ld = 5, 24
    t = g.out(M, ld, dtype=dt, name="holes")
    keep = t[3, 7].clone()
    _fill(t)
    t[3, 7] = keep                                                     # the kernel skipped (3, 7)
    with pytest.raises(AssertionError, match=r"'holes' .*\(row 3, column 7\) was never written \(1 poisoned"):
        g.check()


def test_a_nan_the_kernel_computed_is_not_poison(g):
    t = g.out(8, dtype=torch.float32, name="nan")
    _fill(t)
    t[2] = float("nan")                                                # a value comparison's business, not the guard's
    g.check()


def test_a_body_element_outside_the_defined_part_passes(g):
    """Rows r..15 of a packed rank operand, the columns past the rank: undefined by contract, stated by the caller."""
    r = 5
    t = g.out(16, 32, dtype=torch.bfloat16, name="rk")
    t[:r] = 1.0
    with pytest.raises(AssertionError, match=rf"'rk' .*\(row {r}, column 0\) was never written"):
        g.check()
    g.check(defined=slice(0, r))                                       # an index ...
    mask = torch.zeros(16, 32, dtype=torch.bool)
    mask[:r] = True
    g.check(defined=mask, of=t)                                        # ... or a mask; kept for later plain checks
    g.check()
    t[1, 2] = g.record(t).flat[g.record(t).band + 16 * 32 - 1]         # poison inside the defined part still trips
    with pytest.raises(AssertionError, match=r"'rk' .*\(row 1, column 2\)"):
        g.check()
    t[1, 2] = 0.0


def test_a_query_sized_scratch_one_element_short_trips():
    """A kernel that needs n floats of scratch, given a guarded buffer of n - 1 (a query that promises too little): its last
    store lands in the band."""
    gd = Guarded("cpu")
    n = 2 * 37 * 3
    part = gd.out(n - 1, name="part")
    b = gd.record(part)
    b.flat[b.band:b.band + n] = 0.5                                    # the kernel's n stores
    with pytest.raises(AssertionError, match=rf"behind 'part' .*\(row 0, column {n - 1}\)"):
        gd.check()


# ------------------------------------------------------------ windows: a row stride wider than the rows ---
LAYOUTS = [(24, 8, 72), (24, 0, 72), (24, 48, 72), (24, 8, 32)]        # (cols, col0, ld): the three thirds, and the tight gap
LAYOUT_IDS = ["middle-third", "first-third", "last-third", "tight"]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("cols,col0,ld", LAYOUTS, ids=LAYOUT_IDS)
def test_window_layout_and_a_clean_run(g, dt, cols, col0, ld):
    M = 37
    w = g.window(M, ld, col0, cols, dtype=dt, name="win")
    b = g.record(w)
    item = w.element_size()
    assert w.shape == (M, cols) and w.stride() == (ld, 1) and w.dtype == dt
    assert b.shape == (M, ld) and b.body.is_contiguous() and b.window == (col0, cols)
    assert w.data_ptr() == b.body.data_ptr() + col0 * item and b.body.data_ptr() % 16 == 0
    assert w.data_ptr() % 16 == (col0 * item) % 16 and (ld * item) % 16 == 0          # col0 = 8: 16-byte aligned in every dtype
    assert b.band * item >= max(BAND_ROWS * ld * item, MIN_BAND_BYTES)                   # 256 rows of the STRIDE
    if dt.is_floating_point:
        assert bool(torch.isnan(b.body).all()), "window and gap are poisoned alike"
    _fill(w)
    g.check()
    assert torch.equal(w, torch.arange(M * cols).reshape(M, cols).to(dt))
    if dt.is_floating_point:
        gap = torch.ones(M, ld, dtype=torch.bool)
        gap[:, col0:col0 + cols] = False
        assert bool(torch.isnan(b.body[gap]).all())


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("side", ["left", "right"])
def test_a_write_into_the_gap_beside_a_window(g, dt, side):
    """One column left of the window and one column right of it: neither a band nor a poison check of the window sees it."""
    M, cols, col0, ld = 9, 24, 24, 72
    w = g.window(M, ld, col0, cols, dtype=dt, name="third")
    _fill(w)
    col = col0 - 1 if side == "left" else col0 + cols
    g.record(w).body[4, col] = 1
    with pytest.raises(AssertionError, match=rf"'third' \[{M}, {ld}\], window columns \[{col0}, {col0 + cols}\).*outside the window "
                                             rf"changed: first at \(row 4, column {col}\).* 1 element"):
        g.check()


def test_a_vector_store_one_lane_too_wide_into_a_tight_gap(g):
    """ld = cols + 8, col0 = 8: eight elements past the last column of a row are the gap of the next row - and past the last
    row, the band.  The gap is reported first: it names the row the spill came from."""
    M, cols, col0, ld = 5, 24, 8, 32
    w = g.window(M, ld, col0, cols, dtype=torch.bfloat16, name="tight")
    _fill(w)
    b = g.record(w)
    for r in range(1, M):                                              # what every row but the last leaves ...
        b.body[r, :8] = 2.0
    b.flat[b.band + M * ld:b.band + M * ld + 8] = 2.0                  # ... and the last
    with pytest.raises(AssertionError, match=rf"'tight' .*first at \(row 1, column 0\).* {8 * (M - 1)} element"):
        g.check()
    b.body[1:, :8] = b.body[0, :8]                                     # the poison back into the gap: the band is left
    with pytest.raises(AssertionError, match=rf"behind 'tight' .*\(row {M}, column 0\).* 8 element"):
        g.check()


def test_the_gap_is_compared_bit_for_bit(g):
    """Another NaN in the gap is a change: the poison is one NaN, compared through the integer view."""
    w = g.window(4, 32, 8, 24, dtype=torch.float32, name="bits")
    _fill(w)
    g.check()
    g.record(w).body[1, 3] = float("nan")                              # the default NaN, not the poison's payload
    with pytest.raises(AssertionError, match=r"'bits' .*first at \(row 1, column 3\)"):
        g.check()


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_a_window_element_left_unwritten(g, dt):
    M, cols, col0, ld = 5, 24, 8, 32
    w = g.window(M, ld, col0, cols, dtype=dt, name="holes")
    keep = w[3, 7].clone()
    _fill(w)
    w[3, 7] = keep                                                     # the kernel skipped (3, 7) of the window
    with pytest.raises(AssertionError, match=rf"'holes' .*\(row 3, column {col0 + 7}\) was never written \(1 poisoned"):
        g.check()


def test_a_frozen_gap_leaves_scratch_and_defined_parts_as_they_were(g):
    """Frozen is a property of a window alone: beside one, a scratch body may still be written anywhere or nowhere, and
    check(defined=) still restricts the poison check of a plain output - and still trips inside the defined part."""
    w = g.window(6, 32, 8, 24, dtype=torch.float16, name="win")
    sc = g.scratch(6, 32, dtype=torch.float16, name="scratch")
    t = g.out(16, 32, dtype=torch.bfloat16, name="rk")
    _fill(w)
    t[:5] = 1.0
    with pytest.raises(AssertionError, match=r"'rk' .*\(row 5, column 0\) was never written"):
        g.check()
    g.check(defined=slice(0, 5), of=t)
    g.check()                                                          # scratch untouched: accepted
    sc[2, :9] = 3.0                                                    # written where the window's gap would be: accepted
    sc[5, 31] = 3.0
    g.check()
    t[1, 2] = g.record(t).flat[g.record(t).band + 16 * 32 - 1]         # poison inside the defined part still trips
    with pytest.raises(AssertionError, match=r"'rk' .*\(row 1, column 2\)"):
        g.check()
    t[1, 2] = 0.0
    g.record(sc).flat[g.record(sc).band - 1] = 1                       # ... and so does a scratch body's band
    with pytest.raises(AssertionError, match=r"in front of 'scratch'"):
        g.check()


def test_window_in_surrounds_the_source_with_nan(g):
    src = torch.arange(5 * 24, dtype=torch.float32).reshape(5, 24).to(torch.bfloat16)
    v = g.window_in(5, 32, 8, src)
    assert v.shape == (5, 24) and v.stride() == (32, 1) and v.data_ptr() % 16 == 0 and torch.equal(v, src)
    whole = torch.as_strided(v, (5, 32), (32, 1), v.storage_offset() - 8)
    assert bool(torch.isnan(whole[:, :8]).all()) and torch.equal(whole[:, 8:], src)
    with pytest.raises(KeyError):
        g.record(v)                                                    # an input: nothing to check


def test_the_fixture_fails_when_a_buffer_was_never_checked():
    gen = guard_fixture("cpu")
    gd = next(gen)
    t = gd.out(4, name="forgotten")
    _fill(t)
    with pytest.raises(AssertionError, match="never checked: \\['forgotten'\\]"):
        next(gen)
    gen = guard_fixture("cpu")
    gd = next(gen)
    _fill(gd.out(4, name="seen"))
    gd.check()
    with pytest.raises(StopIteration):
        next(gen)
