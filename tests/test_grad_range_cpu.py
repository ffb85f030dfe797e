"""The sweep harness of tests/grad_sweep.py, held to account before it judges a kernel (no GPU).

The "kernels" here are torch emulations on the CPU of x^T v with 256 rows, x unit normal stored in a 16-bit type and v =
fp32 unit normal x 2^k fed as an unscaled hi + lo pair of that type (what lora_grad_mfma_kernel and lg_split do), compared
with float64 on the same rounded x at 2e-4 of max |ref| - the bound lora_grad_partial_ln_case puts on that kernel."""
import torch

from tests import grad_sweep as GS

ROWS, K, R = 256, 64, 8
TOL = 2e-4


def operands(k):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(ROWS, K, generator=g)
    v = torch.randn(ROWS, R, generator=g) * 2.0 ** k
    return x, v


def product_run(dt, hi_only=False, exact=False, flush_out=False):
    def run(k, rec):
        x, v = operands(k)
        ref = x.to(dt).double().t() @ v.double()
        got = ref.clone() if exact else GS.hilo_product(x, v, dt, hi_only)
        if flush_out:                                      # a half-stored output that a kernel flushed to zero
            got, ref = torch.zeros_like(ref, dtype=torch.float16), ref
        rec(got, ref, TOL, "x^T v")
    return run


def test_half_hi_lo_pair_crosses_its_bound_between_2_to_minus_12_and_minus_16():
    table = GS.sweep(product_run(torch.float16))
    assert sorted(table) == list(GS.K_GRID)                 # fp32 output: nothing stops the sweep below the grid's top
    low = GS.lowest_holding(table)
    print(GS.report("emulated f16 hi + lo", table, (-16, 0)))
    assert -16 < low <= -12, low
    assert all(table[k][0].ok for k in table if k >= -12) and not any(table[k][0].ok for k in table if k <= -16)
    # the error grows as the operand sinks: one binade of |v| lost = one bit of the pair lost
    assert table[-20][0].rel > 10 * table[-12][0].rel > 100 * table[0][0].rel
    # ... and the harness fails a window that reaches below the crossing, passes one above it
    GS.assert_sweep("f16 hi + lo, window above the crossing", table, (-12, 6))
    try:
        GS.assert_sweep("f16 hi + lo, window below the crossing", table, (-18, 0))
    except AssertionError as e:
        assert "k=-16" in str(e) and "k=-18" in str(e) and "k=-12" not in str(e)
    else:
        raise AssertionError("a window that reaches 2^-18 passed")


def test_half_hi_only_is_flagged_everywhere_and_bfloat16_hi_only_too():
    """Without the lo half the operand carries 11 (8) bits: 256 rounding errors of up to 2^-12 (2^-9) of |v| add up to
    ~ 2^-12 sqrt(256 / 3) ~ 2e-3 (1.8e-2) of one term against max |ref| ~ 4 sqrt(256) / 16 terms: 1e-4 .. 1e-3 - above or at
    the bound for bf16 at every k, and for half wherever the pair was; the harness must never call hi-only better than the pair."""
    pair, hi = GS.sweep(product_run(torch.float16)), GS.sweep(product_run(torch.float16, hi_only=True))
    assert all(hi[k][0].err >= pair[k][0].err for k in pair)
    assert hi[0][0].rel > 100 * pair[0][0].rel
    b = GS.sweep(product_run(torch.bfloat16, hi_only=True))
    assert GS.lowest_holding(b) is None and not any(b[k][0].ok for k in b)


def test_bfloat16_pair_is_flat():
    table = GS.sweep(product_run(torch.bfloat16))
    rels = [table[k][0].rel for k in sorted(table)]
    assert max(rels) <= min(rels) * (1 + 1e-9), rels        # a power of two moves neither half of the pair
    assert max(rels) < TOL / 10 and GS.lowest_holding(table) == GS.K_GRID[0]
    GS.assert_sweep("bf16 hi + lo", table, (GS.K_GRID[0], GS.K_GRID[-1]))


def test_exact_kernel_is_accepted_at_every_k():
    table = GS.sweep(product_run(torch.float16, exact=True))
    assert sorted(table) == list(GS.K_GRID) and all(e.ok and e.err == 0.0 for k in table for e in table[k])
    GS.assert_sweep("float64", table, (GS.K_GRID[0], GS.K_GRID[-1]))


def test_subnormal_allowance_does_not_hide_an_output_flushed_to_zero():
    """2^-25 is half of half's subnormal spacing: it covers the rounding of a stored half, not a flush.  A half-stored output
    of all zeros fails wherever max |ref| >= 2^-14 (the smallest normal) - and passes only where the reference itself is
    within the allowance."""
    table = GS.sweep(product_run(torch.float16, flush_out=True))
    for k, (e,) in table.items():
        assert e.half
        if e.refmax >= 2.0 ** -14:
            assert not e.ok, (k, e.refmax)
        assert e.ok == (e.refmax <= TOL * e.refmax + 2.0 ** -25), (k, e.refmax)
    assert any(e.refmax >= 2.0 ** -14 for (e,) in table.values())
    rec = GS.Recorder()
    for i, ref in enumerate((2.0 ** -26, 2.0 ** -24, 2.0 ** -14)):     # rounds to zero / the smallest subnormal / the smallest normal
        rec(torch.zeros(3, dtype=torch.float16), torch.full((3,), ref, dtype=torch.float64), TOL, f"zeros against {ref}")
    assert [e.ok for e in rec.entries] == [True, False, False]


def test_sweep_stops_below_a_quarter_of_halfs_largest_number():
    def run(k, rec):
        x, v = operands(k)
        ref = x.double().t() @ v.double()
        rec(ref.to(torch.float16), ref, 2e-3, "half-stored x^T v")
    table = GS.sweep(run)
    top = max(table)
    assert all(e.refmax < GS.HALF_TOP for k in table for e in table[k])
    x, v = operands(top + 2)
    assert float((x.double().t() @ v.double()).abs().max()) >= GS.HALF_TOP      # the next point would have crossed
    assert all(e.ok for k in table for e in table[k])       # a correctly rounded half output holds 2e-3 + 2^-25 at every k


def test_windows_need_four_points_and_nan_fails_outside_the_window():
    def run(k, rec):
        ref = torch.ones(4, dtype=torch.float64) * 2.0 ** k
        got = ref.clone().float()
        if k == -24:
            got[1] = float("nan")
        rec(got, ref, 1e-6, "out")
    table = GS.sweep(run)
    for window, word in (((-3, 1), "fewer than 4"), ((-10, 0), "NaN where the float64 reference is finite")):
        try:
            GS.assert_sweep("t", table, window)
        except AssertionError as e:
            assert word in str(e), str(e)
        else:
            raise AssertionError(f"window {window} passed")


def test_homogeneity_check_sees_an_absolute_threshold():
    def make(eps):
        def run(k, rec):
            g = torch.Generator().manual_seed(5)
            x = torch.randn(64, 32, generator=g)
            dy = (torch.randn(64, 32, generator=g) * 2.0 ** k).bfloat16()
            out = (dy.float() * x / (x * x + 1) + eps).bfloat16()
            rec(x.bfloat16(), x.double(), 1e-2, "forward output")
            rec(out, dy.double() * x.double() / (x.double() ** 2 + 1), 1e-2, "gradient")
        return run
    for k in (-20, 20):
        assert GS.homogeneous(make(0.0), k) == []
        bad = GS.homogeneous(make(1e-6), k)                 # an epsilon on the gradient path
        assert len(bad) == 1 and bad[0].startswith("gradient"), (k, bad)
