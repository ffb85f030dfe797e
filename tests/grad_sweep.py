"""Sweeps of a backward kernel over the magnitude of its gradient operands (tests/test_grad_range_gpu.py; held to account on
the CPU by tests/test_grad_range_cpu.py before it judges a kernel).

The fp16 mode multiplies dL/dlogits by a scale that moves between 2^12 and 1 (engine.py, `scale_state`), so the gradient
operands of every backward kernel wander over many binades while everything the forward left behind stays where it is.  A
`run(k)` here executes one case of a kernel with gradient operands = unit normal x 2^k (rounded to the storage type after
scaling) and hands every (output, float64 reference from the same rounded inputs, tolerance) to a `Recorder`, which stands in
for the `check(got, ref, tol, what)` of the kernel's existing test - same reference, same tolerance.

Two families:
  (a) `homogeneous(...)`: K(2^k g) == 2^k K(g) bit for bit, the right side scaled exactly in its own storage type;
  (b) `sweep(...)` / `assert_sweep(...)`: at every k inside the operand's working window  max |got - ref| <= tol max |ref|
      (+ 2^-25, half of half's subnormal spacing, for an output stored as IEEE half: the storage's own error); outside it only
      "no NaN where the reference is finite".  The sweep stops below the k at which the float64 reference of a half-stored
      output would reach 65504 / 4 (overflow is the scale guard's business).
"""
import math

import torch

K_GRID = tuple(range(-26, 13, 2))          # unit normal x 2^12 still fits IEEE half as an INPUT (5.5 sigma x 4096 < 65504)
HALF_SUBNORMAL_HALF_STEP = 2.0 ** -25
HALF_TOP = 65504.0 / 4


class Entry:
    __slots__ = ("what", "err", "refmax", "tol", "half", "nan", "ok", "got", "ref")

    def __init__(self, what, got, ref, tol, keep, ok=None, err=None):
        g, r = got.detach().double(), ref.detach().double()
        self.what, self.tol = what, tol
        self.half = got.dtype == torch.float16
        self.refmax = float(r.abs().max()) if r.numel() else 0.0
        self.err = float((g - r).abs().max()) if (r.numel() and err is None) else (err or 0.0)
        self.nan = bool((torch.isnan(g) & torch.isfinite(r)).any())
        allow = tol * self.refmax + (HALF_SUBNORMAL_HALF_STEP if self.half else 0.0)
        self.ok = (math.isfinite(self.err) and self.err <= allow and not self.nan) if ok is None else (bool(ok) and not self.nan)
        self.got = got.detach().clone() if keep else None
        self.ref = r.clone() if keep else None

    @property
    def rel(self):
        return self.err / self.refmax if self.refmax > 0 else (0.0 if self.err == 0 else math.inf)


class Recorder:
    """Stands in for check(got, ref, tol, what): records instead of asserting.  keep: also keep the tensors (family (a))."""

    def __init__(self, keep=False):
        self.keep, self.entries = keep, []

    def _name(self, what):
        n = sum(1 for e in self.entries if e.what == what or e.what.startswith(what + " #"))
        return what if n == 0 else f"{what} #{n}"

    def __call__(self, got, ref, tol, what):
        self.entries.append(Entry(self._name(what), got, ref, tol, self.keep))

    def custom(self, what, got, ref, ok, err):
        """A bound of another form (element-wise, from a float32 run of the reference): the caller states the verdict."""
        self.entries.append(Entry(self._name(what), got, ref, 0.0, self.keep, ok=ok, err=err))


def in_window(k, window):
    """window = (lo, hi) as log2 of the operand's rms; unit normal x 2^k has rms 2^k."""
    return window[0] <= k <= window[1]


def points_in(window, grid=K_GRID):
    return [k for k in grid if in_window(k, window)]


def sweep(run, grid=K_GRID):
    """{k: [Entry]} for the k of `grid`, ascending, stopping in front of the k at which the float64 reference of a half-stored
    output would reach 65504 / 4 (predicted from the growth between the last two k: 4 per step for an output that is linear
    in the gradient, 1 for what the forward left)."""
    out = {}
    for k in grid:
        if len(out) >= 2:
            k0, k1 = sorted(out)[-2:]
            step = 2.0 ** (k - k1)
            if any(e1.half and e1.refmax * (step if e1.refmax > 1.5 * e0.refmax else 1.0) >= HALF_TOP
                   for e0, e1 in zip(out[k0], out[k1])):
                break
        rec = Recorder()
        run(k, rec)
        if any(e.half and e.refmax >= HALF_TOP for e in rec.entries):   # (the first two points: no growth estimate yet)
            break
        out[k] = rec.entries
    return out


def lowest_holding(table, what=None):
    """The lowest k from which every entry (or the entry `what`) holds its bound at every k up to the top of the sweep."""
    low = None
    for k in sorted(table, reverse=True):
        if all(e.ok for e in table[k] if what is None or e.what == what):
            low = k
        else:
            break
    return low


def report(name, table, window):
    """One line per k: the relative error of every output; printed by the GPU tests, so a run shows where each kernel stops."""
    lines = [f"grad-range {name}: window log2 rms [{window[0]:g}, {window[1]:g}], lowest k holding its bound: {lowest_holding(table)}"]
    for k in sorted(table):
        cells = ", ".join(f"{e.what} {e.rel:.2e}{'' if e.ok else ' !'}{' NaN' if e.nan else ''}" for e in table[k])
        lines.append(f"  k={k:+3d} {'in ' if in_window(k, window) else 'out'} | {cells}")
    return "\n".join(lines)


def assert_sweep(name, table, window, grid=K_GRID):
    inside = [k for k in table if in_window(k, window)]
    assert len(points_in(window, grid)) >= 4, f"{name}: the window {window} holds fewer than 4 points of the grid"
    assert len(inside) >= 4, f"{name}: the sweep reached only {inside} inside the window {window}"
    bad = []
    for k in sorted(table):
        for e in table[k]:
            if e.nan:
                bad.append(f"k={k:+d} {e.what}: NaN where the float64 reference is finite")
            elif in_window(k, window) and not e.ok:
                bad.append(f"k={k:+d} {e.what}: max err / max |ref| = {e.rel:.3e} > {e.tol:.1e}"
                           f"{' (+ 2^-25 absolute)' if e.half else ''}, max |ref| = {e.refmax:.3e}")
    assert not bad, f"{name}, window log2 rms {window}:\n  " + "\n  ".join(bad)


def homogeneous(run, k):
    """Family (a): run at scale 1 and at 2^k; every output whose float64 reference moved with the scale must equal 2^k times
    the scale-1 output bit for bit (scaled in its own storage type), everything else must not have moved at all.  Returns the
    list of differences (empty: homogeneous)."""
    r0, rk = Recorder(keep=True), Recorder(keep=True)
    run(0, r0)
    run(k, rk)
    assert [e.what for e in r0.entries] == [e.what for e in rk.entries]
    s, bad, moved = 2.0 ** k, [], 0
    for e0, e1 in zip(r0.entries, rk.entries):
        lin = (e1.refmax > e0.refmax * s ** 0.5) if k > 0 else (e1.refmax < e0.refmax * s ** 0.5)
        moved += lin
        want = e0.got * s if lin else e0.got
        assert bool(torch.isfinite(want.double()).all()), f"{e0.what}: 2^{k} x the scale-1 output leaves the storage type"
        if not torch.equal(e1.got, want):
            d = e1.got.double() - want.double()
            n = int((e1.got != want).sum())
            bad.append(f"{e0.what}: {n} of {want.numel()} elements differ from {'2^%d x ' % k if lin else ''}the scale-1 output, "
                       f"largest difference {float(d.abs().max()):.3e} at max |output| {float(want.double().abs().max()):.3e}")
    assert moved, "no output moved with the gradient scale: the case scales no gradient operand"
    return bad


# ------------------------------------------------------------------ the hi + lo operand, emulated (tests/test_grad_range_cpu.py) ---
def hilo_product(x, v, dt, hi_only=False):
    """x^T v as lora_grad_mfma_kernel (csrc/lora.hip) and lg_split (csrc/gemm_panel_impl.h) form it: x stored in `dt`, the
    fp32 operand v fed to the matrix cores as hi = dt(v) and lo = dt(v - hi) without any scaling; products and sums exact
    (float64).  dt = float16 keeps half subnormals."""
    xd = x.to(dt).double()
    hi = v.float().to(dt)
    lo = (v.float() - hi.float()).to(dt)
    vv = hi.double() if hi_only else hi.double() + lo.double()
    return xd.t() @ vv
