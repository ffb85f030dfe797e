"""The flat-buffer optimizer kernels of csrc/optim.hip through the C ABI, against plain references of the same operation.

SGD: every entry point (ffm_sgd_momentum_n, ffm_sgd_momentum_gated on a good step, ffm_sgd_momentum_dev) against ONE
float64 restatement of torch.optim.SGD (dampening 0, no Nesterov) applied `repeats` times to the same gradient, and against
torch.optim.SGD itself in float32 stepped `repeats` times.  Bound: max |error| <= 1e-6 of the tensor's scale (max |ref|), as
tests/test_kernels_gpu.py::test_sgd_matches_torch holds it; the three entry points must agree BIT for bit (the eager step,
its recorded plan and the captured graph train alike).  Sizes either side of 524 288 = 2048 x 256 threads (grid_for's cap)
run the grid-stride tail.

fp16 gradient scale (include/ffm_hip.h, ffm_loss_scale): loss_scale / unscale_check / scale_check bit for bit against the
float32 products, their overflow detection at the lane and wave edges, and the 8-float state machine against a numpy
float32 model, word for word after every step.
"""
import numpy as np
import pytest
import torch

from fairfedmed_amd import _lib as L
from fairfedmed_amd import config as C
from fairfedmed_amd import ops
from fairfedmed_amd.engine import FlatParams

pytestmark = pytest.mark.gpu

GRID_CAP = 2048 * 256                     # grid_for(n): at most 2048 blocks of 256 threads, then grid-stride
VITB_N = FlatParams(C.vit_b16(rank=8, num_groups=3), "cpu").numel   # the real trainable buffer of ViT-B/16 r=8 G=3
SIZES = [1, 255, 257, GRID_CAP - 1, GRID_CAP + 1, VITB_N]
LR = 1e-2
TOL = 1e-6                                 # max |error| / max |ref|
FLT_MAX = float(np.finfo(np.float32).max)


def f32(x: float) -> float:
    """The value a float hyper-parameter has once the kernel receives it."""
    return float(np.float32(x))


def rnd(n, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, device="cuda", generator=g) * scale


def rel_err(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def sgd_ref(p, g, buf, lr, mu, wd, first, repeats):
    """torch.optim.SGD.step() `repeats` times on one gradient, in float64: d = g + wd p; b = d on the first application of
    a first step, mu b + d otherwise; p -= lr b."""
    p, g, b = p.double(), g.double(), buf.double()
    lr, mu, wd = f32(lr), f32(mu), f32(wd)
    for k in range(repeats):
        d = g + wd * p
        b = d.clone() if (first and k == 0) else mu * b + d
        p = p - lr * b
    return p, b


def sgd_torch(p, g, buf, lr, mu, wd, first, repeats):
    """torch.optim.SGD in float32, stepped `repeats` times (momentum buffer seeded with buf unless it is a first step)."""
    q = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([q], lr=lr, momentum=mu, weight_decay=wd)
    if mu != 0 and not first:
        opt.state[q]["momentum_buffer"] = buf.clone()
    for _ in range(repeats):
        q.grad = g.clone()
        opt.step()
    return q.detach()


def good_state(scale=1024.0):
    return torch.tensor([scale, 1.0 / scale, 1.0, 0.0, 0.0, 65536.0, 2000.0, 1.0], device="cuda")


def run_sgd(entry, p, g, buf, lr, mu, wd, first, repeats, state=None):
    """One call of an SGD entry point, in place on p / buf.  For `dev`, a first step is a zeroed buf."""
    if entry == "n":
        ops._call("ffm_sgd_momentum_n", L.ptr(p), L.ptr(g), L.ptr(buf), p.numel(), lr, mu, wd, int(first), int(repeats),
                  L.stream_ptr())
    elif entry == "gated":
        ops.sgd_momentum_gated(p, g, buf, lr, mu, wd, first, repeats, good_state() if state is None else state)
    else:
        if first:
            buf.zero_()
        hp = torch.tensor([lr, mu, wd], device="cuda")
        ops.sgd_momentum_dev(p, g, buf, hp, repeats, state)


def inputs(n, seed):
    return rnd(n, seed), rnd(n, seed + 1), rnd(n, seed + 2, 0.5)


SGD_GRID = [pytest.mark.parametrize("wd", [0.0, 5e-4], ids=["wd0", "wd5e-4"]),
            pytest.mark.parametrize("mu", [0.0, 0.9], ids=["mu0", "mu0.9"]),
            pytest.mark.parametrize("first", [True, False], ids=["first", "later"]),
            pytest.mark.parametrize("repeats", [1, 2, 3, 16]),
            pytest.mark.parametrize("n", SIZES)]


def sgd_grid(f):
    for m in SGD_GRID:
        f = m(f)
    return f


# ------------------------------------------------------------------------------------------------------------- SGD ---
@sgd_grid
@pytest.mark.parametrize("entry", ["n", "gated", "dev"])
def test_sgd_entry_point_matches_float64_and_torch(entry, n, repeats, first, mu, wd):
    p0, g, b0 = inputs(n, seed=n % 1000 + 7 * repeats)
    p, buf = p0.clone(), b0.clone()
    run_sgd(entry, p, g, buf, LR, mu, wd, first, repeats)
    ref_p, ref_b = sgd_ref(p0, g, b0, LR, mu, wd, first, repeats)
    e_p, e_b = rel_err(p, ref_p), rel_err(buf, ref_b)
    assert e_p <= TOL and e_b <= TOL, f"{entry}: p err {e_p:.2e}, buf err {e_b:.2e} > {TOL:.0e} of the scale (float64 ref)"
    e_t = rel_err(p, sgd_torch(p0, g, b0, LR, mu, wd, first, repeats))
    assert e_t <= TOL, f"{entry}: p err {e_t:.2e} > {TOL:.0e} of the scale (torch.optim.SGD, float32)"


@sgd_grid
def test_sgd_entry_points_agree_bit_for_bit(n, repeats, first, mu, wd):
    p0, g, b0 = inputs(n, seed=n % 1000 + 11 * repeats)
    res = {}
    for entry in ("n", "gated", "dev"):
        p, buf = p0.clone(), b0.clone()
        run_sgd(entry, p, g, buf, LR, mu, wd, first, repeats)
        res[entry] = (p, buf)
    for entry in ("gated", "dev"):
        assert torch.equal(res[entry][0], res["n"][0]), f"p of {entry} differs from ffm_sgd_momentum_n"
        assert torch.equal(res[entry][1], res["n"][1]), f"buf of {entry} differs from ffm_sgd_momentum_n"
    if repeats == 1:                              # ffm_sgd_momentum, the eager engine's repeats=1 path
        p, buf = p0.clone(), b0.clone()
        ops.sgd_momentum(p, g, buf, LR, mu, wd, first, 1)
        assert torch.equal(p, res["n"][0]) and torch.equal(buf, res["n"][1])


@pytest.mark.parametrize("repeats", [0, 17, -1])
@pytest.mark.parametrize("entry", ["n", "gated", "dev"])
def test_sgd_repeats_out_of_range_is_einval_and_runs_nothing(entry, repeats):
    n = 1000
    p0, g, b0 = inputs(n, seed=3)
    p, buf, st = p0.clone(), b0.clone(), good_state()
    st0 = st.clone()
    with pytest.raises(RuntimeError, match="invalid argument"):
        run_sgd(entry, p, g, buf, LR, 0.9, 5e-4, False, repeats, state=st if entry != "n" else None)
    torch.cuda.synchronize()
    assert torch.equal(p, p0) and torch.equal(buf, b0) and torch.equal(st, st0)


@pytest.mark.parametrize("entry,first", [("gated", True), ("gated", False), ("dev", False)],
                         ids=["gated-first", "gated-later", "dev"])
def test_gated_sgd_skips_an_overflowed_step_bitwise(entry, first):
    """state[2] == 0: p and buf stay bitwise as they were - with first=1 too (buf is NOT zeroed) - and only the scale moves."""
    n = GRID_CAP + 3
    p0, g, b0 = inputs(n, seed=5)
    p, buf = p0.clone(), b0.clone()
    st = good_state(4096.0)
    st[2] = 0.0
    want = scale_model(st.cpu().numpy())
    if entry == "gated":
        ops.sgd_momentum_gated(p, g, buf, LR, 0.9, 5e-4, first, 2, st)
    else:                                         # the captured step zeroes buf once, at capture: never here
        ops.sgd_momentum_dev(p, g, buf, torch.tensor([LR, 0.9, 5e-4], device="cuda"), 2, st)
    torch.cuda.synchronize()
    assert torch.equal(p, p0) and torch.equal(buf, b0)
    assert np.array_equal(st.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_sgd_dev_without_state_moves_nothing_else():
    """state NULL: ungated (runs whatever a flag elsewhere says) and no scale update follows."""
    n = 4099
    p0, g, b0 = inputs(n, seed=9)
    p, buf = p0.clone(), b0.clone()
    ops.sgd_momentum_dev(p, g, buf, torch.tensor([LR, 0.9, 5e-4], device="cuda"), 3, None)
    ref_p, ref_b = sgd_ref(p0, g, b0, LR, 0.9, 5e-4, False, 3)
    assert rel_err(p, ref_p) <= TOL and rel_err(buf, ref_b) <= TOL


# ---------------------------------------------------------------------------------------------- fp16 gradient scale ---
def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(got, ref):
    """Bit for bit, except that a NaN only has to stay a NaN (its payload is the hardware's business)."""
    nan = torch.isnan(ref)
    return torch.equal(torch.isnan(got), nan) and torch.equal(bits(got)[~nan], bits(ref)[~nan])


@pytest.mark.parametrize("scale", [2.0 ** -3, 1.0, 2.0 ** 12, 2.0 ** 30])
@pytest.mark.parametrize("n", [1, 255, 257, GRID_CAP + 1])
@pytest.mark.parametrize("ok", [0.0, 1.0])
def test_loss_scale_is_the_float32_product_and_marks_the_step_good(n, scale, ok):
    p0 = rnd(n, seed=n + 1)
    p = p0.clone()
    st = torch.tensor([scale, 1.0 / scale, ok, 5.0, 3.0, 65536.0, 2000.0, 0.25], device="cuda")
    st0 = st.clone()
    ops.loss_scale(p, st)
    torch.cuda.synchronize()
    assert torch.equal(bits(p), bits(p0 * scale))
    assert float(st[2]) == 1.0
    keep = [0, 1, 3, 4, 5, 6, 7]
    assert torch.equal(bits(st[keep]), bits(st0[keep])), "loss_scale wrote a state word other than ok"


N_ODD = GRID_CAP + 301                     # not a multiple of 256, past the grid cap
BAD_AT = [0, 63, 64, N_ODD - 1, GRID_CAP + 77]
BAD = [float("inf"), float("-inf"), float("nan")]
BAD_IDS = ["inf", "-inf", "nan"]


def harmless(n):
    """FLT_MAX (times 1.0 stays finite), subnormals and -0.0 scattered over the lanes and the tail: never an overflow."""
    g = rnd(n, seed=21)
    sub = float(np.finfo(np.float32).smallest_subnormal)
    for i, v in ((0, FLT_MAX), (63, -FLT_MAX), (64, sub), (65, -sub), (127, 3 * sub), (n - 1, -0.0),
                 (GRID_CAP + 5, FLT_MAX), (GRID_CAP + 6, -0.0), (n - 2, sub)):
        g[i] = v
    return g


def unscale_state(inv=1.0, ok=1.0):
    return torch.tensor([1.0 / inv, inv, ok, 0.0, 0.0, 65536.0, 2000.0, 1.0], device="cuda")


@pytest.mark.parametrize("inv", [1.0, 2.0 ** -12, 0.375])
def test_unscale_check_is_the_float32_product(inv):
    g0 = harmless(N_ODD)
    g = g0.clone()
    st = unscale_state(inv)
    ops.unscale_check(g, st)
    torch.cuda.synchronize()
    assert torch.equal(bits(g), bits(g0 * inv))
    if inv == 1.0:
        assert float(st[2]) == 1.0, "FLT_MAX, subnormals or -0.0 were taken for an overflow"


@pytest.mark.parametrize("bad", BAD, ids=BAD_IDS)
@pytest.mark.parametrize("at", BAD_AT)
def test_unscale_check_clears_ok_on_a_single_non_finite_value(at, bad):
    g = harmless(N_ODD)
    g[at] = bad
    st = unscale_state(2.0 ** -12)
    st0 = st.clone()
    ops.unscale_check(g, st)
    torch.cuda.synchronize()
    assert float(st[2]) == 0.0, f"{bad} at {at} of {N_ODD} not detected"
    keep = [0, 1, 3, 4, 5, 6, 7]
    assert torch.equal(bits(st[keep]), bits(st0[keep]))


def test_unscale_check_detects_a_product_that_overflows_and_never_sets_ok():
    g = harmless(N_ODD)
    g[GRID_CAP + 9] = 2.0e38                       # finite, but 2e38 * 2 is not
    st = unscale_state(2.0)
    ops.unscale_check(g, st)
    torch.cuda.synchronize()
    assert float(st[2]) == 0.0
    st = unscale_state(1.0, ok=0.0)                # a clean gradient does not undo an earlier overflow mark
    ops.unscale_check(harmless(N_ODD), st)
    torch.cuda.synchronize()
    assert float(st[2]) == 0.0


@pytest.mark.parametrize("bad", BAD, ids=BAD_IDS)
@pytest.mark.parametrize("at", BAD_AT)
@pytest.mark.parametrize("flag", [False, True], ids=["null_flag", "flag"])
def test_scale_check_detection(flag, at, bad):
    g0 = harmless(N_ODD)
    g0[at] = bad
    g = g0.clone()
    fin = torch.ones(1, device="cuda", dtype=torch.int32) if flag else None
    ops.scale_check(g, 0.5, fin)
    torch.cuda.synchronize()
    assert same_bits(g, g0 * 0.5)
    if flag:
        assert int(fin) == 0, f"{bad} at {at} of {N_ODD} not detected"


@pytest.mark.parametrize("flag", [False, True], ids=["null_flag", "flag"])
def test_scale_check_leaves_finite_values_alone(flag):
    g0 = harmless(N_ODD)
    g = g0.clone()
    fin = torch.ones(1, device="cuda", dtype=torch.int32) if flag else None
    ops.scale_check(g, 1.0, fin)
    torch.cuda.synchronize()
    assert torch.equal(bits(g), bits(g0))
    if flag:
        assert int(fin) == 1, "FLT_MAX, subnormals or -0.0 were taken for an overflow"
        fin.zero_()                                # and the flag is never set back
        ops.scale_check(g, 1.0, fin)
        torch.cuda.synchronize()
        assert int(fin) == 0


# --------------------------------------------------------------------------------- the gradient-scale state machine ---
def scale_model(st):
    """scale_update_kernel (csrc/optim.hip) in numpy float32: st = {scale, 1/scale, ok, good_run, overflows, max_scale,
    growth_interval, min_scale}."""
    st = np.array(st, dtype=np.float32)
    one, half, two = np.float32(1), np.float32(0.5), np.float32(2)
    sc = st[0]
    if st[2] == 0:
        sc = max(sc * half, st[7])
        st[3] = 0
        st[4] += one
    else:
        st[3] += one
        if st[6] > 0 and st[3] >= st[6] and sc < st[5]:
            sc = min(sc * two, st[5])
            st[3] = 0
    st[0] = sc
    st[1] = one / sc
    return st


# (initial scale, max_scale, growth_interval, min_scale, overflow pattern over 60 steps)
SCENARIOS = {
    "growth_every_3_to_the_cap": (2.0 ** 10, 2.0 ** 16, 3.0, 1.0, [s in (4, 5, 30, 31, 32, 45) for s in range(60)]),
    "cap_not_a_power_of_two": (2.0 ** 10, 3000.0, 2.0, 1.0, [s in (9, 20, 21, 40) for s in range(60)]),
    "no_growth_at_interval_0": (2.0 ** 12, 2.0 ** 12, 0.0, 1.0, [s % 7 == 3 for s in range(60)]),
    "floor_at_min_scale": (2.0 ** 8, 2.0 ** 8, 3.0, 4.0, [s < 25 or 40 <= s < 50 for s in range(60)]),
}


@pytest.mark.parametrize("entry", ["gated", "dev"])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scale_state_machine_against_a_float32_model(name, entry):
    """One step = loss_scale on a small buffer, unscale_check on a gradient with or without an inf, the gated SGD update;
    the 8 state words must equal the model's bit for bit after every step, and the weights move exactly on the good steps."""
    s0, smax, gi, smin, pattern = SCENARIOS[name]
    st = torch.tensor([s0, 1.0 / s0, 1.0, 0.0, 0.0, smax, gi, smin], device="cuda")
    model = st.cpu().numpy()
    n = 1000
    p, buf = rnd(n, seed=1), torch.zeros(n, device="cuda")
    hp = torch.tensor([LR, 0.9, 5e-4], device="cuda")
    dl0 = rnd(64, seed=2)
    scales, runs = [float(model[0])], []
    for step, overflow in enumerate(pattern):
        dl = dl0.clone()
        ops.loss_scale(dl, st)
        g = rnd(n, seed=100 + step)
        if overflow:
            g[(step * 37) % n] = float("inf")
        before = p.clone()
        ops.unscale_check(g, st)
        if entry == "gated":
            ops.sgd_momentum_gated(p, g, buf, LR, 0.9, 5e-4, False, 2, st)
        else:
            ops.sgd_momentum_dev(p, g, buf, hp, 2, st)
        torch.cuda.synchronize()
        want_dl = dl0 * float(model[0])
        model[2] = 0.0 if overflow else 1.0
        model = scale_model(model)
        got = st.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), model.view(np.uint32)), (step, got.tolist(), model.tolist())
        assert torch.equal(bits(dl), bits(want_dl)), step
        assert torch.equal(p, before) == overflow, step
        scales.append(float(got[0]))
        runs.append(float(got[3]))
    grew = any(b > a for a, b in zip(scales, scales[1:]))
    if name == "growth_every_3_to_the_cap":
        assert grew and max(scales) == smax
    elif name == "cap_not_a_power_of_two":
        assert max(scales) == 3000.0 and scales[-1] == 3000.0
    elif name == "no_growth_at_interval_0":
        assert not grew and scales[-1] < s0 and max(runs) == 6     # six good steps between overflows, never a doubling
    else:                                          # repeated overflow: the scale rests on min_scale, the count goes on
        at_floor = [i for i, ovf in enumerate(pattern) if ovf and scales[i] == smin == scales[i + 1]]
        assert len(at_floor) >= 10 and float(st[4]) == sum(pattern)
    assert bool(torch.isfinite(p).all())
