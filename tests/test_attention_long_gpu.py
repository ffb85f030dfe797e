"""Streaming attention beyond 256 tokens (csrc/attention_long.hip) through the two public entry points, against float64.

The kernels keep a 64-query tile resident and stream 64-key tiles (the dK/dV kernel the other way round), so the lengths
below sit on and around multiples of 64 above 256 (319, 320, 321; 383, 384, 385) next to the ViT-B/16 token counts of
272^2 .. 512^2 inputs (290, 442, 577, 785, 1025).  Bounds are those of test_kernels_gpu.py (test_attention_fwd_bwd,
test_attention3_lengths): max error / tensor scale.
"""
import math

import pytest
import torch

from tests.guarded import guard_fixture

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
LENGTHS = [257, 290, 319, 320, 321, 383, 384, 385, 442, 577, 785, 1025]


def tol(dt):
    return 2e-5 if dt == torch.float32 else 1.2e-2 if dt == torch.bfloat16 else 2e-3


def tol_lse(dt):
    return 1e-5 if dt == torch.float32 else 2e-3


def rel_err(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def check(got, ref, t, what):
    e = rel_err(got, ref)
    print(f"{what}: {e:.3e} (bound {t:.1e})")
    assert math.isfinite(e) and e <= t, f"{what}: max err / scale = {e:.3e} > {t:.1e}"


@pytest.fixture(scope="module")
def ops():
    from fairfedmed_amd import ops
    return ops


def rnd(*shape, dt=torch.float32, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dt)


def ref_attention(qkv, B, L, heads, causal):
    E = heads * 64
    q, k, v = qkv.double().reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    if causal:
        s = s + torch.full((L, L), float("-inf"), device=qkv.device, dtype=torch.float64).triu_(1)
    p = torch.softmax(s, -1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B * L, E)
    return o, torch.logsumexp(s, -1)


@pytest.fixture
def guard():
    """Every kernel output of this file: poisoned body between two guard bands (tests/guarded.py); unchecked at teardown = failure."""
    yield from guard_fixture()


def run(ops, guard, qkv, dout, B, L, heads, causal, with_lse=True):
    """forward + backward into poisoned, guarded outputs: (out, lse, dqkv); lse is None for a forward without it"""
    E = heads * 64
    out = guard.out(B * L, E, dtype=qkv.dtype, name="out")
    lse = guard.out(B, heads, L, name="lse") if with_lse else None
    ops.attention_fwd(qkv, out, lse, B, L, heads, causal)
    if dout is None:
        guard.check()
        return out, lse, None
    dqkv = guard.out(B * L, 3 * E, dtype=qkv.dtype, name="dqkv")
    delta = guard.scratch(B, heads, L, name="delta")                  # (scratch by the header: bands only)
    ops.attention_bwd(qkv, out, dout, lse, delta, dqkv, B, L, heads, causal)
    guard.check()
    return out, lse, dqkv


def fwd_bwd_against_float64(ops, guard, dt, B, L, heads, causal):
    E = heads * 64
    qkv = rnd(B * L, 3 * E, dt=dt, seed=23 + L)
    dout = rnd(B * L, E, dt=dt, seed=24 + L)
    out, lse, dqkv = run(ops, guard, qkv, dout, B, L, heads, causal)
    qd = qkv.double().requires_grad_(True)
    ref, ref_lse = ref_attention(qd, B, L, heads, causal)
    ref.backward(dout.double())
    check(out, ref.detach(), tol(dt), "attn out")
    check(lse, ref_lse.detach(), tol_lse(dt), "lse")
    t = tol(dt) * (1 if dt == torch.float32 else 2)
    check(dqkv[:, :E], qd.grad[:, :E], t, "dq")
    check(dqkv[:, E:2 * E], qd.grad[:, E:2 * E], t, "dk")
    check(dqkv[:, 2 * E:], qd.grad[:, 2 * E:], t, "dv")


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("L", LENGTHS)
def test_long_lengths(ops, guard, dt, L):
    fwd_bwd_against_float64(ops, guard, dt, 2, L, 3, False)


def test_long_grid_not_a_power_of_two(ops, guard):
    fwd_bwd_against_float64(ops, guard, torch.bfloat16, 3, 577, 5, False)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("B,L,heads", [(1, 300, 2), (2, 513, 1)])
def test_long_causal(ops, guard, dt, B, L, heads):
    fwd_bwd_against_float64(ops, guard, dt, B, L, heads, True)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_long_forward_without_lse_gives_the_same_bits(ops, guard, dt, causal):
    B, L, heads = 2, 321, 3
    qkv = rnd(B * L, 3 * heads * 64, dt=dt, seed=31)
    a, _, _ = run(ops, guard, qkv, None, B, L, heads, causal, with_lse=True)
    b, _, _ = run(ops, guard, qkv, None, B, L, heads, causal, with_lse=False)
    assert bool(torch.isfinite(a.float()).all())
    assert torch.equal(a, b)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_long_online_softmax_rows(ops, guard, dt):
    """Three rows through the three ways a running maximum can move over the ten key tiles of L = 577: raised by the very
    last tile (one rescale of everything before), set by the first tile (never rescaled), and raised by every tile.
    Per-row comparison so that one wrong row cannot hide."""
    B, heads, L = 2, 3, 577
    E = heads * 64
    qkv = rnd(B * L, 3 * E, dt=dt, seed=77, scale=0.5)
    v = qkv.view(B, L, 3, heads, 64)
    v[0, 5, 0, 1] = 2.0                                    # query 5 of head 1 ...
    v[0, L - 1, 1, 1] = 3.0                                # ... against the only key of the last tile: score 384 / 8
    v[1, 40, 0, 2] = -2.0
    v[1, 3, 1, 2] = -3.0                                   # query 40 of head 2 peaks at key 3 (first tile)
    v[1, 7, 0, 0] = 0.5                                    # query 7 of head 0: score 0.04 j + noise of 0.25, 2.56 per tile
    v[1, :, 1, 0] += (0.01 * torch.arange(L, device="cuda"))[:, None].to(dt)
    out, lse, _ = run(ops, guard, qkv, None, B, L, heads, False)
    ref, ref_lse = ref_attention(qkv.double(), B, L, heads, False)
    err = (out.double() - ref).abs().reshape(B, L, heads, 64).amax(-1)
    print("out", float(err.max()) / float(ref.abs().max()), "lse", float((lse.double() - ref_lse).abs().max()) / float(ref_lse.abs().max()))
    assert float(err.max()) <= tol(dt) * float(ref.abs().max()), (float(err.max()), err.argmax())
    assert float((lse.double() - ref_lse).abs().max()) <= tol_lse(dt) * float(ref_lse.abs().max())
    assert float(lse[0, 1, 5]) > 40.0                      # the spike really is the row maximum
    assert float(lse[1, 2, 40]) > 40.0
    s7 = (qkv.double().view(B, L, 3, heads, 64)[1, 7, 0, 0] * qkv.double().view(B, L, 3, heads, 64)[1, :, 1, 0]).sum(-1) * 0.125
    tile_max = torch.nn.functional.pad(s7, (0, 64 * 10 - L), value=float("-inf")).view(10, 64).amax(-1)
    assert bool((tile_max[1:9] > tile_max[:8]).all()), "the rising row does not raise its maximum in every full tile"


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_long_propagates_non_finite_inputs(ops, guard, dt, bad):
    """The step's only divergence guard is the finite flag ce_loss raises from the logits: a NaN / Inf in q, k or v must
    come out of the attention output (and one in dO out of dq, dk, dv), not be folded away by a running maximum, a rescale
    or a mask select - and must stay inside its (batch, head) pair."""
    B, heads, L = 2, 3, 300
    E = heads * 64
    b, h = 1, 2                                                   # the (batch, head) pair that is poisoned
    rows = slice(b * L, (b + 1) * L)
    for which, row in (("q", 5), ("k", 100), ("v", 299)):
        qkv = rnd(B * L, 3 * E, dt=dt, seed=250)
        col = {"q": 0, "k": E, "v": 2 * E}[which] + h * 64 + 7
        qkv[b * L + row, col] = bad
        out, _, _ = run(ops, guard, qkv, None, B, L, heads, False)
        o = out[rows, h * 64:(h + 1) * 64].float()
        hit = ~torch.isfinite(o).all(dim=1)
        if which == "q":
            assert bool(hit[row]), (which, "the poisoned query's output row is finite")
            assert int(hit.sum()) == 1, (which, int(hit.sum()), "other queries of the pair are hit")
        elif which == "k" and bad == float("inf"):
            # q . k = +inf where the query's element is positive (inf - inf in the softmax), -inf elsewhere: that key then
            # simply carries no weight, and the row is finite in exact arithmetic too
            pos = qkv[rows, h * 64 + 7].float() > 0
            assert bool(hit[pos].all()) and int(pos.sum()) > 0, (which, int(hit.sum()), int(pos.sum()))
        else:
            assert bool(hit.all()), (which, int(hit.sum()), "every query of the pair sees the poisoned key / value")
        out[rows, h * 64:(h + 1) * 64] = 0                        # everything outside the pair stays finite
        assert bool(torch.isfinite(out.float()).all())
    qkv = rnd(B * L, 3 * E, dt=dt, seed=251)
    dout = rnd(B * L, E, dt=dt, seed=252)
    dout[b * L + 11, h * 64 + 3] = bad
    _, _, dqkv = run(ops, guard, qkv, dout, B, L, heads, False)
    dq = dqkv[rows, h * 64:(h + 1) * 64].float()
    dk = dqkv[rows, E + h * 64:E + (h + 1) * 64].float()
    dv = dqkv[rows, 2 * E + h * 64:2 * E + (h + 1) * 64].float()
    assert not bool(torch.isfinite(dq[11]).all()), "dq of the poisoned row"
    assert bool(torch.isfinite(torch.cat([dq[:11], dq[12:]])).all()), "dq of another row"
    assert not bool(torch.isfinite(dk).all()) and not bool(torch.isfinite(dv).all()), "dk / dv of the pair"
    for part in range(3):
        dqkv[rows, part * E + h * 64:part * E + (h + 1) * 64] = 0
    assert bool(torch.isfinite(dqkv.float()).all()), "outside the pair"


def test_long_bitwise_repeatable_and_independent_of_the_grid(ops, guard):
    """No atomics and no sum across workgroups: three runs give the same bits, and so does the same batch as the first
    half of a batch twice as large (twice the grid)."""
    dt, B, L, heads = torch.bfloat16, 4, 577, 6
    E = heads * 64
    qkv = rnd(B * L, 3 * E, dt=dt, seed=901)
    dout = rnd(B * L, E, dt=dt, seed=902)
    first = run(ops, guard, qkv, dout, B, L, heads, False)
    assert all(bool(torch.isfinite(t.float()).all()) for t in first)
    for _ in range(2):
        again = run(ops, guard, qkv, dout, B, L, heads, False)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    twice = run(ops, guard, qkv.repeat(2, 1), dout.repeat(2, 1), 2 * B, L, heads, False)
    assert torch.equal(twice[0][:B * L], first[0])
    assert torch.equal(twice[1][:B], first[1])
    assert torch.equal(twice[2][:B * L], first[2])
    assert torch.equal(twice[0][B * L:], first[0]) and torch.equal(twice[2][B * L:], first[2])
