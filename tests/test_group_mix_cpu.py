"""The per-sample group mix pi_b of the oracle (oracle.fairlora_oracle.group_mix) for attribute values outside [0, G).

The reference (trainers/GLP_OT_SVLoRA.py:453-462) raises in F.one_hot on such a value; the project defines it as
"unknown" -> the uniform 1/G of `attr is None`, and the HIP kernels are held to this oracle
(tests/test_group_mix_gpu.py).  For valid attributes the reference's expression must not move by one bit."""
import pytest
import torch
import torch.nn.functional as F

from fairfedmed_amd import config as C
from fairfedmed_amd import synth
from oracle import fairlora_oracle as O


def pattern(G):
    """The fixed attribute pattern of the GPU tests: valid values and the unknown ones {-2, -1, G, G + 1}."""
    return torch.tensor([0, -1, G - 1, G, 1, -2, 0, G + 1, 1], dtype=torch.int64)


def reference_expression(attr, G, lam, dtype):
    """The expression group_mix had before it learnt about unknown values (the reference's own)."""
    onehot = F.one_hot(attr.long(), num_classes=G).to(dtype)
    return onehot * lam + (1 - onehot) * (1 - lam) / (G - 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("G", [2, 3, 8])
@pytest.mark.parametrize("lam", [0.7, 0.55])
def test_valid_attributes_are_bit_identical_to_the_reference_expression(G, lam, dtype):
    attr = torch.arange(5 * G) % G
    got = O.group_mix(attr, G, lam, dtype=dtype)
    assert got.dtype == dtype and torch.equal(got, reference_expression(attr, G, lam, dtype))
    got32 = O.group_mix(attr.to(torch.int32), G, lam, dtype=dtype)
    assert torch.equal(got32, got)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("G", [2, 3, 8])
def test_unknown_rows_are_exactly_uniform_and_the_valid_rows_do_not_move(G, dtype):
    attr = pattern(G)
    known = (attr >= 0) & (attr < G)
    assert int(known.sum()) == 5 and int((~known).sum()) == 4
    pi = O.group_mix(attr, G, dtype=dtype)
    assert pi.shape == (9, G) and pi.dtype == dtype
    uni = torch.full((G,), 1.0 / G, dtype=dtype)
    for b in range(9):
        if known[b]:
            assert torch.equal(pi[b], reference_expression(attr[b:b + 1], G, 0.7, dtype)[0]), (b, int(attr[b]))
        else:
            assert torch.equal(pi[b], uni), (b, int(attr[b]))


@pytest.mark.parametrize("G", [2, 3, 8])
def test_every_row_sums_to_one(G):
    pi = O.group_mix(pattern(G), G, dtype=torch.float64)
    assert float((pi.sum(1) - 1.0).abs().max()) <= 1e-15


@pytest.mark.parametrize("G", [2, 3, 8])
@pytest.mark.parametrize("value", ["-1", "-2", "G", "G+1"])
def test_an_all_unknown_vector_is_the_no_attribute_mix(G, value):
    v = {"-1": -1, "-2": -2, "G": G, "G+1": G + 1}[value]
    attr = torch.full((6,), v, dtype=torch.int64)
    for dtype in (torch.float32, torch.float64):
        none = O.group_mix(None, G, dtype=dtype)
        assert torch.equal(O.group_mix(attr, G, dtype=dtype), none.expand(6, G))


def test_hand_backward_with_a_mixed_attribute_vector_matches_autograd():
    """fairlora_backward (which builds its own pi through group_mix) against float64 autograd through fairlora_linear."""
    G, r, L, Bn, din, dout = 3, 4, 5, 9, 16, 12
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, W, b, A, S, Bm = rn(L, Bn, din), rn(dout, din), rn(dout), rn(din, r), rn(G, r), rn(r, dout)
    attr = pattern(G)
    leaves = [t.clone().requires_grad_(True) for t in (x, A, S, Bm)]
    y = O.fairlora_linear(leaves[0], W, b, leaves[1], leaves[2], leaves[3], attr, 0.25)
    gy = rn(L, Bn, dout)
    (y * gy).sum().backward()
    dx, dA, dS, dB = O.fairlora_backward(x, gy, W, A, S, Bm, attr, 0.25)
    for got, leaf, name in zip((dx, dA, dS, dB), leaves, ("dx", "dA", "dS", "dB")):
        assert float((got - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max()), name


def test_loss_and_grads_with_a_mixed_attribute_vector_matches_float64_autograd():
    """The whole oracle step (fp32) on a batch whose attribute column holds the mixed pattern, against float64 autograd
    through a ViT block chain whose FairLoRA layers are fairlora_linear with s_b = pi S built HERE from the rule
    (uniform rows for the unknown samples) - not through group_mix."""
    mcfg = C.vit_tiny(rank=4, num_groups=3)
    G = 3
    sd = synth.make_state_dict(mcfg, seed=5, lora_init="random")
    batch = synth.make_batch(mcfg, 9, seed=21)
    attr = pattern(G)
    batch["attrs"] = attr[:, None].clone()
    keys = synth.trainable_keys(mcfg)
    loss, logits, grads = O.loss_and_grads(sd, batch, mcfg, keys)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(logits).all())

    # the same step in float64 with the mix stated independently: each FairLoRA layer gets S_eff = S and a per-sample
    # mix matrix; a valid sample is passed through as its attribute, an unknown sample as "no attribute" by replacing
    # the layer's mix with hand-built rows
    pi = torch.empty(9, G, dtype=torch.float64)
    for b_, a in enumerate(attr.tolist()):
        pi[b_] = torch.tensor([0.7 if g_ == a else 0.3 / (G - 1) for g_ in range(G)]) if 0 <= a < G else 1.0 / G
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    leaves = {k: sd64[k].clone().requires_grad_(True) for k in keys}
    work = dict(sd64, **leaves)
    orig = O.group_mix, O.layer_norm
    try:
        O.group_mix = lambda attr_, num_groups, lambda_group=0.7, dtype=torch.float32: pi.to(dtype)
        O.layer_norm = lambda x, w, b: F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)      # (the oracle's computes in fp32)
        out = O.clip_logits(work, batch["img"].double(), attr, mcfg)
    finally:
        O.group_mix, O.layer_norm = orig
    loss64 = F.cross_entropy(out, batch["label"])
    loss64.backward()
    l64 = float(loss64.detach())
    assert abs(float(loss) - l64) <= 1e-5 * abs(l64)
    assert float((logits.double() - out.detach()).abs().max()) <= 1e-5 * float(out.detach().abs().max())
    for k in keys:
        ref = leaves[k].grad if leaves[k].grad is not None else torch.zeros_like(leaves[k])
        scale = float(ref.abs().max())
        if scale == 0.0:
            assert float(grads[k].abs().max()) == 0.0, k
        else:
            assert float((grads[k].double() - ref).abs().max()) <= 2e-4 * scale, k
