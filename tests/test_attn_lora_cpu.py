"""Adapters on the ViT attention projections (LoraCfg.targets), everything that needs no GPU: the key set, the float
restatement used as the yardstick of the GPU tests (tests/attn_lora_ref.py) against the UNCHANGED oracle on merged weights,
FedAvg on the new keys, and the kernels the adapted qkv product is routed to (host-side queries of the library alone)."""
import dataclasses
import os

import pytest
import torch

from fairfedmed_amd import _lib as L
from fairfedmed_amd import config as C
from fairfedmed_amd import federated as F
from fairfedmed_amd import ops, synth
from fairfedmed_amd.engine import Switches, Targets, tower_route
from oracle import fairlora_oracle as O
from tests import attn_lora_ref as R


def with_targets(mcfg, targets):
    return dataclasses.replace(mcfg, lora=dataclasses.replace(mcfg.lora, targets=targets))


def rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ keys and counts --
def test_default_targets_is_todays_manifest():
    base = C.vit_b16()
    assert base.lora.targets == "mlp"
    m0, m1 = synth.manifest(base), synth.manifest(with_targets(base, "mlp"))
    assert list(m0.items()) == list(m1.items())
    assert not any(".attn.in_proj_lora." in k or ".attn.out_proj_lora." in k for k in m0)
    sd0, sd1 = synth.make_state_dict(C.vit_tiny()), synth.make_state_dict(with_targets(C.vit_tiny(), "mlp+attn"))
    for k, v in sd0.items():                      # synth keys its values by name: existing tensors keep their values
        assert torch.equal(v, sd1[k]), k


@pytest.mark.parametrize("lora_type,global_s", [("FairLoRA", False), ("FairLoRA", True), ("SVLoRA", True), ("LoRA", False)])
@pytest.mark.parametrize("targets", ["attn", "mlp+attn"])
def test_new_keys_sit_behind_out_proj_bias(targets, lora_type, global_s):
    mcfg = with_targets(C.vit_tiny_lora(lora_type, global_s), targets)
    lo, w = mcfg.lora, mcfg.vision.width
    keys = list(synth.manifest(mcfg))
    shapes = synth.manifest(mcfg)
    s_shape = (lo.num_groups, lo.rank) if lora_type == "FairLoRA" else (lo.rank,)
    for i in range(mcfg.vision.layers):
        p = f"image_encoder.transformer.resblocks.{i}.attn."
        at = keys.index(p + "out_proj.bias") + 1
        want = []
        for site, fout in (("in_proj_lora.", 3 * w), ("out_proj_lora.", w)):
            want.append((p + site + "lora_A.weight", (w, lo.rank)))
            if lora_type != "LoRA":
                want.append((p + site + "lora_S.weight", s_shape))
                if global_s:
                    want.append((p + site + "lora_S_global.weight", (lo.rank,)))
            want.append((p + site + "lora_B.weight", (lo.rank, fout)))
        assert [(k, tuple(shapes[k])) for k in keys[at:at + len(want)]] == want
        assert keys[at + len(want)] == f"image_encoder.transformer.resblocks.{i}.ln_1.weight"
        mlp_keys = [k for k in keys if f"resblocks.{i}.mlp." in k and ".lora_" in k and k.startswith("image_encoder.")]
        assert bool(mlp_keys) == (targets == "mlp+attn")
    # the frozen keys do not move, the text tower carries no adapter, and the new tensors are trainable
    frozen = [k for k in keys if ".lora_" not in k]
    assert frozen == [k for k in synth.manifest(with_targets(mcfg, "mlp")) if ".lora_" not in k]
    assert not any(".lora_" in k for k in keys if k.startswith("text_encoder."))
    assert all(k in synth.trainable_keys(mcfg) for k in keys if "_proj_lora." in k)
    # init as on the MLP sites: A = 0, S 'same+cycle'
    sd = synth.make_state_dict(mcfg, lora_init="reference")
    q = "image_encoder.transformer.resblocks.0.attn.in_proj_lora."
    assert float(sd[q + "lora_A.weight"].abs().max()) == 0.0 and float(sd[q + "lora_B.weight"].std()) > 0.5
    if lora_type == "FairLoRA":
        assert torch.equal(sd[q + "lora_S.weight"], synth.lora_s_init(lo.rank, lo.num_groups))


def test_trainable_counts_vit_b16():
    def count(targets):
        mcfg = with_targets(C.vit_b16(rank=8, num_groups=3), targets)
        m = synth.manifest(mcfg)
        return sum(int(torch.Size(m[k]).numel()) for k in synth.trainable_keys(mcfg))
    assert count("mlp") == 741952
    assert count("mlp+attn") == 1184896
    assert count("attn") == 447040


def test_bad_targets_and_rn_raise():
    with pytest.raises(ValueError):
        C.LoraCfg(targets="qkv")
    for targets in ("attn", "mlp+attn"):
        with pytest.raises(NotImplementedError):
            synth.manifest(with_targets(C.rn_tiny(), targets))
        with pytest.raises(NotImplementedError):
            synth.trainable_keys(with_targets(C.rn50(), targets))
    synth.manifest(with_targets(C.rn_tiny(), "mlp"))


# ----------------------------------------------------------------------------- the helper against the oracle itself --
@pytest.mark.parametrize("targets", ["attn", "mlp+attn"])
def test_helper_equals_oracle_on_merged_weights(targets, tol=1e-5):
    """attr=None gives every sample the same s_bar, so the attention adapters are ONE dense update of in_proj_weight /
    out_proj.weight: the helper on the adapted state dict must equal the unchanged oracle on the merged one, to fp32
    rounding (1e-5).  The oracle does not run in float64 - its layer_norm computes in float32 (`x.float()`) - so there is
    no tighter second case."""
    mcfg = with_targets(C.vit_tiny(rank=4), targets)
    sd = synth.make_state_dict(mcfg, seed=3, lora_init="random")
    merged = R.merged_state_dict(sd, mcfg)
    assert not any("_proj_lora." in k for k in merged)
    img = synth.make_batch(mcfg, 5, seed=11)["img"]
    ref = O.clip_logits(merged, img, None, mcfg)
    with R.adapted_oracle():
        got = O.clip_logits(sd, img, None, mcfg)
    assert O.vision_block is not R.adapted_block            # the substitution ends with the context
    e = rel(got, ref)
    print(targets, "helper vs oracle on merged weights:", e)
    assert e < tol
    # ... and the adapters are not a no-op in this state dict: the plain weights give other logits
    plain = {**merged, **{k: v for k, v in sd.items() if k.endswith(("attn.in_proj_weight", "attn.out_proj.weight"))}}
    assert rel(O.clip_logits(plain, img, None, mcfg), ref) > 1e-4


def test_helper_without_attention_keys_is_the_oracle():
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    batch = synth.make_batch(mcfg, 4, seed=5)
    attr = batch["attrs"].t()[0]
    ref = O.clip_logits(sd, batch["img"], attr, mcfg)
    with R.adapted_oracle():
        got = O.clip_logits(sd, batch["img"], attr, mcfg)
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------------- FedAvg --
@pytest.mark.parametrize("shared_half_s", [False, True])
def test_fedavg_weights_the_new_lora_s_rows_per_group(shared_half_s):
    """w = sum_k (n_k / sum n) w_k, row g of every lora_S [G, r] block sum_k (n_kg / sum_k n_kg) w_k[g], the
    first r/2 columns of such a block replaced by their mean over the groups under shared_half_s, then the EMA
    (1 - b) avg + b w_g with b = beta epoch / max_epoch.  Nothing in it knows the new keys: they carry 'lora_S'."""
    mcfg = with_targets(C.vit_tiny(rank=4), "mlp+attn")
    G, r = mcfg.lora.num_groups, mcfg.lora.rank
    p = "image_encoder.transformer.resblocks.1.attn."
    keys = [p + "in_proj_lora.lora_A.weight", p + "in_proj_lora.lora_S.weight", p + "in_proj_lora.lora_B.weight",
            p + "out_proj_lora.lora_S.weight", p + "out_proj_lora.lora_B.weight", "prompt_learner.ctx"]
    shapes = synth.manifest(mcfg)
    gen = torch.Generator().manual_seed(5)
    w = {u: {k: torch.randn(shapes[k], generator=gen, dtype=torch.float64) for k in keys} for u in range(3)}
    w_g = {k: torch.randn(shapes[k], generator=gen, dtype=torch.float64) for k in keys}
    n = [10, 30, 60]
    n_attr = [[1, 4, 5], [20, 5, 5], [0, 30, 30]]
    epoch, max_epoch, beta = 3, 10, 0.999
    got = F.average_weights_ema(w_g, w, [0, 1, 2], n, n_attr, epoch, max_epoch, beta=beta, shared_half_s=shared_half_s)
    b = beta * epoch / max_epoch
    tot = [sum(col) for col in zip(*n_attr)]
    for k in keys:
        if k.endswith("lora_S.weight"):
            avg = torch.stack([sum(w[u][k][g] * (n_attr[u][g] / tot[g]) for u in range(3)) for g in range(G)])
            if shared_half_s:
                avg = torch.cat([avg[:, :r // 2].mean(0, keepdim=True).expand(G, -1), avg[:, r // 2:]], dim=1)
        else:
            avg = sum(w[u][k] * (n[u] / sum(n)) for u in range(3))
        # (the per-group weights n_kg / sum n_kg are formed in float32 there: 2^-24 each, on values of order one)
        assert torch.allclose(got[k], (1 - b) * avg + b * w_g[k], rtol=1e-6, atol=1e-6), k
    # LOCAL_S personalisation picks the new keys up by name as well
    args = F.FedArgs(num_users=3, idxs_users_train=[1], local_s=True)
    local_s = {1: {k: v + 1 for k, v in w[1].items() if "lora_S" in k}}
    per = F.personalize(got, 1, args, {1: got["prompt_learner.ctx"][args.avg_prompt:args.num_prompt]}, local_s)
    for k in keys:
        assert torch.equal(per[k], local_s[1][k] if "lora_S" in k else got[k]), k


# ------------------------------------------------------------------------------------------------------ routing --
def _panel_override() -> bool:
    return "FFM_PANEL" in os.environ or "FFM_PANEL_MASK" in os.environ


@pytest.mark.parametrize("images", [28, 32])
@pytest.mark.parametrize("lnin", [False, True], ids=["plain", "lnin"])
def test_adapted_qkv_product_runs_on_a_panel_tile(images, lnin):
    """The qkv forward of an adapted ViT-B/16 tower (N = 3 x 768, K = 768, rank 8, bf16, packed weight) has a kernel with and
    without ln_1 folded in.  With the fold - what tower_route chooses at these row counts - it is the panel kernel: without
    the word FFM_EPI_BIAS | FFM_EPI_LORA | FFM_EPI_LNIN of FFM_PANEL_EPI_RK this query answers with an error code, the fold
    is off and the product falls to the 128x128 kernel behind a LayerNorm launch.  Without the fold the product stays on the
    128x128 kernel, which measured level with the panel tile for it: 18 column tiles."""
    if _panel_override():
        return
    flags = L.EPI_BIAS | L.EPI_LORA | L.EPI_RANKOP | (L.EPI_LNIN if lnin else 0)
    rows = images * 197
    assert ops.gemm_tiles_n(rows, 3 * 768, 768, flags, 8, torch.bfloat16, True) > 0
    cfg, bm, bn, _ = ops.gemm_tile_shape(rows, 3 * 768, 768, flags, 8, torch.bfloat16, True)
    if lnin:
        assert cfg >= 0 and (3 * 768) % bn == 0 and (bm, bn) != (128, 128)
    else:
        assert cfg == -1 and ops.gemm_tiles_n(rows, 3 * 768, 768, flags, 8, torch.bfloat16, True) == 18
    # what exists today answers as it did: the plain qkv words and the c_fc word at the same shape
    assert ops.gemm_tile_shape(rows, 3 * 768, 768, L.EPI_BIAS | L.EPI_LNIN, 0, torch.bfloat16, True)[0] == 10
    fc = L.EPI_BIAS | L.EPI_LORA | L.EPI_GELU | L.EPI_RANKOP | L.EPI_LNIN
    assert ops.gemm_tile_shape(rows, 4 * 768, 768, fc, 8, torch.bfloat16, True)[0] == 7


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("images", [28, 32])
def test_adapted_tower_route(images, dtype):
    if _panel_override():
        return
    sw = Switches()
    route = lambda **k: tower_route(768, 12, 197, False, 8, dtype, True, images * 197, sw, **k)
    base = route()
    assert route(targets=Targets()) == base and base.ln1 > 0 and base.ln1_bwd > 0
    both = route(targets=Targets(mlp=True, attn=True))
    # ln_1 and ln_2 stay folded forward, the MLP's backward folds stay, ln_1's backward fold is off (its row sums would
    # miss the adapter's terms)
    assert both == dataclasses.replace(base, ln1_bwd=0)
    att = route(targets=Targets(mlp=False, attn=True))
    assert att.ln1 > 0 and (att.ln2, att.lgrad, att.ln2_bwd, att.ln1_bwd) == (0, 0, 0, 0)
    # fp32 storage and ranks beyond one MFMA tile fold nothing, as for the reference's placement
    assert tower_route(768, 12, 197, False, 24, dtype, True, images * 197, sw, targets=Targets(True, True)).ln1 == 0
    assert tower_route(768, 12, 197, False, 8, torch.float32, False, images * 197, sw, targets=Targets(True, True)).ln1 == 0
