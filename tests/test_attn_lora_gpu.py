"""Adapters on the ViT attention projections (LoraCfg.targets 'attn' / 'mlp+attn') through the HIP engine.

The reference has no such placement, so nothing here is a golden of it.  The yardstick is tests/attn_lora_ref.py - the
adapted block written with the oracle's own pieces and itself held to the unchanged oracle on merged weights
(tests/test_attn_lora_cpu.py) - and, independently of it, a default-targets ENGINE on merged weights (test 4).  The bounds
are those of tests/test_engine_gpu.py for the same arithmetic on the MLP sites."""
import dataclasses
from collections import Counter
from types import SimpleNamespace as NS

import pytest
import torch

from fairfedmed_amd import _lib as L
from fairfedmed_amd import config as C
from fairfedmed_amd import synth
from oracle import fairlora_oracle as O
from tests import attn_lora_ref as R
from tests.test_attn_lora_cpu import with_targets
from tests.test_route_cpu import panel_override

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ATTN_SITES = ("attn.in_proj_lora.", "attn.out_proj_lora.")


def cos(got, ref):
    got, ref = torch.as_tensor(got).double().cpu().flatten(), torch.as_tensor(ref).double().cpu().flatten()
    return float(torch.dot(got, ref) / (got.norm() * ref.norm()).clamp_min(1e-300))


def rel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def make_engine(mcfg, sd, dtype, max_images, **kw):
    from fairfedmed_amd.engine import FairLoRAEngine
    return FairLoRAEngine(mcfg, sd, dtype=dtype, max_images=max_images, **kw)


def to_dev(batch, attr=True):
    return batch["img"].cuda(), (batch["attrs"].t()[0].contiguous().cuda() if attr else None), batch["label"].cuda()


def images_of(mcfg, bs):
    return bs * 2 if mcfg.dim_per_3d_slice else bs


_REF = {}


def helper_ref(mcfg, seed, bs, init="random", attr=True):
    """(state dict, batch, keys, loss, logits, gradients) of the helper - computed once per case and shared."""
    key = (mcfg, seed, bs, init, attr)
    if key not in _REF:
        sd = synth.make_state_dict(mcfg, seed=seed, lora_init=init)
        batch = synth.make_batch(mcfg, bs, seed=1234)
        keys = synth.trainable_keys(mcfg)
        with R.adapted_oracle():
            loss, logits, grads = O.loss_and_grads(sd, batch if attr else {**batch, "attrs": None}, mcfg, keys)
        _REF[key] = (sd, batch, keys, loss, logits, grads)
    return _REF[key]


def check_step(eng, out, keys, logits, grads, dtype, tag=""):
    f32, f16 = dtype == F32, dtype == F16
    e = rel(out["logits"], logits)
    print(tag, dtype, "logits rel", e)
    assert e < (1e-5 if f32 else 4e-3 if f16 else 2e-2)
    assert int(out["finite"]) == 1
    worst, wcos = 0.0, 1.0
    for k in keys:
        g, ref = eng.params.view(k, "grad"), grads[k]
        if float(ref.abs().max()) == 0.0:
            assert float(g.abs().max()) < 1e-12, k
            continue
        e, c = rel(g, ref), cos(g, ref)
        worst, wcos = max(worst, e), min(wcos, c)
        if f32:
            assert e < 2e-3, (k, e)
        else:
            assert c > (0.999 if f16 else 0.99) and e < (0.03 if f16 else 0.15), (k, c, e)
    print(tag, dtype, "worst grad err", worst, "worst cosine", wcos)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("targets", ["attn", "mlp+attn"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_tiny_step_vs_helper(targets, dtype):
    mcfg = with_targets(C.vit_tiny(rank=4), targets)
    sd, batch, keys, loss, logits, grads = helper_ref(mcfg, 1, 8)
    assert any(ATTN_SITES[0] in k for k in keys) and any("mlp.c_fc.lora_A" in k for k in keys) == (targets == "mlp+attn")
    eng = make_engine(mcfg, sd, dtype, 8)
    img, attr, label = to_dev(batch)
    out = eng.forward_backward(img, attr, label)
    torch.cuda.synchronize()
    assert abs(float(out["loss"]) - float(loss)) <= (1e-5 if dtype == F32 else 1e-3 if dtype == F16 else 5e-3) * abs(float(loss))
    check_step(eng, out, keys, logits, grads, dtype, targets)
    assert rel(eng.forward(img, attr), out["logits"]) < 1e-6


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,mcfg,bs,attr", [
    ("lora", C.vit_tiny_lora("LoRA", False), 8, True),
    ("svlora", C.vit_tiny_lora("SVLoRA", False), 8, True),
    ("svlora_globals", C.vit_tiny_lora("SVLoRA", True), 8, True),
    ("globals", C.vit_tiny_lora("FairLoRA", True), 8, True),
    ("tiny3d", C.vit_tiny_3d(rank=4, dim_per_3d_slice=4), 6, True),       # 6 samples x 2 slice groups
    ("no_attr", C.vit_tiny(rank=4), 8, False),
])
def test_other_types_3d_and_no_attr_f32(tag, mcfg, bs, attr):
    mcfg = with_targets(mcfg, "mlp+attn")
    sd, batch, keys, loss, logits, grads = helper_ref(mcfg, 1, bs, attr=attr)
    eng = make_engine(mcfg, sd, F32, images_of(mcfg, bs))
    out = eng.forward_backward(*to_dev(batch, attr))
    torch.cuda.synchronize()
    check_step(eng, out, keys, logits, grads, F32, tag)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_attribute_outside_the_groups_is_the_uniform_mix_bit_for_bit(dtype):
    """-1 and G give a sample the uniform mix of attr=None.  All samples out of range == no attribute at all,
    gradients bit-equal; and mixed with valid attributes the step still agrees with the helper (whose group_mix holds
    the same rule)."""
    mcfg = with_targets(C.vit_tiny(rank=4), "mlp+attn")
    G = mcfg.lora.num_groups
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    batch = synth.make_batch(mcfg, 8, seed=1234)
    img, _, label = to_dev(batch)
    bad = torch.tensor([-1, G, -1, G, G, -1, -1, G], device="cuda")
    e1, e2 = make_engine(mcfg, sd, dtype, 8), make_engine(mcfg, sd, dtype, 8)
    o1, o2 = e1.forward_backward(img, bad, label), e2.forward_backward(img, None, label)
    torch.cuda.synchronize()
    assert torch.equal(o1["logits"], o2["logits"]) and torch.equal(e1.params.grad, e2.params.grad)
    assert float(e1.params.grad.abs().max()) > 0
    if dtype == F32:
        mixed = batch["attrs"].clone()
        mixed[1, 0], mixed[4, 0] = -1, G
        b2 = {**batch, "attrs": mixed}
        keys = synth.trainable_keys(mcfg)
        with R.adapted_oracle():
            loss, logits, grads = O.loss_and_grads(sd, b2, mcfg, keys)
        e3 = make_engine(mcfg, sd, F32, 8)
        out = e3.forward_backward(*to_dev(b2))
        torch.cuda.synchronize()
        check_step(e3, out, keys, logits, grads, F32, "mixed attr")


# 3 ---------------------------------------------------------------------------------------------------------------
def test_rank_24_route_bf16():
    """rank > 16: the down projections are launches of their own in front of the products."""
    mcfg = with_targets(C.vit_tiny(rank=24), "mlp+attn")
    sd, batch, keys, loss, logits, grads = helper_ref(mcfg, 1, 8)
    eng = make_engine(mcfg, sd, BF16, 8)
    assert not eng.fused_rank
    out = eng.forward_backward(*to_dev(batch))
    torch.cuda.synchronize()
    check_step(eng, out, keys, logits, grads, BF16, "rank24")


# 4 ---------------------------------------------------------------------------------------------------------------
def test_merged_weights_on_the_gpu_without_the_helper():
    mcfg = with_targets(C.vit_tiny(rank=4), "mlp+attn")
    sd = synth.make_state_dict(mcfg, seed=3, lora_init="random")
    img = synth.make_batch(mcfg, 8, seed=11)["img"].cuda()
    got = make_engine(mcfg, sd, F32, 8).forward(img, None).clone()
    base = make_engine(with_targets(mcfg, "mlp"), R.merged_state_dict(sd, mcfg), F32, 8)
    ref = base.forward(img, None)
    plain = make_engine(with_targets(mcfg, "mlp"), {k: v for k, v in sd.items() if "_proj_lora." not in k}, F32, 8).forward(img, None)
    print("merged-weight engine vs adapted engine:", rel(got, ref), "(adapters off:", rel(plain, ref), ")")
    assert rel(got, ref) < 1e-5
    assert rel(plain, ref) > 1e-4                   # the adapters are not a no-op here


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_reference_init_is_a_no_op_and_the_chain_reaches_block_0(dtype):
    """lora_A = 0: the logits of the default placement; dB and dS of the new sites exactly zero (their t is zero), dA not -
    in block 0 too, whose dA(in_proj) exists only if the dX chain runs through dX(out_proj) and the attention backward."""
    mcfg = with_targets(C.vit_tiny(rank=4), "mlp+attn")
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="reference")
    batch = synth.make_batch(mcfg, 8, seed=1234)
    img, attr, label = to_dev(batch)
    eng = make_engine(mcfg, sd, dtype, 8)
    base = make_engine(with_targets(mcfg, "mlp"), {k: v for k, v in sd.items() if "_proj_lora." not in k}, dtype, 8)
    if dtype == F32:
        assert rel(eng.forward(img, attr), base.forward(img, attr)) < 1e-6
    eng.forward_backward(img, attr, label)
    torch.cuda.synchronize()
    for i in range(mcfg.vision.layers):
        for site in ATTN_SITES:
            q = f"image_encoder.transformer.resblocks.{i}.{site}"
            assert float(eng.params.view(q + "lora_B.weight", "grad").abs().max()) == 0.0, q
            assert float(eng.params.view(q + "lora_S.weight", "grad").abs().max()) == 0.0, q
            assert float(eng.params.view(q + "lora_A.weight", "grad").abs().max()) > 0.0, q
    if dtype == F32:
        keys = synth.trainable_keys(mcfg)
        with R.adapted_oracle():
            _, logits, grads = O.loss_and_grads(sd, batch, mcfg, keys)
        for k in keys:
            if "_proj_lora.lora_A" in k:
                assert rel(eng.params.view(k, "grad"), grads[k]) < 2e-3, k


# 6 ---------------------------------------------------------------------------------------------------------------
V_LAYERS, MAX_IMAGES = 2, 28


def route_cfg():
    base = C.vit_b16(rank=8)
    base = dataclasses.replace(base, vision=dataclasses.replace(base.vision, layers=V_LAYERS), text=C.vit_tiny().text)
    return with_targets(base, "mlp+attn")


@pytest.fixture(scope="module")
def panel_engines():
    mcfg = route_cfg()
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    return mcfg, make_engine(mcfg, sd, BF16, MAX_IMAGES), make_engine(mcfg, sd, F32, MAX_IMAGES)


def gemm_launches(plan):
    return [f.args[0]._obj for f in plan if getattr(f, "name", None) == "ffm_gemm_nt"]


@pytest.mark.parametrize("images", [13, 28])
def test_vitb16_width_panel_path_and_folds(panel_engines, images):
    """ViT-B/16 width, heads and tokens: the bf16 step against the fp32 engine (the bounds of
    test_vitb16_bs32_panel_path_vs_fp32_engine), and the recorded plan counted as tests/test_route_gpu.py counts it."""
    mcfg, eng, ref = panel_engines
    v = mcfg.vision
    batch = synth.make_batch(mcfg, images, seed=1234)
    args = to_dev(batch)
    eng.step_plans.clear()
    out = eng.forward_backward(*args)
    oref = ref.forward_backward(*args)
    torch.cuda.synchronize()
    e = rel(out["logits"], oref["logits"])
    print(f"images {images}: logits rel {e}")
    assert e < 2e-2 and int(out["finite"]) == 1
    worst = 1.0
    for k in synth.trainable_keys(mcfg):
        g, gr = eng.params.view(k, "grad"), ref.params.view(k, "grad")
        c = cos(g, gr)
        worst = min(worst, c)
        assert c > 0.99 and rel(g, gr) < 0.15, (k, c, rel(g, gr))
    print(f"images {images}: worst gradient cosine {worst}")
    if panel_override():
        return
    rows = images * v.tokens
    rt = eng.vis.route(rows)
    (plan,) = eng.step_plans.values()
    gem = gemm_launches(plan)
    fwd_lora = [a for a in gem if (a.flags & L.EPI_LORA) and not (a.flags & L.EPI_LORA_KR)]
    bwd_lora = [a for a in gem if (a.flags & L.EPI_LORA) and (a.flags & L.EPI_LORA_KR)]
    # four adapted products per block forward; backward: block 0 stops at dqkv (no dX(in_proj)), every other block has four
    assert len(fwd_lora) == 4 * V_LAYERS
    assert len(bwd_lora) == 4 * V_LAYERS - 1
    assert sum(bool(a.flags & L.EPI_LNIN) for a in gem) == V_LAYERS * (bool(rt.ln1) + bool(rt.ln2))
    qkv = [a for a in gem if a.N == 3 * v.width and a.K == v.width and a.M == rows]
    assert len(qkv) == V_LAYERS and all(a.flags & L.EPI_LORA and a.flags & L.EPI_RANKOP for a in qkv)
    assert all(bool(a.flags & L.EPI_LNIN) == bool(rt.ln1) for a in qkv)
    # ln_1's backward is never folded for an adapted in-projection
    names = Counter(getattr(f, "name", None) for f in plan)
    assert rt.ln1_bwd == 0 and names["ffm_attention_bwd_lnstat"] == 0
    assert names["ffm_attention_bwd"] == V_LAYERS + mcfg.text.layers
    if images == 28:
        assert rt.ln1 > 0 and rt.ln2 > 0                # the folds are on where the default placement has them


# 7 ---------------------------------------------------------------------------------------------------------------
def test_five_sgd_steps_f32():
    mcfg = with_targets(C.vit_tiny(rank=4), "mlp+attn")
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    batch = synth.make_batch(mcfg, 8, seed=1234)
    keys = synth.trainable_keys(mcfg)
    eng = make_engine(mcfg, sd, F32, 8)
    args = to_dev(batch)
    ref_sd = {k: v.clone() for k, v in sd.items()}
    opt = O.SgdState(lr=1e-3, momentum=0.9, weight_decay=5e-4)
    with R.adapted_oracle():
        for _ in range(5):
            out = eng.forward_backward(*args)
            eng.sgd_step(1e-3, 0.9, 5e-4, repeats=2)
            ref_loss = O.train_step(ref_sd, opt, batch, mcfg, keys, optimizer_steps=2)[0]["loss"]
            assert abs(float(out["loss"]) - ref_loss) <= 1e-4 * abs(ref_loss), (float(out["loss"]), ref_loss)
    for k in keys:
        assert rel(eng.params.view(k), ref_sd[k]) < 1e-4, k


# 8 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,rank", [(F32, 4), (BF16, 4), (F16, 4), (BF16, 24)], ids=["f32", "bf16", "f16", "bf16_r24"])
def test_infer_is_bit_identical_to_forward(dtype, rank):
    mcfg = with_targets(C.vit_tiny(rank=rank), "mlp+attn")
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    batch = synth.make_batch(mcfg, 8, seed=1234)
    img, attr, _ = to_dev(batch)
    eng = make_engine(mcfg, sd, dtype, 8)
    want = eng.forward(img, attr).clone()
    assert torch.equal(eng.infer(img, attr), want)
    with eng.inference():
        assert torch.equal(eng.infer(img, attr), want)
        assert torch.equal(eng.infer(img[:3], attr[:3]), eng.forward(img[:3], attr[:3]))
    assert torch.equal(eng.infer(img, None), eng.forward(img, None))


def test_infer_bit_identical_on_the_panel_path(panel_engines):
    mcfg, eng, _ = panel_engines
    batch = synth.make_batch(mcfg, MAX_IMAGES, seed=5)
    img, attr, _ = to_dev(batch)
    want = eng.forward(img, attr).clone()
    assert torch.equal(eng.infer(img, attr), want)


# 9 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_two_engines_train_bit_identically(dtype):
    mcfg = with_targets(C.vit_tiny(rank=4), "mlp+attn")
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    args = to_dev(synth.make_batch(mcfg, 8, seed=1234))
    a, b = make_engine(mcfg, sd, dtype, 8), make_engine(mcfg, sd, dtype, 8)
    for _ in range(3):
        oa, ob = a.forward_backward(*args), b.forward_backward(*args)
        assert torch.equal(oa["loss"], ob["loss"]) and torch.equal(a.params.grad, b.params.grad)
        a.sgd_step(1e-3, 0.9, 5e-4)
        b.sgd_step(1e-3, 0.9, 5e-4)
    torch.cuda.synchronize()
    assert torch.equal(a.params.flat, b.params.flat)


# 10 --------------------------------------------------------------------------------------------------------------
def trainer_cfg(targets):
    return NS(
        SEED=1, OUTPUT_DIR="", VERBOSE=False,
        INPUT=NS(PIXEL_MEAN=list(C.CLIP_PIXEL_MEAN), PIXEL_STD=list(C.CLIP_PIXEL_STD), SIZE=(64, 64)),
        DATASET=NS(NAME="FairFedMed", ATTRIBUTES=["race"], ATTRIBUTE_TYPE="race"),
        MODEL=NS(BACKBONE=NS(NAME="tiny"), GEOMETRY=C.vit_tiny(), STATE_DICT=None),
        TRAINER=NS(NAME="GLP_OT_SVLoRA", LAMBDA_FAIRNESS=0.0,
                   GLP_OT=NS(N=2, N_CTX=4, PREC="fp32", OT="None"),
                   GLP_OT_LORA=NS(RANK=4, ALPHA=2.0, TYPE="FairLoRA", GLOBAL_S=False, DISABLE_ATTR=False,
                                  UNFREEZE_IMAGE_ENCODER=True, TARGETS=targets)),
        OPTIM=NS(NAME="sgd", LR=1e-3, MOMENTUM=0.9, WEIGHT_DECAY=5e-4, LR_SCHEDULER="single_step", STEPSIZE=2,
                 GAMMA=0.1, MAX_EPOCH=1),
        DATALOADER=NS(TRAIN_X=NS(BATCH_SIZE=8)), TEST=NS(BATCH_SIZE=8, NO_TEST=True),
        TRAIN=NS(METRICS_EVERY=1, CHECKPOINT_FREQ=0),
    )


def test_trainer_with_attention_targets(tmp_path):
    from fairfedmed_amd.model import apply_lora_to_model
    from fairfedmed_amd.trainer import GLP_OT_SVLoRA, SyntheticFedData
    mcfg = with_targets(C.vit_tiny(rank=4), "mlp+attn")
    data = SyntheticFedData(mcfg, 1, 2, 1, 8, signal=0.3)
    tr = GLP_OT_SVLoRA(trainer_cfg("mlp+attn"), data=data)
    assert tr.model.cfg.lora.targets == "mlp+attn"
    assert list(tr.model.state_dict()) == list(synth.manifest(mcfg))
    apply_lora_to_model(tr.model, True, rank=4, alpha=2.0, lora_type="FairLoRA", num_attrs=3, targets="mlp+attn")
    with pytest.raises(ValueError):
        apply_lora_to_model(tr.model, True, rank=4, alpha=2.0, lora_type="FairLoRA", num_attrs=3)
    tr.fed_before_train()
    before = {k: v.clone() for k, v in tr.model.state_dict().items() if "_proj_lora." in k}
    batch = synth.make_batch(mcfg, 8, seed=1234)
    tr.num_batches = 10 ** 9
    for i in range(2):
        tr.batch_idx = i
        s = tr.forward_backward(batch)
        assert float(s["loss"]) == float(s["loss"])
    after = tr.model.state_dict()
    assert all(not torch.equal(after[k], before[k]) for k in before if k.endswith("lora_A.weight"))
    res = tr.test(idx=0, current_epoch=0)
    assert len(res) >= 4 and all(x == x for x in res[:4])
    # save / load round trip: the new keys come back
    tr.save_model(0, str(tmp_path), is_best=True)
    img, attr = batch["img"].cuda(), batch["attrs"].t()[0].cuda()
    want = tr.model_inference(img, attr).clone()
    fresh = GLP_OT_SVLoRA(trainer_cfg("mlp+attn"), data=data)
    assert not torch.equal(fresh.model_inference(img, attr), want)
    fresh.load_model(str(tmp_path))
    assert torch.equal(fresh.model_inference(img, attr), want)
    got = fresh.model.state_dict()
    for k in before:
        assert torch.equal(got[k], after[k]), k
    # a config tree without the key is the reference's placement
    cfg0 = trainer_cfg("mlp")
    del cfg0.TRAINER.GLP_OT_LORA.TARGETS
    assert GLP_OT_SVLoRA(cfg0, data=SyntheticFedData(C.vit_tiny(rank=4), 1, 1, 1, 8)).model.cfg.lora.targets == "mlp"
