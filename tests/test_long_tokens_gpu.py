"""The engine and the trainer on a ViT of more than 256 tokens (streaming attention, csrc/attention_long.hip): the tiny
tower at 272^2 (290 tokens) and 336^2 (442 tokens), against the host oracle with the bounds of
test_engine_gpu.py::test_tiny_step_vs_oracle_and_golden."""
import math
from types import SimpleNamespace as NS

import pytest
import torch

from fairfedmed_amd import config as C
from fairfedmed_amd import synth

pytestmark = pytest.mark.gpu

BS = 4
SIZES = [272, 336]
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])


def cos(got, ref):
    got = torch.as_tensor(got).double().cpu().flatten()
    ref = torch.as_tensor(ref).double().cpu().flatten()
    return float(torch.dot(got, ref) / (got.norm() * ref.norm()).clamp_min(1e-300))


def rel(got, ref):
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def make_engine(mcfg, sd, dtype, max_images):
    from fairfedmed_amd.engine import FairLoRAEngine
    return FairLoRAEngine(mcfg, sd, dtype=dtype, max_images=max_images)


def to_dev(batch):
    return batch["img"].cuda(), batch["attrs"].t()[0].cuda(), batch["label"].cuda()


_CASES = {}


def case(mcfg, bs):
    """(state_dict, batch, trainable keys, oracle logits, oracle gradients) - computed once per geometry, never modified."""
    if mcfg not in _CASES:
        from oracle import fairlora_oracle as O
        sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
        batch = synth.make_batch(mcfg, bs, seed=1234)
        keys = synth.trainable_keys(mcfg)
        _, logits, grads = O.loss_and_grads(sd, batch, mcfg, keys)
        _CASES[mcfg] = (sd, batch, keys, logits, grads)
    return _CASES[mcfg]


def step_against_oracle(mcfg, bs, images, dtype):
    sd, batch, keys, logits, grads = case(mcfg, bs)
    assert mcfg.vision.tokens > 256
    eng = make_engine(mcfg, sd, dtype, images)
    img, attr, label = to_dev(batch)
    out = eng.forward_backward(img, attr, label)
    torch.cuda.synchronize()
    f32, f16 = dtype == torch.float32, dtype == torch.float16
    e = rel(out["logits"], logits)
    print(mcfg.vision.tokens, dtype, "logits", e)
    assert e < (1e-5 if f32 else 4e-3 if f16 else 2e-2)
    assert int(out["finite"]) == 1
    worst, wcos = 0.0, 1.0
    for k in keys:
        g = eng.params.view(k, "grad")
        ref = grads[k]
        if float(ref.abs().max()) == 0.0:
            assert float(g.abs().max()) < 1e-12, k
            continue
        e = rel(g, ref)
        worst, wcos = max(worst, e), min(wcos, cos(g, ref))
        if f32:
            assert e < 2e-3, (k, e)
        else:
            assert cos(g, ref) > (0.999 if f16 else 0.99) and e < (0.03 if f16 else 0.15), (k, cos(g, ref), e)
    print(mcfg.vision.tokens, dtype, "worst grad err", worst, "worst cosine", wcos)
    assert rel(eng.forward(img, attr), out["logits"]) < 1e-6
    return eng, img, attr


@pytest.mark.parametrize("size", SIZES)
@DTYPES
def test_long_step_vs_oracle_and_inference(size, dtype):
    eng, img, attr = step_against_oracle(C.vit_tiny(rank=4, image_size=size), BS, BS, dtype)
    # the forward-only pass (its own workspace, attention without lse) gives forward()'s bits
    want = eng.forward(img, attr).clone()
    assert bool(torch.isfinite(want).all())
    with eng.inference():
        inside = eng.infer(img, attr).clone()
    assert torch.equal(inside, want) and torch.equal(eng.infer(img, attr), want)


def test_long_step_3d_front_end_vs_oracle():
    """The slice front end multiplies the image count (2 samples x 2 slice groups of 290 tokens)."""
    step_against_oracle(C.vit_tiny_3d(rank=4, dim_per_3d_slice=4, image_size=272), 2, 4, torch.float32)


@DTYPES
def test_long_two_engines_train_bit_identically(dtype):
    mcfg = C.vit_tiny(rank=4, image_size=272)
    sd, batch, keys, _, _ = case(mcfg, BS)
    img, attr, label = to_dev(batch)
    engines = [make_engine(mcfg, sd, dtype, BS) for _ in range(2)]
    for eng in engines:
        for _ in range(2):
            out = eng.forward_backward(img, attr, label)
            assert int(out["finite"]) == 1
            eng.sgd_step(1e-3, 0.9, 5e-4)
    torch.cuda.synchronize()
    moved = False
    for k in keys:
        a, b = engines[0].params.view(k), engines[1].params.view(k)
        assert torch.equal(a, b), k
        moved = moved or not torch.equal(a.cpu().reshape(-1), sd[k].reshape(-1))
    assert moved, "two steps changed no trainable tensor"


def test_long_trainer_resizes_a_64px_checkpoint():
    """GLP_OT_SVLoRA with INPUT.INTERPOLATE_POS: a checkpoint of the 64^2 tiny tower (17 positional rows) trains and
    evaluates at 272^2 (290 rows)."""
    from fairfedmed_amd.trainer import GLP_OT_SVLoRA, SyntheticFedData
    ckpt = C.vit_tiny(rank=4)
    cfg = NS(
        SEED=1, OUTPUT_DIR="", VERBOSE=False,
        INPUT=NS(PIXEL_MEAN=list(C.CLIP_PIXEL_MEAN), PIXEL_STD=list(C.CLIP_PIXEL_STD), SIZE=(272, 272), INTERPOLATE_POS=True),
        DATASET=NS(NAME="FairFedMed", ATTRIBUTES=["race"], ATTRIBUTE_TYPE="race"),
        MODEL=NS(BACKBONE=NS(NAME="tiny"), GEOMETRY=ckpt, STATE_DICT=None),
        TRAINER=NS(NAME="GLP_OT_SVLoRA", LAMBDA_FAIRNESS=0.0,
                   GLP_OT=NS(N=2, N_CTX=4, PREC="bf16", OT="None"),
                   GLP_OT_LORA=NS(RANK=4, ALPHA=2.0, TYPE="FairLoRA", GLOBAL_S=False, DISABLE_ATTR=False,
                                  UNFREEZE_IMAGE_ENCODER=True)),
        OPTIM=NS(NAME="sgd", LR=1e-3, MOMENTUM=0.9, WEIGHT_DECAY=5e-4, LR_SCHEDULER="single_step", STEPSIZE=2,
                 GAMMA=0.1, MAX_EPOCH=1),
        DATALOADER=NS(TRAIN_X=NS(BATCH_SIZE=BS)), TEST=NS(BATCH_SIZE=BS, NO_TEST=True),
        TRAIN=NS(METRICS_EVERY=1, CHECKPOINT_FREQ=0),
    )
    sd = synth.make_state_dict(ckpt, seed=1, lora_init="random")
    assert sd["image_encoder.positional_embedding"].shape[0] == 17
    data = SyntheticFedData(C.vit_tiny(rank=4, image_size=272), 1, 1, 1, BS)
    tr = GLP_OT_SVLoRA(cfg, data=data, state_dict=sd)
    assert tr.engine.cfg.vision.tokens == 290
    assert sd["image_encoder.positional_embedding"].shape[0] == 17, "the caller's checkpoint was modified"
    pos = tr.model.state_dict()["image_encoder.positional_embedding"]
    assert tuple(pos.shape) == (290, 128)
    assert torch.equal(pos[0].float().cpu(), sd["image_encoder.positional_embedding"][0])
    tr.train(idx=0, global_epoch=0)
    batch = next(iter(data.fed_train_loader_x_dict[0]))
    s = tr.forward_backward(batch)
    assert math.isfinite(float(s["loss"]))
    res = tr.test(idx=0)
    assert len(res) == 4 and all(math.isfinite(float(x)) for x in res[:3])
