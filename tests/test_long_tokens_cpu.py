"""Host side of a ViT at an input size other than its checkpoint's (more than 256 tokens from 272^2 on): configuration,
positional-embedding resize, the opt-in flag INPUT.INTERPOLATE_POS through the adapter, the trainer and the command line,
and the route of such a tower.  No GPU."""
import dataclasses
from types import SimpleNamespace as NS

import pytest
import torch

from fairfedmed_amd import config as C
from fairfedmed_amd import synth


def test_image_size_of_the_configurations():
    assert C.vit_b16(image_size=384).vision.tokens == 577
    assert C.vit_b16(image_size=512).vision.tokens == 1025
    assert C.vit_b16() == C.ModelCfg(lora=C.LoraCfg(rank=8, alpha=2.0, num_groups=3)) and C.vit_b16().vision.tokens == 197
    assert C.vit_b16(rank=16, image_size=224) == C.vit_b16(rank=16)
    assert C.vit_tiny().vision.image_size == 64 and C.vit_tiny().vision.tokens == 17
    assert C.vit_tiny(image_size=272).vision.tokens == 290 and C.vit_tiny(image_size=336).vision.tokens == 442
    assert C.vit_tiny_3d(image_size=272).vision.tokens == 290 and C.vit_tiny_3d(image_size=272).dim_per_3d_slice == 4
    assert dataclasses.replace(C.vit_tiny(image_size=272), vision=C.vit_tiny().vision) == C.vit_tiny()
    with pytest.raises(ValueError, match="multiple of the patch"):
        C.vit_b16(image_size=230)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16, torch.float64])
def test_resize_positional_embedding(dt):
    from fairfedmed_amd.clip_adapter import resize_positional_embedding as resize
    g, w = 4, 32
    pos = torch.randn(1 + g * g, w, generator=torch.Generator().manual_seed(3)).to(dt)
    same = resize(pos, g)
    assert same.dtype == torch.float32 and torch.equal(same, pos.float())           # same grid: bit for bit
    big = resize(pos, 17)
    assert big.dtype == torch.float32 and tuple(big.shape) == (1 + 17 * 17, w)
    assert torch.equal(big[0], pos[0].float())                                      # the class row is untouched
    assert not torch.equal(big[1:1 + g * g], pos[1:].float())
    small = resize(pos, 2)
    assert tuple(small.shape) == (5, w) and torch.equal(small[0], pos[0].float())
    const = torch.cat([pos[:1].float(), torch.full((g * g, w), 0.37)])
    out = resize(const.to(dt), 21)
    assert float((out[1:] - const[1].to(dt).float()).abs().max()) <= 1e-6           # a constant embedding stays constant
    with pytest.raises(AssertionError):
        resize(pos[:-1], g)                                                         # not 1 + g * g rows


def _ref_style_cfg(mcfg, size, flag):
    inp = NS(SIZE=(size, size), PIXEL_MEAN=list(mcfg.pixel_mean), PIXEL_STD=list(mcfg.pixel_std))
    if flag is not None:
        inp.INTERPOLATE_POS = flag
    return NS(INPUT=inp,
              DATASET=NS(NAME="FairFedMed", ATTRIBUTE_TYPE="race", ATTRIBUTES=["race"], MODALITY_TYPE="slo_fundus", DIM_PER_3D_SLICE=0),
              DATALOADER=NS(TRAIN_X=NS(BATCH_SIZE=6)), TEST=NS(BATCH_SIZE=6),
              MODEL=NS(BACKBONE=NS(NAME="tiny"), GEOMETRY=mcfg, STATE_DICT=None),
              TRAINER=NS(GLP_OT=NS(N=mcfg.n_prompts, N_CTX=mcfg.n_ctx, PREC="fp32", OT="None", CTX_INIT=False, CSC=False,
                                   CLASS_TOKEN_POSITION="end"),
                         GLP_OT_LORA=NS(RANK=mcfg.lora.rank, ALPHA=mcfg.lora.alpha, TYPE="FairLoRA", GLOBAL_S=False,
                                        UNFREEZE_IMAGE_ENCODER=True, DISABLE_ATTR=False)))


def test_adapter_resizes_a_checkpoint_only_with_the_flag():
    from fairfedmed_amd import clip_adapter as A
    mcfg = C.vit_tiny(rank=4)
    clip_model = synth.make_clip_model(mcfg, seed=1)
    names = ["NOT Glaucoma", "Glaucoma"]
    clip_pos = clip_model.state_dict()["visual.positional_embedding"]
    assert clip_pos.shape[0] == 17
    # the reference's assertion stands without the flag (absent or off)
    for flag in (None, False):
        with pytest.raises(AssertionError, match="must equal to clip_imsize"):
            A.from_reference_args(_ref_style_cfg(mcfg, 272, flag), names, clip_model)
    # equal sizes: the flag changes nothing
    torch.manual_seed(0)
    plain, sd0, _ = A.from_reference_args(_ref_style_cfg(mcfg, 64, None), names, clip_model)
    torch.manual_seed(0)
    flagged, sd1, _ = A.from_reference_args(_ref_style_cfg(mcfg, 64, True), names, clip_model)
    assert plain == flagged == mcfg and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    assert torch.equal(sd0["image_encoder.positional_embedding"], clip_pos.float())
    # with it: the geometry of INPUT.SIZE, the positional embedding resized, everything else the checkpoint's
    got, sd, _ = A.from_reference_args(_ref_style_cfg(mcfg, 272, True), names, clip_model)
    assert got.vision.tokens == 290 and got == C.vit_tiny(rank=4, image_size=272)
    pos = sd["image_encoder.positional_embedding"]
    assert tuple(pos.shape) == (290, 128) and pos.dtype == torch.float32
    assert torch.equal(pos, A.resize_positional_embedding(clip_pos, 17)) and torch.equal(pos[0], clip_pos[0].float())
    assert list(sd.keys()) == list(synth.manifest(got).keys())
    assert torch.equal(sd["image_encoder.conv1.weight"], sd0["image_encoder.conv1.weight"])
    with pytest.raises(ValueError, match="multiple of the patch"):
        A.from_reference_args(_ref_style_cfg(mcfg, 280, True), names, clip_model)
    rn = synth.make_clip_model(C.rn_tiny(rank=4), seed=1)
    with pytest.raises(NotImplementedError, match="ViT"):
        A.model_cfg_from_reference(_ref_style_cfg(C.rn_tiny(rank=4), 96, True), ["NOT Pleural Effusion", "Pleural Effusion"],
                                   {k: v for k, v in rn.state_dict().items()}, A.tokenize_prompts(["NOT Pleural Effusion", "Pleural Effusion"], 4))


def _trainer_model_cfg(cfg):
    """GLP_OT_SVLoRA.model_cfg without the engine (the constructor needs a GPU)."""
    from fairfedmed_amd.trainer import GLP_OT_SVLoRA
    tr = object.__new__(GLP_OT_SVLoRA)
    tr.cfg, tr.dm = cfg, NS(dataset=NS(classnames=["NOT Glaucoma", "Glaucoma"]))
    return tr.model_cfg()


def test_trainer_model_cfg_follows_input_size_only_with_the_flag():
    base = C.vit_tiny(rank=4)
    # without the flag the trainer keeps the geometry it is given, as before (its configurations carry the reference's
    # INPUT.SIZE of 224 beside a reduced MODEL.GEOMETRY; the size assertion is the adapter's, above)
    for flag in (None, False):
        assert _trainer_model_cfg(_ref_style_cfg(base, 272, flag)).vision == base.vision
    assert _trainer_model_cfg(_ref_style_cfg(base, 64, True)).vision == base.vision
    got = _trainer_model_cfg(_ref_style_cfg(base, 272, True))
    assert got.vision.tokens == 290 and got.vision == C.vit_tiny(image_size=272).vision and got.text == base.text
    assert _trainer_model_cfg(_ref_style_cfg(base, 336, True)).vision.tokens == 442
    with pytest.raises(ValueError, match="multiple of the patch"):
        _trainer_model_cfg(_ref_style_cfg(base, 300, True))
    cfg = _ref_style_cfg(base, 384, True)
    cfg.MODEL.BACKBONE.NAME = "ViT-B/16"
    assert _trainer_model_cfg(cfg).vision == C.vit_b16(image_size=384).vision
    cfg = _ref_style_cfg(C.rn_tiny(rank=4), 96, True)
    with pytest.raises(NotImplementedError, match="ViT"):
        _trainer_model_cfg(cfg)


def test_command_line_carries_the_size_and_the_flag():
    from fairfedmed_amd import federated_main as FM
    p = FM.build_parser()
    base = ["--unfreeze_image_encoder", "True", "--OT", "None"]
    cfg = FM.setup_cfg(p.parse_args(base))
    assert cfg.INPUT.SIZE == (224, 224) and cfg.INPUT.INTERPOLATE_POS is False
    args = p.parse_args(base + ["--input_size", "384", "--interpolate_pos"])
    assert args.input_size == 384 and args.interpolate_pos is True
    cfg = FM.setup_cfg(args)
    FM.check_scope(args, cfg)
    assert cfg.INPUT.SIZE == (384, 384) and cfg.INPUT.INTERPOLATE_POS is True
    cfg = FM.setup_cfg(p.parse_args(base + ["--input_size", "384"]))
    assert cfg.INPUT.SIZE == (384, 384) and cfg.INPUT.INTERPOLATE_POS is False
    text = p.format_help()
    assert "--interpolate_pos" in text and "--input_size" in text and "extension" in text


def test_route_of_a_577_token_tower():
    """More than 256 tokens: ffm_attention_bwd_lnstat does not serve the length, so ln_1's backward is the stand-alone
    kernel; every other decision depends on the row count alone."""
    from fairfedmed_amd.engine import Switches, tower_route
    rows = 32 * 577
    long = tower_route(768, 12, 577, False, 8, torch.bfloat16, True, rows, Switches())
    short = tower_route(768, 12, 197, False, 8, torch.bfloat16, True, rows, Switches())
    assert long.ln1_bwd == 0
    assert long == dataclasses.replace(short, ln1_bwd=0)
    # 11 images of 577 tokens: a row count at which the 197-token tower does fold ln_1's backward into its attention
    # backward - the fold that the long tower must not take, and the only field that differs
    rows = 11 * 577
    long = tower_route(768, 12, 577, False, 8, torch.bfloat16, True, rows, Switches())
    short = tower_route(768, 12, 197, False, 8, torch.bfloat16, True, rows, Switches())
    assert short.ln1_bwd == 24 and long.ln1_bwd == 0 and long.ln1 > 0
    assert long == dataclasses.replace(short, ln1_bwd=0)
