"""transport="native" through the engines and the trainer.  The engine resizes a ``NativeBatch`` with ffm_resize_u8 into the
buffer it expands uint8 batches into and goes on as for a float32 tensor, so against the float32 tensor that
``ops.resize_u8`` leaves for the same batch everything is held to ``torch.equal``; against the host resize
(transport="float32") the trained weights are held to the 1e-4 relative DESIGN.md section 2 holds fp32 trajectories to."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from fairfedmed_amd import config as C
from fairfedmed_amd import data as D
from fairfedmed_amd import synth

pytestmark = pytest.mark.gpu


def rel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def native_batch(R=64, seed=21):
    g = np.random.default_rng(seed)
    sizes = ((40, 40), (96, 96), (64, 64), (50, 70))                               # enlarge, shrink, identity, non-square
    return D.NativeBatch.from_planes([g.integers(0, 256, size=(1, h, w), dtype=np.uint8) for h, w in sizes], 3, R)


@pytest.mark.parametrize("case,dtype", [("vit", torch.float32), ("vit", torch.bfloat16), ("rn", torch.float32)],
                         ids=["vit_f32", "vit_bf16", "rn_f32"])
def test_engines_take_a_native_batch_as_the_resized_tensor(case, dtype):
    from fairfedmed_amd import ops
    from fairfedmed_amd.engine_rn import create_engine
    mcfg = C.rn_tiny(rank=4, num_groups=2) if case == "rn" else C.vit_tiny(rank=4)
    nb = native_batch().to("cuda")
    f32 = ops.resize_u8(nb, torch.empty(4, 3, 64, 64, device="cuda")).clone()
    g = torch.Generator().manual_seed(3)
    attr = torch.randint(0, mcfg.lora.num_groups, (4,), generator=g).cuda()
    label = torch.randint(0, 2, (4,), generator=g).cuda()
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    ea = create_engine(mcfg, sd, dtype=dtype, max_images=8)
    eb = create_engine(mcfg, sd, dtype=dtype, max_images=8)
    assert torch.equal(ea.forward(f32, attr), eb.forward(nb, attr))
    assert torch.equal(ea.infer(f32, attr), eb.infer(nb, attr))
    oa, ob = ea.forward_backward(f32, attr, label), eb.forward_backward(nb, attr, label)
    assert torch.equal(oa["loss"], ob["loss"]) and torch.equal(oa["logits"], ob["logits"])
    assert torch.equal(ea.params.grad, eb.params.grad) and float(ea.params.grad.abs().max()) > 0
    ob2 = eb.forward_backward(nb, attr, label)                                     # (the replayed plan: inputs load outside it)
    assert torch.equal(ob2["loss"], oa["loss"])
    # what is refused stays refused
    with pytest.raises(ValueError, match="resizes to 32"):
        eb.forward(native_batch(R=32).to("cuda"), attr)
    with pytest.raises(TypeError):
        eb.forward(native_batch(), attr)                                           # on the host: no CPU path
    with pytest.raises(ValueError, match="expected"):
        eb.forward(torch.zeros(2, 1, 32, 32, dtype=torch.uint8, device="cuda"), None)
    with pytest.raises(ValueError, match="expected"):
        eb.forward(torch.zeros(2, 3, 32, 32, device="cuda"), None)


def make_cfg(bs=8):
    return NS(
        SEED=1, OUTPUT_DIR="", VERBOSE=False,
        INPUT=NS(PIXEL_MEAN=list(C.CLIP_PIXEL_MEAN), PIXEL_STD=list(C.CLIP_PIXEL_STD), SIZE=(64, 64)),
        DATASET=NS(NAME="FairFedMed", ATTRIBUTES=["race"], ATTRIBUTE_TYPE="race"),
        MODEL=NS(BACKBONE=NS(NAME="tiny"), GEOMETRY=C.vit_tiny(), STATE_DICT=None),
        TRAINER=NS(NAME="GLP_OT_SVLoRA", LAMBDA_FAIRNESS=0.0,
                   GLP_OT=NS(N=2, N_CTX=4, PREC="fp32", OT="None"),
                   GLP_OT_LORA=NS(RANK=4, ALPHA=2.0, TYPE="FairLoRA", GLOBAL_S=False, DISABLE_ATTR=False,
                                  UNFREEZE_IMAGE_ENCODER=True)),
        OPTIM=NS(NAME="sgd", LR=1e-3, MOMENTUM=0.9, WEIGHT_DECAY=5e-4, LR_SCHEDULER="single_step", STEPSIZE=2,
                 GAMMA=0.1, MAX_EPOCH=1),
        DATALOADER=NS(TRAIN_X=NS(BATCH_SIZE=bs)), TEST=NS(BATCH_SIZE=bs, NO_TEST=True),
        TRAIN=NS(METRICS_EVERY=1, CHECKPOINT_FREQ=0),
    )


class _ResizedUpFront:
    """A native loader whose batches are resized with ops.resize_u8 before the trainer sees them: float32 tensors."""

    def __init__(self, loader):
        self.loader = loader

    def __getattr__(self, k):
        return getattr(self.loader, k)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        from fairfedmed_amd import ops
        for b in self.loader:
            nb = b["img"]
            assert isinstance(nb, D.NativeBatch)
            dst = torch.empty(len(nb), nb.C1 * nb.rep, nb.R, nb.R, device="cuda")
            yield dict(b, img=ops.resize_u8(nb.to("cuda"), dst))


def test_trainer_native_transport_on_mixed_sizes(tmp_path):
    """Two clients read a FairFedMed tree whose samples are stored at 40, 96 and 64 pixels (tower: 64)."""
    from fairfedmed_amd import federated as F
    from fairfedmed_amd.registry import build_trainer
    import fairfedmed_amd.trainer  # noqa: F401  (registers GLP_OT_SVLoRA)
    D.write_synthetic_fairfedmed(str(tmp_path), sites=2, n_train=16, n_test=8, seed=4, sizes=[40, 96, 64])
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="reference")
    hist = {}
    for mode in ("native", "upfront", "float32"):
        cfg = make_cfg(bs=8)
        cfg.DATASET = NS(NAME="FairFedMed", ROOT=str(tmp_path), USERS=2, ATTRIBUTE_TYPE="race",
                         ATTRIBUTES=["race", "gender"], MODALITY_TYPE="slo_fundus")
        cfg.TEST.NO_TEST = True
        cfg.DATA = D.FedData(cfg, transport="float32" if mode == "float32" else "native")
        if mode == "upfront":
            for d in (cfg.DATA.fed_train_loader_x_dict, cfg.DATA.fed_test_loader_x_dict):
                for k in d:
                    d[k] = _ResizedUpFront(d[k])
        cfg.MODEL.STATE_DICT = sd
        tr = build_trainer(cfg)
        first = next(iter(tr.fed_train_loader_x_dict[0]))["img"]
        if mode == "native":
            assert isinstance(first, D.NativeBatch) and len(first) == 8 and set(first.sizes) == {(40, 40), (96, 96), (64, 64)}
        else:
            assert first.dtype == torch.float32 and tuple(first.shape) == (8, 3, 64, 64)
        hist[mode] = F.run_fedotplora(tr, F.FedArgs(num_users=2, frac=1.0, round=2, shared_half_s=True, seed=0),
                                      log=lambda *_: None)
    a, b, c = hist["native"], hist["upfront"], hist["float32"]
    for k, v in a["global_weights"].items():
        assert torch.equal(v, b["global_weights"][k]), k
        r = rel(v, c["global_weights"][k])
        print(k, r)
        assert r < 1e-4, (k, r)
    assert a["acc"] == b["acc"] and a["auc"] == b["auc"]


def test_cli_runs_the_fairlora_script_with_native_transport(tmp_path):
    """python -m fairfedmed_amd.federated_main with the flags of scripts/fairfedlora_fairfedmed.sh and --transport native on a
    tree none of whose samples has the tower's size."""
    from fairfedmed_amd import federated_main as FM
    D.write_synthetic_fairfedmed(str(tmp_path / "DATA"), sites=2, n_train=8, n_test=8, seed=9, attribute_type="language",
                                 sizes=[40, (96, 80)])
    (tmp_path / "tr.yaml").write_text('DATALOADER:\n  TRAIN_X:\n    BATCH_SIZE: 8\n  TEST:\n    BATCH_SIZE: 8\n'
                                      'INPUT:\n  SIZE: (64, 64)\nMODEL:\n  BACKBONE:\n    NAME: "tiny"\n')
    argv = ["--root", str(tmp_path / "DATA"), "--model", "FedOTPLoRA", "--seed", "1", "--num_users", "2", "--frac", "1.0",
            "--lr", "0.001", "--OT", "None", "--gamma", "0.1", "--trainer", "GLP_OT_SVLoRA", "--round", "1",
            "--stepsize", "200", "--attribute_type", "language", "--attributes", "language", "race", "gender",
            "--n_ctx", "4", "--num_prompt", "2", "--unfreeze_image_encoder", "True", "--lora_rank", "4",
            "--lora_alpha", "2", "--lora_type", "FairLoRA", "--config-file", str(tmp_path / "tr.yaml"),
            "--output-dir", str(tmp_path / "out"), "--shared_half_s", "True", "--prec", "fp32", "--transport", "native"]
    seen = {}

    def hook(cfg):
        cfg.MODEL.GEOMETRY = C.vit_tiny(rank=4)
        seen["cfg"] = cfg

    hist = FM.main(argv, log=lambda *a: None, cfg_hook=hook)
    assert len(hist["acc"]) == 1 and all(np.isfinite(hist["auc"]))
    first = next(iter(seen["cfg"].DATA.fed_test_loader_x_dict[0]))["img"]
    assert isinstance(first, D.NativeBatch) and set(first.sizes) == {(40, 40), (80, 96)}
