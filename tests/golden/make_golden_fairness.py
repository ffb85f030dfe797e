#!/usr/bin/env python3
"""Generate tests/golden/fairness_loss.json by IMPORTING the reference (the harness of make_golden.py, untouched).

The reference's own GLP_OT_SVLoRA.forward_backward (trainers/GLP_OT_SVLoRA.py:883-973) runs one step on the tiny ViT
for TRAINER.LAMBDA_FAIRNESS in {0, 0.5} on two synthetic batches; the reported losses (loss.item(), :960) are stored.
Runs only where the reference is present; only numbers travel.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fairness.py
"""
from __future__ import annotations

import json
import os
import sys
from collections import OrderedDict

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden as MG          # noqa: E402
from fairfedmed_amd import config as C      # noqa: E402
from fairfedmed_amd import synth            # noqa: E402

LAMBDAS = (0.0, 0.5)
BATCHES = ((8, 11), (8, 1234))             # (batch size, synth.make_batch seed)
STATE_SEED = 1


def reference_step(M, CLIP, mcfg, lam: float, bs: int, seed: int) -> dict:
    """One forward_backward of a freshly built reference trainer (object.__new__ + the attributes it touches, as
    make_golden.golden_model does)."""
    sd = synth.make_state_dict(mcfg, seed=STATE_SEED, lora_init="random")
    model = MG.build_reference_model(M, CLIP, mcfg, sd)
    tr = object.__new__(M.GLP_OT_SVLoRA)
    tr.cfg = MG.ref_cfg(mcfg, lambda_fairness=lam)
    tr.model = model
    tr.device = torch.device("cpu")
    params = list(model.prompt_learner.parameters()) + list(model.image_encoder.parameters())
    tr.optim = torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, dampening=0, nesterov=False)
    tr.sched = torch.optim.lr_scheduler.StepLR(tr.optim, step_size=200, gamma=0.1)
    tr._models, tr._optims, tr._scheds = OrderedDict(), OrderedDict(), OrderedDict()
    tr.register_model("prompt_learner", model.prompt_learner, tr.optim, tr.sched)
    tr.register_model("image_encoder", model.image_encoder, tr.optim, tr.sched)
    tr._writer = None
    tr.num_batches, tr.batch_idx = 10, 0
    model.train()
    s = tr.forward_backward(synth.make_batch(mcfg, bs, seed=seed))
    return {"lambda": lam, "batch_size": bs, "batch_seed": seed, "loss": float(s["loss"]), "acc": float(s["acc"]),
            "auc": float(s["auc"])}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    M, CLIP, _, _ = MG.import_reference()
    mcfg = C.vit_tiny(rank=4)
    cases = [reference_step(M, CLIP, mcfg, lam, bs, seed) for bs, seed in BATCHES for lam in LAMBDAS]
    for c in cases:
        print(c)
    out = {"model": "vit_tiny(rank=4)", "state_seed": STATE_SEED, "lora_init": "random", "prec": "fp32",
           "torch": torch.__version__, "cases": cases}
    json.dump(out, open(os.path.join(HERE, "fairness_loss.json"), "w"), indent=1, sort_keys=True)
    print("wrote", os.path.join(HERE, "fairness_loss.json"))


if __name__ == "__main__":
    main()
