#!/usr/bin/env python
"""Generate tests/golden/optim.npz + optim.json by IMPORTING the reference's build_optimizer / build_lr_scheduler
(Dassl/dassl/optim/optimizer.py:13-142, lr_scheduler.py:83-155), the way make_golden.py imports the reference.

Runs only where the reference tree is (make_golden.REF).  The outputs are data: recorded parameter trajectories and
learning-rate sequences.  The tests read the two files and never this script.

Optimizers (all six of AVAI_OPTIMS): one parameter vector of 4096 float32 values, a fixed sequence of 8 gradients ~N(0, 1e-3)
with one element in seven exactly zero, TWO optimizer steps per gradient (the reference's shared optimizer is stepped once
per registered model name, Dassl/dassl/engine/trainer.py:333-337), the parameters after every gradient, for weight decay 0
and 5e-4.  RAdam's 16 steps cross its N_sma >= 5 switch at beta2 = 0.999 (asserted below).

To keep the files small the trajectories are stored LOSSLESSLY as differences of the float32 bit patterns between
consecutive rows (row 0 against the initial parameters; the second weight decay's differences against the first's), split
into their four byte planes: `decode` below (restated in the test) adds them back up.

Schedulers: the LR after each of 24 step() calls for every scheduler x warm-up combination of SCHEDS x WARMUPS and
MAX_EPOCH in {1, 5}.  A combination the reference itself cannot step (CosineAnnealingLR entered at an odd multiple of T_max
by WARMUP_RECOUNT = False divides by zero) is recorded as {"error": "ZeroDivisionError", "lrs": [... up to the failure]}.

The installed torch dropped the `verbose` argument of LRScheduler.__init__, which Dassl's warm-up wrappers still pass
positionally; a three-line base class that swallows it is put under them here - nothing else of the reference is touched.
"""
from __future__ import annotations

import json
import os
import sys
import warnings
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF      # noqa: E402

N, GRADS, STEPS_PER_GRAD, NSCHED = 4096, 8, 2, 24
LR, WDS = 1e-3, (0.0, 5e-4)
OPTIMS = ["sgd", "adam", "adamw", "amsgrad", "rmsprop", "radam"]
SCHEDS = {"single_step": ("single_step", 4), "single_step_max_epoch": ("single_step", (-1,)),
          "multi_step": ("multi_step", [3, 7, 7, 12]), "cosine": ("cosine", (-1,))}
WARMUPS = {"none": dict(WARMUP_EPOCH=-1), "constant2": dict(WARMUP_EPOCH=2, WARMUP_TYPE="constant"),
           "linear3": dict(WARMUP_EPOCH=3, WARMUP_TYPE="linear"),
           "constant2_norecount": dict(WARMUP_EPOCH=2, WARMUP_TYPE="constant", WARMUP_RECOUNT=False),
           "linear3_norecount": dict(WARMUP_EPOCH=3, WARMUP_TYPE="linear", WARMUP_RECOUNT=False)}


def optim_cfg(**kw):
    """Dassl/dassl/config/defaults.py's OPTIM node, the keys the two builders read."""
    base = dict(NAME="sgd", LR=LR, WEIGHT_DECAY=5e-4, MOMENTUM=0.9, SGD_DAMPNING=0, SGD_NESTEROV=False, RMSPROP_ALPHA=0.99,
                ADAM_BETA1=0.9, ADAM_BETA2=0.999, STAGED_LR=False, NEW_LAYERS=(), BASE_LR_MULT=0.1,
                LR_SCHEDULER="single_step", STEPSIZE=(-1,), GAMMA=0.1, MAX_EPOCH=10, WARMUP_EPOCH=-1, WARMUP_TYPE="linear",
                WARMUP_CONS_LR=1e-5, WARMUP_MIN_LR=1e-5, WARMUP_RECOUNT=True)
    base.update(kw)
    return NS(**base)


def import_builders():
    sys.path.insert(0, os.path.join(REF, "Dassl"))
    import dassl.optim.lr_scheduler as RL
    from dassl.optim.optimizer import build_optimizer

    class _TakesVerbose(torch.optim.lr_scheduler.LRScheduler):
        def __init__(self, optimizer, last_epoch=-1, verbose=False):
            super().__init__(optimizer, last_epoch)

    RL._BaseWarmupScheduler.__bases__ = (_TakesVerbose,)
    return build_optimizer, RL.build_lr_scheduler


def _planes(d: np.ndarray) -> np.ndarray:
    """[rows, N] int32 -> [rows, 4, N] uint8 byte planes (the high planes are mostly zero and compress away)."""
    d = np.ascontiguousarray(d.astype(np.int32))
    return np.ascontiguousarray(d.view(np.uint8).reshape(d.shape[0], N, 4).transpose(0, 2, 1))


def _unplanes(planes: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(planes.transpose(0, 2, 1)).view(np.int32).reshape(planes.shape[0], N).astype(np.int64)


def row_diffs(p0: np.ndarray, traj: np.ndarray) -> np.ndarray:
    """int64 differences between the float32 bit patterns of consecutive rows (row 0 against p0)."""
    return np.diff(np.concatenate([p0[None], traj]).view(np.int32).astype(np.int64), axis=0)


def from_diffs(p0: np.ndarray, d: np.ndarray) -> np.ndarray:
    return (p0.view(np.int32).astype(np.int64)[None] + np.cumsum(d, axis=0)).astype(np.int32).view(np.float32)


def decode(p0: np.ndarray, z, name: str):
    """The two trajectories (weight decay WDS[0], WDS[1]) of optimizer `name`: `<name>.wd0` holds the row differences of
    the first, `<name>.wd1` the second's row differences MINUS the first's."""
    d0 = _unplanes(z[f"{name}.wd0"])
    return from_diffs(p0, d0), from_diffs(p0, d0 + _unplanes(z[f"{name}.wd1"]))


def main():
    build_optimizer, build_lr_scheduler = import_builders()
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(20240607)
    p0 = rng.standard_normal(N).astype(np.float32)
    g = (rng.standard_normal((GRADS, N)) * 1e-3).astype(np.float32)
    g[:, ::7] = 0.0
    out = {"p0": p0, "g": g}
    meta = {"n": N, "grads": GRADS, "steps_per_grad": STEPS_PER_GRAD, "lr": LR, "wds": list(WDS), "optims": OPTIMS,
            "hyper": {"momentum": 0.9, "alpha": 0.99, "beta1": 0.9, "beta2": 0.999}, "torch": torch.__version__}
    for name in OPTIMS:
        for wi, wd in enumerate(WDS):
            p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
            opt = build_optimizer([p], optim_cfg(NAME=name, WEIGHT_DECAY=wd))
            rows, nsma = [], []
            for k in range(GRADS):
                p.grad = torch.from_numpy(g[k].copy())
                for _ in range(STEPS_PER_GRAD):
                    opt.step()
                    if name == "radam":           # the [step, N_sma, step_size] entry this step filled or reused
                        b = opt.buffer[opt.state[p]["step"] % 10]
                        nsma.append((b[0], b[1]))
                rows.append(p.detach().numpy().copy())
            traj = np.stack(rows)
            d = row_diffs(p0, traj)
            out[f"{name}.wd{wi}"] = _planes(d if wi == 0 else d - d_first)
            d_first = d if wi == 0 else d_first
            assert np.array_equal(decode(p0, out, name)[wi].view(np.int32), traj.view(np.int32)) if wi else True
            if name == "radam":
                assert [t for t, _ in nsma] == list(range(1, GRADS * STEPS_PER_GRAD + 1))
                assert min(n for _, n in nsma) < 5 <= max(n for _, n in nsma), "both RAdam branches must be taken"
                assert opt.state[p]["step"] == GRADS * STEPS_PER_GRAD
                meta["radam_nsma"] = [[int(t), float(n)] for t, n in nsma]
    sched = {}
    for sname, (kind, stepsize) in SCHEDS.items():
        for wname, wkw in WARMUPS.items():
            for max_epoch in (1, 5):
                p = torch.nn.Parameter(torch.zeros(1))
                cfg = optim_cfg(NAME="sgd", LR=2e-3, LR_SCHEDULER=kind, STEPSIZE=stepsize, MAX_EPOCH=max_epoch, **wkw)
                opt = build_optimizer([p], cfg)
                s = build_lr_scheduler(opt, cfg)
                rec = {"kind": kind, "stepsize": list(stepsize) if isinstance(stepsize, (list, tuple)) else stepsize,
                       "max_epoch": max_epoch, "lr": 2e-3, "gamma": 0.1, "warmup": wkw, "lr0": opt.param_groups[0]["lr"],
                       "lrs": []}
                try:
                    for _ in range(NSCHED):
                        opt.step()
                        s.step()
                        rec["lrs"].append(float(opt.param_groups[0]["lr"]))
                except ZeroDivisionError:
                    rec["error"] = "ZeroDivisionError"
                sched[f"{sname}|{wname}|{max_epoch}"] = rec
    meta["sched"] = sched
    meta["sched_steps"] = NSCHED
    np.savez_compressed(os.path.join(HERE, "optim.npz"), **out)
    with open(os.path.join(HERE, "optim.json"), "w") as f:
        json.dump(meta, f, indent=1)
    tot = sum(os.path.getsize(os.path.join(HERE, n)) for n in ("optim.npz", "optim.json"))
    print(f"optim.npz + optim.json: {tot} bytes;", sum("error" in r for r in sched.values()), "combinations the reference cannot step")
    assert tot < 1_000_000


if __name__ == "__main__":
    main()
