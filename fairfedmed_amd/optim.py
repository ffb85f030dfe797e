"""The optimizer and LR-schedule surface of cfg.OPTIM, on the host (no GPU needed to import or to run this module).

`build_optim_spec` / `build_lr_schedule` read what the reference's build_optimizer (Dassl/dassl/optim/optimizer.py:13-142)
and build_lr_scheduler (Dassl/dassl/optim/lr_scheduler.py:83-155) read, every key with its Dassl default, and raise the
same ValueError texts for names they do not know.

OptimSpec is the small host object the engines take (kind, betas, eps, alpha, momentum, weight decay): it fills the
ffm_optim_desc of an optimizer step (include/ffm_hip.h) and keeps beta1^t / beta2^t as RUNNING PRODUCTS, one double
multiplication per application and never a pow(), which is how the device-side counter block of a captured step advances
them too - the two stay bit-identical.

LRSchedule restates torch's StepLR / MultiStepLR / CosineAnnealingLR and Dassl's constant / linear warm-up wrappers as
one stateful host object over the shared parameter group's ``lr``.  StepLR and MultiStepLR use the closed forms (what the
trainer has always computed for single_step); CosineAnnealingLR is torch's recursive, chainable form, branch at
(last_epoch - 1 - T_max) % (2 T_max) == 0 included: the federated loop runs MAX_EPOCH = 1 per train() call on a scheduler
that lives across clients and rounds, so last_epoch runs far past T_max, where the closed form is NOT what torch computes.
"""
from __future__ import annotations

import bisect
import math
from dataclasses import dataclass, field
from typing import List, Tuple

AVAI_OPTIMS = ["adam", "amsgrad", "sgd", "rmsprop", "radam", "adamw"]
AVAI_SCHEDS = ["single_step", "multi_step", "cosine"]
AVAI_WARMUPS = ["constant", "linear"]


# ------------------------------------------------------------------------------------------------------ optimizer ---
@dataclass
class OptimSpec:
    kind: str = "sgd"
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8              # the default of torch.optim.Adam / AdamW / RMSprop and of the reference's RAdam
    alpha: float = 0.99
    momentum: float = 0.9
    weight_decay: float = 5e-4
    _at: List[float] = field(default_factory=lambda: [0, 1.0, 1.0], repr=False, compare=False)

    def __post_init__(self):
        if self.kind not in AVAI_OPTIMS:
            raise ValueError(f"optim must be one of {AVAI_OPTIMS}, but got {self.kind}")

    @property
    def rows(self) -> int:
        """Rows of the [K, numel] state tensor (what ffm_optim_state_rows answers)."""
        return {"sgd": 1, "amsgrad": 3}.get(self.kind, 2)

    def powers(self, steps: int) -> Tuple[float, float]:
        """(beta1^steps, beta2^steps) as running products from 1.0, memoised at the last position asked for."""
        t, p1, p2 = self._at
        if steps < t:
            t, p1, p2 = 0, 1.0, 1.0
        while t < steps:
            p1, p2, t = p1 * self.beta1, p2 * self.beta2, t + 1
        self._at[:] = [t, p1, p2]
        return p1, p2

    def desc_values(self, lr: float, steps: int) -> List[float]:
        """The ten doubles of ffm_optim_desc after `steps` applications."""
        p1, p2 = self.powers(int(steps))
        return [float(lr), float(self.beta1), float(self.beta2), float(self.eps), float(self.alpha), float(self.momentum),
                float(self.weight_decay), p1, p2, float(int(steps))]

    def desc(self, lr: float, steps: int):
        from . import _lib
        return _lib.OptimDesc(*self.desc_values(lr, steps))


def build_optim_spec(optim_cfg) -> OptimSpec:
    """OPTIM.NAME / ADAM_BETA1 / ADAM_BETA2 / RMSPROP_ALPHA / MOMENTUM / WEIGHT_DECAY -> OptimSpec (Dassl defaults)."""
    o = optim_cfg
    return OptimSpec(kind=getattr(o, "NAME", "sgd"), beta1=getattr(o, "ADAM_BETA1", 0.9), beta2=getattr(o, "ADAM_BETA2", 0.999),
                     alpha=getattr(o, "RMSPROP_ALPHA", 0.99), momentum=getattr(o, "MOMENTUM", 0.9),
                     weight_decay=getattr(o, "WEIGHT_DECAY", 5e-4))


# ------------------------------------------------------------------------------------------------------- schedule ---
class LRSchedule:
    """The scheduler build_lr_scheduler returns, over ``group["lr"]``.  ``step()`` is scheduler.step(); ``last_epoch``
    counts the step() calls (for a plain scheduler, torch's last_epoch).  With a warm-up of W epochs the first W calls step
    the wrapper and every later one the successor, which starts at last_epoch 0 (WARMUP_RECOUNT) or W."""

    def __init__(self, group: dict, name: str = "single_step", stepsize=0, gamma: float = 0.1, max_epoch: int = 1,
                 warmup_epoch: int = -1, warmup_type: str = "linear", cons_lr: float = 1e-5, min_lr: float = 1e-5,
                 recount: bool = True):
        if name not in AVAI_SCHEDS:
            raise ValueError(f"scheduler must be one of {AVAI_SCHEDS}, but got {name}")
        if name == "single_step":
            if isinstance(stepsize, (list, tuple)):
                stepsize = stepsize[-1]
            if stepsize <= 0:
                stepsize = max_epoch
        elif name == "multi_step":
            if not isinstance(stepsize, (list, tuple)):
                raise TypeError(f"For multi_step lr_scheduler, stepsize must be a list, but got {type(stepsize)}")
            stepsize = sorted(stepsize)
        if warmup_epoch > 0 and warmup_type not in AVAI_WARMUPS:
            raise ValueError(f"warmup type must be one of {AVAI_WARMUPS}, but got {warmup_type}")
        self.group, self.name, self.stepsize, self.gamma = group, name, stepsize, gamma
        self.t_max = float(max_epoch)
        self.warmup_epoch, self.warmup_type, self.cons_lr, self.min_lr = int(warmup_epoch), warmup_type, cons_lr, min_lr
        self.recount = bool(recount)
        self.base_lr = group["lr"]
        self.reset()

    def reset(self) -> None:
        W = self.warmup_epoch
        self.last_epoch = 0                       # step() calls so far
        self._w = 0                               # the warm-up wrapper's last_epoch
        self._s0 = W if (W > 0 and not self.recount) else 0       # the successor's first last_epoch (lr_scheduler.py:136-138)
        self._s = self._s0
        lr = self.base_lr
        if W > 0:
            lr = self.cons_lr if self.warmup_type == "constant" else self.min_lr
        self.group["lr"] = lr

    @property
    def lr(self) -> float:
        return self.group["lr"]

    def _successor(self, lr: float) -> float:
        s, base = self._s, self.base_lr
        # (the decays torch's chainable form has applied: those of the epochs stepped INTO, i.e. after the start s0, which
        # WARMUP_RECOUNT = False moves to the warm-up length - a milestone at or before it never takes effect)
        s0 = self._s0
        if self.name == "single_step":
            return base * self.gamma ** (s // self.stepsize - s0 // self.stepsize)
        if self.name == "multi_step":
            return base * self.gamma ** (bisect.bisect_right(self.stepsize, s) - bisect.bisect_right(self.stepsize, s0))
        T = self.t_max                            # CosineAnnealingLR(T_max=float(MAX_EPOCH), eta_min=0), chainable form
        if (s - 1 - T) % (2 * T) == 0:
            return lr + base * (1 - math.cos(math.pi / T)) / 2
        return (1 + math.cos(math.pi * s / T)) / (1 + math.cos(math.pi * (s - 1) / T)) * lr

    def step(self) -> float:
        W = self.warmup_epoch
        self.last_epoch += 1
        if W > 0 and self._w < W:
            self._w += 1
            if self._w >= W:
                lr = self.base_lr                 # successor.get_last_lr(): its initial value
            elif self.warmup_type == "constant":
                lr = self.cons_lr
            else:
                lr = self.base_lr * self._w / W
        else:
            self._s += 1
            lr = self._successor(self.group["lr"])
        self.group["lr"] = lr
        return lr

    def set_lr_epoch(self, n: int) -> float:
        """Position the schedule as after `n` step() calls by replaying them from zero (exact, and a few dozen flops)."""
        self.reset()
        for _ in range(int(n)):
            self.step()
        return self.group["lr"]


def build_lr_schedule(group: dict, optim_cfg) -> LRSchedule:
    """OPTIM.LR_SCHEDULER / STEPSIZE / GAMMA / MAX_EPOCH / WARMUP_* -> LRSchedule over `group` (Dassl defaults)."""
    o = optim_cfg
    return LRSchedule(group, name=getattr(o, "LR_SCHEDULER", "single_step"), stepsize=getattr(o, "STEPSIZE", (-1,)),
                      gamma=getattr(o, "GAMMA", 0.1), max_epoch=o.MAX_EPOCH, warmup_epoch=getattr(o, "WARMUP_EPOCH", -1),
                      warmup_type=getattr(o, "WARMUP_TYPE", "linear"), cons_lr=getattr(o, "WARMUP_CONS_LR", 1e-5),
                      min_lr=getattr(o, "WARMUP_MIN_LR", 1e-5), recount=getattr(o, "WARMUP_RECOUNT", True))
