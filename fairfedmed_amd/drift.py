"""Client-drift correction in the local step (an extension beyond the reference, whose FedOTPLoRA
branch runs plain FedAvg): FedProx's proximal pull and SCAFFOLD's control variates on the flat gradient buffer, between the
backward pass and the optimizer launch.  On a GPU the correction is one launch of ffm_drift_correct (csrc/drift.hip); for CPU
tensors (the gloo plumbing configuration, and the twin the GPU tests compare against) ``host_correct`` performs the same
fp32 operations in the same order.

Per local step, for every element of the flat buffer, each line one rounded fp32 operation::

    raw = g
    scaffold:  gsum = gsum + raw;  count += 1 (once per step)
    fedprox:   d = p - anchor;  t = mu * d;  g = raw + t          anchor: the weights the client started the round from
    scaffold:  g = raw + c_diff                                   c_diff = c - c_i, formed once per client-round

Per client-round (scaffold): c_i' = gsum / count, the mean raw gradient along the local trajectory.  For plain SGD this is
SCAFFOLD's option II, c_i - c + (x - y_i) / (K lr) (Karimireddy et al. 2020), written without a learning rate, so that it stays
defined under momentum, Adam and an optimizer that is stepped twice per batch.  Per round, on all ranks identically and in
ascending client order: c = c + (c_i' - c_i) / N with N the number of clients, then c_i = c_i'.

The reported loss stays the task loss (the reference's FedProx baselines add (mu / 2) |p - anchor|^2 to the printed loss; here
only the gradient carries the term), and weight decay stays inside the optimizer kernels.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch
import torch.distributed as dist

Tensor = torch.Tensor

NAMES = ("none", "fedprox", "scaffold")


@dataclass(frozen=True)
class DriftCfg:
    name: str = "none"                # none | fedprox | scaffold
    mu: float = 0.0                   # fedprox: the weight of the proximal term (the reference's --mu); unused otherwise

    def __post_init__(self):
        if self.name not in NAMES:
            raise ValueError(f"DriftCfg.name must be one of {NAMES} (got {self.name!r})")
        if self.name == "fedprox" and not (math.isfinite(self.mu) and self.mu >= 0):
            raise ValueError(f"DriftCfg.mu must be a finite number >= 0 (got {self.mu})")


@torch.no_grad()
def host_correct(g: Tensor, p: Optional[Tensor] = None, anchor: Optional[Tensor] = None, mu: float = 0.0,
                 c_diff: Optional[Tensor] = None, gsum: Optional[Tensor] = None, count: Optional[Tensor] = None,
                 scale_state: Optional[Tensor] = None) -> None:
    """ffm_drift_correct for CPU tensors: the same operands, the same fp32 operations in the same order, in place."""
    if scale_state is not None and float(scale_state[2]) == 0.0:
        return                                              # the step overflowed: nothing moves
    if gsum is not None:
        gsum.add_(g)                                        # the raw gradient
        count.add_(1)
    if anchor is not None:
        d = torch.sub(p, anchor)
        t = torch.mul(d, torch.tensor(mu, dtype=torch.float32))
        g.add_(t)
    if c_diff is not None:
        g.add_(c_diff)


class DriftCorrector:
    """The state of one run's drift correction over the flat trainable buffer ``flat`` of ``users`` clients.

    Every tensor is fp32 (``count``: int64 [1]) on ``flat``'s device, zero at construction and allocated once, so that a
    captured training step keeps valid addresses: ``anchor``, ``c_diff``, ``gsum`` [n], the global control variate ``c`` [n]
    and the per-client table ``c_i`` [users, n] (30 MB at 10 users x 742 k elements).

    A round: for each client this rank trains, ``begin_client(idx)`` once its starting weights are in ``flat``, the local
    steps (the engine calls ``apply`` at the end of every forward_backward after ``ClipEngine.set_drift``), ``end_client(idx)``;
    then ``finish_round(participants)`` on ALL ranks, behind the aggregator's ``finish``."""

    def __init__(self, flat: Tensor, users: int, cfg: DriftCfg, group=None):
        if flat.dtype != torch.float32 or flat.dim() != 1 or not flat.is_contiguous():
            raise TypeError("DriftCorrector needs the contiguous fp32 flat buffer")
        self.flat, self.users, self.cfg, self.group = flat, int(users), cfg, group
        n = flat.numel()
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=flat.device)
        self.anchor, self.c_diff, self.gsum, self.c = z(n), z(n), z(n), z(n)
        self.count = z(1, dt=torch.int64)
        self.c_i = z(self.users, n)
        scaffold = cfg.name == "scaffold"
        # this round's new rows and their step counts, zero-padded: one all_reduce(SUM) each hands them to every rank
        self._rows = z(self.users, n) if scaffold else None
        self._steps = z(self.users, dt=torch.int64) if scaffold else None

    def live(self) -> List[Tensor]:
        """What ``apply`` writes besides the gradient (a captured step's warm-up runs restore these)."""
        return [self.gsum, self.count] if self.cfg.name == "scaffold" else []

    @torch.no_grad()
    def begin_client(self, idx: int) -> None:
        if self.cfg.name == "fedprox":
            self.anchor.copy_(self.flat)
        elif self.cfg.name == "scaffold":
            torch.sub(self.c, self.c_i[idx], out=self.c_diff)
            self.gsum.zero_()
            self.count.zero_()

    @torch.no_grad()
    def apply(self, grad: Tensor, flat: Tensor, scale_state: Optional[Tensor] = None) -> None:
        """Correct ``grad`` in place: one launch on a GPU, the host twin on the CPU; nothing with ``none``."""
        name = self.cfg.name
        if name == "none":
            return
        if name == "fedprox":
            kw = dict(p=flat, anchor=self.anchor, mu=self.cfg.mu)
        else:
            kw = dict(c_diff=self.c_diff, gsum=self.gsum, count=self.count)
        if grad.is_cuda:
            from . import ops
            ops.drift_correct(grad, scale_state=scale_state, **kw)
        else:
            host_correct(grad, scale_state=scale_state, **kw)

    @torch.no_grad()
    def end_client(self, idx: int) -> None:
        """scaffold: the client's new control variate, gsum / count, into this round's rows.  Reading ``count`` is the one
        host sync per client-round; a client that made no (unskipped) step keeps its row."""
        if self.cfg.name != "scaffold":
            return
        k = int(self.count)
        if k > 0:
            torch.div(self.gsum, torch.tensor(float(k), dtype=torch.float32, device=self.gsum.device), out=self._rows[idx])
            self._steps[idx] = k

    @torch.no_grad()
    def finish_round(self, participants: Sequence[int]) -> Dict[str, object]:
        """All ranks, once per round.  Exactly one rank contributes each new row, so the all-reduced sum is exact; the update
        of ``c`` then runs in ascending client order on every rank.  Returns {"c_norm", "steps": {client: steps}}."""
        out: Dict[str, object] = {"c_norm": 0.0, "steps": {}}
        if self.cfg.name != "scaffold":
            return out
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self._rows, op=dist.ReduceOp.SUM, group=self.group)
            dist.all_reduce(self._steps, op=dist.ReduceOp.SUM, group=self.group)
        steps = self._steps.tolist()
        inv = torch.tensor(float(self.users), dtype=torch.float32, device=self.c.device)
        for i in sorted(set(int(u) for u in participants)):
            out["steps"][i] = int(steps[i])
            if steps[i] > 0:
                self.c.add_(torch.sub(self._rows[i], self.c_i[i]).div_(inv))
                self.c_i[i].copy_(self._rows[i])
        self._rows.zero_()
        self._steps.zero_()
        out["c_norm"] = float(self.c.norm())
        return out
