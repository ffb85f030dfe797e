"""One (Fair)LoRA-wrapped linear of either image tower: everything the engines know about it, in one object."""
from __future__ import annotations

from typing import TYPE_CHECKING, Optional, Tuple

import torch

from . import _lib as L
from . import ops

if TYPE_CHECKING:
    from .engine import ClipEngine

Tensor = torch.Tensor


class LoraSite:
    """One adapted linear over token / pixel rows: y = x W^T (+b) + scaling ((x A) * s_b) B, K -> N features.
    fair=False is the reference's LoRALinear (:218-241): the same update with s = 1 and no groups.

    It owns its flat-buffer keys and the views behind them, its prefix in the engine's SOperands, the saved rank vectors
    t / ts (forward) and u / us (backward), the partial sums pA / pB / pS of its gradients and - rank <= 16, the down
    projections inside the GEMMs (FFM_EPI_RANKOP) - A and B re-packed to [16, K] / [16, N] in the compute dtype, with
      wide      their [K, 32] / [N, 32] copies too: the `lw` operand of the GEMM whose OUTPUT columns they span;
      ln        (gamma, beta) of a LayerNorm folded into the forward product: rkA_ln, its [2, 16] corrections lnrk;
      row1415   two vectors as rows 14 / 15 of rkB (rank <= 14): the dX product's t[14] / t[15] are the row sums against them.
    The towers pass in what differs: the rows to size for, a shared `u`, the floats of pS (alloc_ds), and the t / ts a
    forward product writes (the evaluation pass keeps one pair for all layers).  fwd / bwd are the adapted products of
    both towers: the rank operands above around the caller's GEMM and its epilogue keywords."""

    def __init__(self, eng: "ClipEngine", prefix: str, K: int, N: int, max_rows: int, fair: bool = True, u: Optional[Tensor] = None,
                 wide: bool = False, ln: Optional[Tuple[Tensor, Tensor]] = None,
                 row1415: Optional[Tuple[Tensor, Tensor]] = None):
        self.eng, self.prefix, self.K, self.N, self.fair = eng, prefix, K, N, fair
        self.kA, self.kB = prefix + "lora_A.weight", prefix + "lora_B.weight"
        self.kS = prefix + "lora_S.weight" if fair else None
        p, dt, dev = eng.params, eng.dtype, eng.device
        self.A, self.B, self.gA, self.gB = p.view(self.kA), p.view(self.kB), p.view(self.kA, "grad"), p.view(self.kB, "grad")
        self.rank = r = eng.cfg.lora.rank
        f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        e = lambda *s: torch.zeros(*s, device=dev, dtype=dt)
        self.t, self.ts = f(max_rows, r), f(max_rows, r)
        self.u, self.us = f(max_rows, r) if u is None else u, f(max_rows, r)
        ns = ops.lora_grad_splits(max_rows)
        self.pA, self.pB, self.pS = f(ns * K * r), f(ns * N * r), None
        self.fused = 0 < r <= 16
        self.rkA = self.rkB = self.wA = self.wB = self.rkA_ln = self.lnrk = None
        self.ln, self.row1415 = ln, row1415
        if self.fused:
            self.rkA, self.rkB = e(16, K), e(16, N)
            if wide:
                self.wA, self.wB = e(K, 32), e(N, 32)
            if ln is not None:
                self.rkA_ln, self.lnrk = e(16, K), f(32)

    def alloc_ds(self, floats: int) -> None:
        self.pS = torch.zeros(floats, device=self.eng.device, dtype=torch.float32)

    def pack_entries(self) -> list:
        """ops.PackPlan entries [A, B(, A folded with its LayerNorm)] of a fused site."""
        ent = [(self.A, False, self.rkA, self.wA, None, None), (self.B, True, self.rkB, self.wB, None, self.row1415)]
        if self.ln is not None:
            ent.append((self.A, False, self.rkA_ln, None, (self.ln[0], self.ln[1], self.lnrk)))
        return ent

    def ds_tiles(self, rows: int, packed: bool = False, dgelu: bool = False) -> int:
        """dS partial rows the dX GEMM (M = rows, N = in features, K = out features) writes."""
        fl = L.EPI_LORA | L.EPI_LORA_KR | L.EPI_RANKOP | (L.EPI_DGELU if dgelu else 0)
        return ops.gemm_tiles_m(rows, self.K, self.N, fl, self.rank, self.eng.dtype, packed)

    def ds_rows(self, rows: int, packed: bool = False, dgelu: bool = False, gemm: bool = True) -> int:
        """dS partial rows to reduce over: the dX GEMM's row tiles (fused, and the GEMM runs), else ffm_lora_down's blocks."""
        if self.fused and gemm:
            return self.ds_tiles(rows, packed, dgelu)
        return ops.lora_down_blocks(rows, self.N, self.rank, self.eng.dtype)

    def _tail(self, attr: Optional[Tensor], rps: int) -> tuple:
        """(S, attr, G) and the (rows per sample, scaling, lambda) every rank product of this site takes."""
        e, lo = self.eng, self.eng.cfg.lora
        S, G = (e.sops.op(self.prefix), lo.num_groups) if self.fair else (e.ones_s, 1)
        return S, (attr if self.fair else None), G, (rps, lo.scaling, lo.lambda_group)

    # -- rank <= 16: the operands of FFM_EPI_RANKOP ------------------------------------------------------------
    def rank_fwd(self, attr: Optional[Tensor], rps: int, t: Optional[Tensor], ts: Optional[Tensor],
                 ln: bool = False) -> ops.RankOp:
        """The forward product's x A, t / ts into the caller's vectors (ln: x raw, its LayerNorm folded into the product)."""
        S, attr, _, tail = self._tail(attr, rps)
        return ops.RankOp(self.rkA_ln if ln else self.rkA, S, attr, *tail, t_out=t, ts_out=ts, lw_wide=self.wB)

    def rank_bwd(self, attr: Optional[Tensor], rps: int, rows: int, lgrad: Optional[tuple] = None) -> ops.RankOp:
        """The dX product's u = g B^T: us and the dS partials into the site's own buffers; lgrad: ops.RankOp.lgrad."""
        S, attr, _, tail = self._tail(attr, rps)
        return ops.RankOp(self.rkB, S, attr, *tail, ts_out=self.us[:rows], t_fwd=self.t[:rows] if self.fair else None,
                          ds_part=self.pS, lw_wide=self.wA, lgrad=lgrad)

    # -- rank > 16: ffm_lora_down in front of the product ------------------------------------------------------
    def down_fwd(self, x: Tensor, attr: Optional[Tensor], rps: int, t: Tensor, ts: Tensor) -> None:
        S, attr, G, tail = self._tail(attr, rps)
        ops.lora_down(x, self.A, False, S, attr, self.rank, G, *tail, t, ts)

    def down_bwd(self, g: Tensor, attr: Optional[Tensor], rps: int) -> None:
        S, attr, G, tail = self._tail(attr, rps)
        u, us, t = (b[:g.shape[0]] for b in (self.u, self.us, self.t))
        ops.lora_down(g, self.B, True, S, attr, self.rank, G, *tail, u, us, t if self.fair else None, self.pS)

    # -- the adapted product: the down projection inside the GEMM, or in front of it ----------------------------
    # what the rank > 16 arm hands its GEMM of the caller's epilogue keywords: the kernels that serve `ts=` take no
    # packed weight, no LayerNorm fold and no BatchNorm-backward sums
    _PLAIN = ("bias", "res", "gelu_out", "gelu_only", "dgelu_aux", "colstats")

    def fwd(self, x: Tensor, W: Tensor, out: Tensor, attr: Optional[Tensor], rps: int, gemm=None,
            tts: Optional[Tuple[Optional[Tensor], Optional[Tensor]]] = None, ln: bool = False, **k) -> None:
        """out = x W^T + the adapter's term, through `gemm` (default: ops.gemm_nt, looked up at the call as every caller of
        it does - the benchmark's timing wrapper replaces it; k: its epilogue keywords).
        tts: the (t, ts) the product writes (default: the site's own); ln: x raw, its LayerNorm folded in (k: ln_in)."""
        t, ts = (self.t[:x.shape[0]], self.ts[:x.shape[0]]) if tts is None else tts
        gemm = gemm or ops.gemm_nt
        if self.fused:
            gemm(x, W, out, lw=self.B, rankop=self.rank_fwd(attr, rps, t, ts, ln=ln), **k)
            return
        self.down_fwd(x, attr, rps, t, ts)
        gemm(x, W, out, ts=ts, lw=self.B, **{n: k[n] for n in self._PLAIN if n in k})

    def bwd(self, g: Tensor, Wt: Tensor, dx: Tensor, attr: Optional[Tensor], rps: int, gemm=None,
            lgrad: Optional[tuple] = None, down: bool = True, **k) -> None:
        """g = dL/dy; writes dx = g W (+ the adapter's term) and us, the partial sums of dS; the caller runs the two
        reductions (dA, dB) itself, on the gradient stream.  lgrad: ops.RankOp.lgrad.  down=False (rank > 16): the caller
        has run down_bwd already, with launches of its own between the two."""
        gemm = gemm or ops.gemm_nt
        if self.fused:
            gemm(g, Wt, dx, lw=self.A, lw_is_kr=True, rankop=self.rank_bwd(attr, rps, g.shape[0], lgrad), **k)
            return
        assert k.get("bnbwd") is None and lgrad is None
        if down:
            self.down_bwd(g, attr, rps)
        gemm(g, Wt, dx, ts=self.us[:g.shape[0]], lw=self.A, lw_is_kr=True, **{n: k[n] for n in self._PLAIN if n in k})

    # -- the rank-r gradient reductions (partials) and their sum ------------------------------------------------
    def grad_B(self, g: Tensor) -> None:
        """dB = g^T ts."""
        ops.lora_grad_partial(g, self.ts[:g.shape[0]], self.rank, self.pB)

    def grad_A(self, x: Tensor, ln_stats: Optional[Tuple[Tensor, Tensor]] = None) -> None:
        """dA = x^T us; ln_stats (mean, rstd): x holds the RAW rows of the LayerNorm that was folded into the product."""
        us = self.us[:x.shape[0]]
        if ln_stats is not None:
            ops.lora_grad_partial_ln(x, us, ln_stats[0], ln_stats[1], self.ln[0], self.ln[1], self.rank, self.pA)
        else:
            ops.lora_grad_partial(x, us, self.rank, self.pA)

    def reduce_entries(self, rows: int, ds_rows: Optional[int] = None, splits_A: Optional[int] = None,
                       splits_B: Optional[int] = None) -> list:
        """ops.ReducePlan entries [dB, dA(, dS)] that sum the partials into params.grad.  ds_rows: partial rows of dS (default:
        ds_rows(rows)); splits_A / splits_B: those of dA / dB where not the site's own reduction left them (FFM_EPI_LGRAD)."""
        r, nsp = self.rank, ops.lora_grad_splits(rows)
        ent = [(self.pB, splits_B or nsp, self.N * r, self.gB, self.N, r), (self.pA, splits_A or nsp, self.K * r, self.gA, 0, 0)]
        if self.fair:
            nb = self.ds_rows(rows) if ds_rows is None else ds_rows
            ent.append((self.pS, nb, self.eng.cfg.lora.num_groups * r, self.eng.sops.grad(self.prefix), 0, 0))
        return ent
