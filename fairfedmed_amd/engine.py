"""FairLoRA local-training engine: one training step of the reference's
``GLP_OT_SVLoRA.forward_backward`` (trainers/GLP_OT_SVLoRA.py:883-975) as a
fixed sequence of HIP kernel launches over preallocated HBM buffers.

Data layout in HBM (all row-major):
  * token matrices [rows, width], row = image*L + token (image-major);
  * frozen weights twice, in the compute dtype: W [out, in] for the forward
    product and W^T [in, out] for the dX product (both are the "B[N,K]" operand
    of ffm_gemm_nt, K contiguous) — weights are frozen so W^T is built once;
  * every trainable tensor (prompt ctx, lora_A/S/B of the 24 wrapped linears)
    is a view into ONE flat fp32 buffer `flat`, with matching `grad` and
    `momentum` buffers: the SGD step is one kernel and the FedAvg exchange is
    one all-reduce of `flat`;
  * activations saved for the backward pass live in per-layer buffers sized
    once for `max_images` (no allocation inside a step).

Backward computes dX only (every dense weight is frozen): LoRA gradients come
from rank-r reductions (ffm_lora_grad_partial) and the LoRA dx term is an
epilogue of the dX GEMM, so the dense dW = A diag(s) B is never formed.
"""
from __future__ import annotations

import contextlib
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from ._lib import is16 as _is16
from . import ops
from .config import ModelCfg
from .data import NativeBatch
from .lora_site import LoraSite
from .synth import manifest, trainable_keys

Tensor = torch.Tensor


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class FlatParams:
    """All trainable tensors as views of one flat fp32 buffer (+ grad, momentum)."""

    def __init__(self, cfg: ModelCfg, device):
        shapes = manifest(cfg)
        self.keys = trainable_keys(cfg)
        self.offsets: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        off = 0
        for k in self.keys:
            shp = tuple(shapes[k])
            n = 1
            for s in shp:
                n *= s
            self.offsets[k] = (off, shp)
            off = _round_up(off + n, 4)
        self.numel = off
        self.flat = torch.zeros(off, device=device, dtype=torch.float32)
        self.grad = torch.zeros(off, device=device, dtype=torch.float32)
        # optimizer state: rows of one [K, numel] tensor (K = ffm_optim_state_rows: 1 for SGD - exactly this allocation -
        # 2 for adam / adamw / rmsprop / radam, 3 for amsgrad); `momentum` is always the row-0 view
        self.optim_state = torch.zeros(1, off, device=device, dtype=torch.float32)
        self.momentum = self.optim_state[0]
        self.optim_desc: Optional[Tensor] = None      # ffm_optim_desc in device memory (fp16 steps / captured steps)
        # optimizer applications ATTEMPTED on the host side.  With the device descriptor (fp16, captured steps) an overflowed
        # step is skipped on the device and optim_desc[9] is the count applied: `steps` is then an upper bound, and
        # ClipEngine.optim_steps() answers the applied count (SGD only uses `steps == 0` as its first-step flag)
        self.steps = 0

    def set_optim_rows(self, rows: int) -> None:
        """Give the state tensor `rows` rows for the optimizer chosen; row 0 (momentum) keeps its values."""
        if rows != self.optim_state.shape[0]:
            new = torch.zeros(rows, self.numel, device=self.flat.device, dtype=torch.float32)
            k = min(rows, self.optim_state.shape[0])
            new[:k].copy_(self.optim_state[:k])
            self.optim_state, self.momentum = new, new[0]

    def view(self, key: str, which: str = "flat") -> Tensor:
        off, shp = self.offsets[key]
        n = 1
        for s in shp:
            n *= s
        return getattr(self, which)[off:off + n].view(shp)

    def load(self, sd: Dict[str, Tensor]) -> None:
        for k in self.keys:
            self.view(k).copy_(sd[k].to(self.flat.device, torch.float32))

    def lora_s_offsets(self) -> Tensor:
        return torch.tensor([self.offsets[k][0] for k in self.keys if k.endswith("lora_S.weight")],
                            dtype=torch.int64, device=self.flat.device)


class SOperands:
    """The singular-value operand S [Geff, r] (and the tensor that receives dS) of every adapter, by prefix
    ('...mlp.c_fc.'), for the adapter types of apply_lora_to_model (trainers/GLP_OT_SVLoRA.py:516-540):

      FairLoRA            lora_S [G, r] itself (a view of the flat buffer), gradient straight into its grad view;
      SVLoRA              lora_S [r] viewed as one group [1, r] (one diagonal shared by all samples, :307-311);
      LoRA                a constant row of ones (:241-242), dS discarded;
      ... + GLOBAL_S      s_b = pi_b S + S_global (:300-304, 418-422, 467-468).  The group mix sums to one, so this is
                          the same kernel call on S_eff[g] = S[g] + S_global, with dS[g] = dS_eff[g] and
                          dS_global = sum_g dS_eff[g]: S_eff is refreshed once per step (`prepare`) and the two gradients
                          are scattered after the reduction (`finish`), three small launches for all adapters together.
    """

    def __init__(self, params: FlatParams, prefixes: List[str], cfg: ModelCfg, device):
        lo = cfg.lora
        self.params, self.r = params, lo.rank
        self.type, self.glob = getattr(lo, "lora_type", "FairLoRA"), bool(getattr(lo, "global_s", False))
        if self.type not in ("FairLoRA", "SVLoRA", "LoRA"):
            raise NotImplementedError(self.type)                   # trainers/GLP_OT_SVLoRA.py:533-534
        if self.type != "FairLoRA" and lo.num_groups != 1:
            raise ValueError(f"lora_type {self.type} has no demographic groups: set num_groups = 1")
        self.G = lo.num_groups
        self.glob = self.glob and self.type != "LoRA"
        self.index = {p: i for i, p in enumerate(prefixes)}
        n, G, r = len(prefixes), self.G, self.r
        f32 = torch.float32
        if self.type == "LoRA":
            self.ones = torch.ones(1, r, device=device, dtype=f32)
            self.scratch = torch.zeros(n, 1, r, device=device, dtype=f32)
        if self.glob:
            base = torch.arange(G * r, device=device)
            self.idx_S = torch.stack([params.offsets[p + "lora_S.weight"][0] + base for p in prefixes])       # [n, G*r]
            self.idx_G = torch.stack([params.offsets[p + "lora_S_global.weight"][0] + base[:r] for p in prefixes])
            self.eff = torch.zeros(n, G, r, device=device, dtype=f32)
            self.deff = torch.zeros(n, G, r, device=device, dtype=f32)
        self.prefixes = prefixes

    def op(self, prefix: str) -> Tensor:
        i = self.index[prefix]
        if self.type == "LoRA":
            return self.ones
        if self.glob:
            return self.eff[i]
        return self.params.view(prefix + "lora_S.weight").view(self.G, self.r)

    def grad(self, prefix: str) -> Tensor:
        i = self.index[prefix]
        if self.type == "LoRA":
            return self.scratch[i]
        if self.glob:
            return self.deff[i]
        return self.params.view(prefix + "lora_S.weight", "grad").view(self.G, self.r)

    def prepare(self) -> None:
        if self.glob:
            flat = self.params.flat
            torch.add(flat[self.idx_S].view(-1, self.G, self.r), flat[self.idx_G].view(-1, 1, self.r), out=self.eff)

    def finish(self) -> None:
        if self.glob:
            g = self.params.grad
            g[self.idx_S.view(-1)] = self.deff.view(-1)
            g[self.idx_G.view(-1)] = self.deff.sum(1).view(-1)


@dataclass(frozen=True)
class Switches:
    """Every Python-side A/B switch of the engines, read from the environment ONCE, when an engine is constructed
    (ClipEngine.sw).  The kernel-side switches are the library's own: the table of csrc/switches.h,
    read once per process as well and readable through ops.switch (ffm_switch)."""
    red_at: Optional[int] = None           # FFM_RED_AT=0|1|2: where a block's LoRA-gradient reductions start (unset: by row count)
    lgrad: bool = True                     # FFM_LGRAD=0: the two large reductions as launches again, not inside dX(c_proj)
    pack_out: bool = True                  # FFM_PACK_OUT=0: patch embedding / final projection weights not in fragment order
    lnb_fold: bool = True                  # FFM_LNB_FOLD=0: both LayerNorm backward passes as kernels of their own
    lnb_fold1: bool = True                 # FFM_LNB_FOLD1=0: ln_1's backward pass as its own kernel
    bn_bwd_fused: bool = True              # FFM_BN_BWD_FUSED=0 (RN50): BatchNorm backward sums from BatchNorm's own pass
    f16_grad_scale: float = 4096.0         # FFM_F16_GRAD_SCALE: initial (and largest) fp16 gradient scale
    f16_growth_interval: float = 2000.0    # FFM_F16_GROWTH_INTERVAL: good steps before the scale doubles again

    @classmethod
    def from_env(cls, env=None) -> "Switches":
        env = os.environ if env is None else env
        on = lambda name: env.get(name, "1") != "0"
        return cls(red_at=int(env["FFM_RED_AT"]) if "FFM_RED_AT" in env else None, lgrad=on("FFM_LGRAD"),
                   pack_out=on("FFM_PACK_OUT"), lnb_fold=on("FFM_LNB_FOLD"), lnb_fold1=on("FFM_LNB_FOLD1"),
                   bn_bwd_fused=on("FFM_BN_BWD_FUSED"), f16_grad_scale=float(env.get("FFM_F16_GRAD_SCALE", "4096")),
                   f16_growth_interval=float(env.get("FFM_F16_GROWTH_INTERVAL", "2000")))


@dataclass(frozen=True)
class Route:
    """Which fused kernels serve a transformer tower at one row count (tower_route).  0: not folded / a kernel of its own."""
    ln1: int = 0          # ln_1 inside the qkv product: partial row sums per row the c_proj forward leaves (its column tiles)
    ln2: int = 0          # ln_2 inside c_fc: partial row sums per row from the out-proj forward
    lgrad: int = 0        # dB(c_fc) and dA(c_proj) inside dX(c_proj) (FFM_EPI_LGRAD): row tiles of their partials
    ln2_bwd: int = 0      # ln_2's backward inside dX(c_proj) / dX(c_fc) (FFM_EPI_LNB_*): column tiles of dX(c_proj)
    ln1_bwd: int = 0      # ln_1's backward inside the attention backward and dX(qkv): partial rows (2 per head)
    red_at: int = 0       # where the side stream starts a block's LoRA-gradient reductions (_stack_backward)


@dataclass(frozen=True)
class Targets:
    """Which linears of a tower's blocks carry an adapter (LoraCfg.targets): what the attention sites add to routing.
    A record of its own - Route keeps its fields for every tower - and the `targets` keyword of tower_route."""
    mlp: bool = True      # mlp.c_fc / mlp.c_proj (the reference's placement)
    attn: bool = False    # attn.in_proj / attn.out_proj

    @classmethod
    def of(cls, lora_cfg) -> "Targets":
        return cls(lora_cfg.on_mlp, lora_cfg.on_attn)


def _can_fold(rank: int, dtype) -> bool:
    """A tower can take a fold at all (it owns the partial-sum buffers rowp / rowp2 / lnb_part): adapters, 16-bit storage."""
    return bool(rank) and _is16(dtype)


def tower_route(width: int, heads: int, tokens: int, causal: bool, rank: int, dtype, packed: bool, rows: int,
                sw: Switches, targets: Targets = Targets()) -> Route:
    """The route of a tower of this geometry at `rows` rows: a pure function of its arguments and of the library's host-side
    queries (which kernel ffm_gemm_nt picks for a shape, and how it tiles it) - no GPU, no engine.  Every fold needs the
    panel kernel with the folding epilogue for EACH product it touches at this row count, the rank inside one MFMA tile
    (0 < rank <= 16: FFM_EPI_RANKOP) and 16-bit storage; tests/test_route_cpu.py pins the regimes of ViT-B/16.
    targets: which linears carry adapters.  An adapted in-projection / out-projection asks for the FairLoRA word of its
    product (the qkv forward: FFM_EPI_BIAS | FFM_EPI_LORA | FFM_EPI_LNIN), a tower without MLP sites for the plain words of
    c_fc / c_proj (no ln_2 fold: the plain GELU product has no folding epilogue), and ln_1's BACKWARD fold stays off for an
    adapted in-projection: ffm_attention_bwd_lnstat forms the row sums from dqkv alone and would miss the adapter's
    terms (us A^T gamma, us A^T beta), so ffm_layernorm_bwd runs."""
    w, r = width, rank
    # red_at by row count - measured (one call, alternating): configs[1] (6304 rows) 4.65-4.71 / 4.66-4.67 / 4.75-4.76 ms per
    # step for 0 / 1 / 2; configs[3] (19 700 rows, rank 16: 52 MB of partials per block, whose sum took the attention
    # backward beside it from 49 to 74 us) 12.45 / 12.42-12.46 / 12.37-12.38
    red_at = 0 if not r else ((2 if rows > 12608 else 0) if sw.red_at is None else sw.red_at)
    if not (_can_fold(r, dtype) and r <= 16):
        return Route(red_at=red_at)
    tiles = lambda n, k, flags, rk=0: ops.gemm_tiles_n(rows, n, k, flags, rk, dtype, True)
    # ln_1: the c_proj forward leaves the row sums, the qkv product normalises in its epilogue
    lora, mlp, att = L.EPI_LORA | L.EPI_RANKOP, targets.mlp, targets.attn
    npj = tiles(w, 4 * w, L.EPI_BIAS | L.EPI_RESIDUAL | L.EPI_ROWSTATS | (lora if mlp else 0), r if mlp else 0)
    nq = tiles(3 * w, w, L.EPI_BIAS | L.EPI_LNIN | (lora if att else 0), r if att else 0)
    ln1 = npj if (npj > 0 and npj <= 8 and nq > 0) else 0
    # ln_2: row sums from the out-proj forward, the FairLoRA c_fc product with the folding epilogue (its rank operand
    # gamma-scaled), and dA(c_fc) from the raw rows (ffm_lora_grad_partial_ln)
    npo = tiles(w, w, L.EPI_BIAS | L.EPI_RESIDUAL | L.EPI_ROWSTATS | (lora if att else 0), r if att else 0)
    nf = tiles(4 * w, w, L.EPI_BIAS | L.EPI_LORA | L.EPI_GELU | L.EPI_RANKOP | L.EPI_LNIN, r) if mlp else 0
    ln2 = npo if (npo > 0 and npo <= 8 and nf > 0 and w % 128 == 0 and r <= 16) else 0
    # FFM_EPI_LGRAD: 0 when the kernel that serves dX(c_proj) has no such epilogue (then the two reduction launches run)
    lgrad = 0
    if sw.lgrad and packed and r % 4 == 0 and mlp:
        lgrad = max(0, ops.gemm_lgrad_rows(rows, 4 * w, w, r, dtype, True))
        if lgrad > ops.lora_grad_splits(rows):                # (the partial buffers are sized for the reduction kernel's splits)
            lgrad = 0
    # ln_2's backward: needs the forward fold (its W gamma / W beta + b / A^T gamma / A^T beta vectors, rows 14 / 15 of the
    # rank operand), the LGRAD epilogue beside which dX(c_proj) leaves the two row sums, and both kernels
    ln2_bwd = 0
    if sw.lnb_fold and ln2 and lgrad > 0 and r <= 14:
        f1 = L.EPI_LORA | L.EPI_LORA_KR | L.EPI_DGELU | L.EPI_RANKOP | L.EPI_LGRAD | L.EPI_LNB_STAT
        n1 = tiles(4 * w, w, f1, r)
        n2 = tiles(w, 4 * w, L.EPI_LORA | L.EPI_LORA_KR | L.EPI_RANKOP | L.EPI_LNB_APPLY, r)
        ln2_bwd = n1 if (0 < n1 <= 8 and n2 > 0) else 0
    # ln_1's backward: row sums per head from ffm_attention_bwd_lnstat, FFM_EPI_LNB_APPLY on the plain panel tile of dX(qkv)
    ln1_bwd = 0
    if sw.lnb_fold and sw.lnb_fold1 and ln1 and not att and 2 * heads <= 24 and ops.attention_bwd_lnstat_ok(tokens, causal, dtype):
        if tiles(w, 3 * w, L.EPI_LNB_APPLY) > 0:
            ln1_bwd = 2 * heads
    return Route(ln1, ln2, lgrad, ln2_bwd, ln1_bwd, red_at)


_PACKED = ("w_in", "w_in_t", "w_out", "w_out_t", "w_fc", "w_fc_t", "w_proj", "w_proj_t", "w_in_ln", "w_fc_ln")


@dataclass
class _Block:
    """Frozen weights of one residual attention block in the compute dtype."""
    w_in: Tensor
    w_in_t: Tensor
    b_in: Tensor
    w_out: Tensor
    w_out_t: Tensor
    b_out: Tensor
    ln1_w: Tensor
    ln1_b: Tensor
    ln2_w: Tensor
    ln2_b: Tensor
    w_fc: Tensor
    w_fc_t: Tensor
    b_fc: Tensor
    w_proj: Tensor
    w_proj_t: Tensor
    b_proj: Tensor
    packed: Optional[Dict[str, Tensor]] = None # bf16 vision blocks: the eight weights in MFMA-fragment order (ops.pack_b)
    # bf16 vision blocks, ln_1 folded into the qkv product (FFM_EPI_LNIN): gamma-scaled in_proj weight, its row sums c
    # and d = W beta + b (frozen: built once at load time)
    w_in_ln: Optional[Tensor] = None
    c_in: Optional[Tensor] = None
    d_in: Optional[Tensor] = None
    # ... and ln_2 folded into the c_fc product
    w_fc_ln: Optional[Tensor] = None
    c_fc: Optional[Tensor] = None
    d_fc: Optional[Tensor] = None

    def pk(self, name: str) -> Optional[Tensor]:
        return self.packed[name] if self.packed else None


_TTS = Tuple[Optional[Tensor], Optional[Tensor]]


@dataclass
class _LayerBufs:
    """What one residual block of `_stack_forward` reads and writes, cut to the rows in use.  Two providers: `_Stack.layer`
    (training: one set per layer, everything the backward needs) and `_InferWorkspace.layer` (evaluation: one set for all
    layers, the optional outputs None).  pre None: the c_fc product stores the activation alone (FFM_EPI_GELU_ONLY)."""
    x: Tensor                                  # block input
    xm: Tensor                                 # after the attention residual
    qkv: Tensor
    o: Tensor
    h: Tensor                                  # ln_1 output (unfolded route)
    h2: Tensor                                 # ln_2 output (unfolded route)
    pre: Optional[Tensor]
    act: Tensor
    x_out: Tensor                              # block output = the next block's input
    lse: Optional[Tensor] = None
    st1: Tuple[Optional[Tensor], Optional[Tensor]] = (None, None)      # ln_1 mean / rstd
    st2: Tuple[Optional[Tensor], Optional[Tensor]] = (None, None)
    rowp: Optional[Tensor] = None              # partial row sums of x (ln_1 folded into qkv), of x_out, of xm (ln_2 into c_fc)
    rowp_out: Optional[Tensor] = None
    rowp2: Optional[Tensor] = None
    # rank vectors (t, ts) of the block's four linears, where they carry a site: outputs of the fused route (optional
    # there), operands of the rank > 16 route
    in_proj: _TTS = (None, None)
    out_proj: _TTS = (None, None)
    c_fc: _TTS = (None, None)
    c_proj: _TTS = (None, None)


class _Stack:
    """A transformer tower (vision with FairLoRA, or text) with its saved activations."""

    def __init__(self, width: int, heads: int, layers: int, tokens: int, max_images: int, causal: bool,
                 rank: int, dtype, device, sw: Switches, x3: bool = False, targets: Targets = Targets()):
        self.width, self.heads, self.layers, self.L = width, heads, layers, tokens
        self.causal, self.rank, self.dtype, self.sw = causal, rank, dtype, sw
        self.targets = targets if rank else Targets(False, False)
        self.routes: Dict[int, Route] = {}                   # rows -> tower_route (route())
        # x3: float32 tower whose products run on the bf16 matrix cores as hi/lo pairs (FFM_F32_X3)
        # a tower with adapters: (c_fc, c_proj) of every block, made once the frozen weights are loaded (_init_vision_late)
        self.sites: List[Tuple[LoraSite, LoraSite]] = []
        # ... and (in_proj, out_proj) of every block, where the attention projections carry adapters (Targets.attn)
        self.asites: List[Tuple[LoraSite, LoraSite]] = []
        # x3 (the text tower, 40 token rows): scratch for the products that are split over K across the grid
        # (ffm_gemm_args.sk_part, csrc/gemm_skinny.hip: N = 512 against K = 1536 / 2048 - c_proj forward, dX(c_fc), dX(qkv));
        # one buffer per tower: its launches are ordered on the tower's stream
        rows_max = max_images * tokens
        self.sk_part = None
        if x3 and rows_max <= 48:
            need = max(ops.gemm_splitk_floats(rows_max, n_, k_, False)
                       for n_, k_ in ((width, 4 * width), (width, 3 * width), (4 * width, width), (3 * width, width), (width, width)))
            if need > 0:
                self.sk_part = torch.empty(need, device=device, dtype=torch.float32)

        def _gemm(*a, **k):
            if self.sk_part is not None:
                k["sk_part"] = self.sk_part
            return ops.gemm_nt(*a, x3=x3, **k)
        self.gemm = _gemm
        self.blocks: List[_Block] = []
        T = max_images * tokens
        self.max_rows = T
        e = lambda *s: torch.zeros(*s, device=device, dtype=dtype)
        f = lambda *s: torch.zeros(*s, device=device, dtype=torch.float32)
        w = width
        self.x = [e(T, w) for _ in range(layers + 1)]        # block inputs; x[layers] = tower output
        self.xm = [e(T, w) for _ in range(layers)]           # after the attention residual
        self.qkv = [e(T, 3 * w) for _ in range(layers)]
        self.o = [e(T, w) for _ in range(layers)]
        self.lse = [f(max_images * heads * tokens) for _ in range(layers)]
        self.st1 = [(f(T), f(T)) for _ in range(layers)]
        self.st2 = [(f(T), f(T)) for _ in range(layers)]
        self.h2 = [e(T, w) for _ in range(layers)]
        self.pre = [e(T, 4 * w) for _ in range(layers)]
        self.act = [e(T, 4 * w) for _ in range(layers)]
        # partial row sums {sum, sum of squares} of every block input, left behind by its producer (FFM_EPI_ROWSTATS /
        # embed_lnpre) for the ln_1 that is folded into the qkv product: up to 8 column tiles
        fold = _can_fold(rank, dtype)
        self.rowp = [f(8 * T * 2) for _ in range(layers + 1)] if fold else None
        self.rowp2 = [f(8 * T * 2) for _ in range(layers)] if fold else None   # ... of xm (ln_2)
        # ln_2's BACKWARD folded into dX(c_proj) / dX(c_fc) (FFM_EPI_LNB_STAT / FFM_EPI_LNB_APPLY): the producer's partial row
        # sums, consumed by the very next launch - one buffer per tower
        # (ln_1's: two partial rows per head from the attention backward kernels, consumed by dX(qkv))
        self.lnb_part = f(max(8, 2 * heads) * T * 2) if fold else None
        # transient buffers
        self.h = e(T, w)
        self.g = e(T, w)          # running gradient w.r.t. the residual stream
        self.g1 = e(T, w)
        self.dh = e(T, w)
        self.do = e(T, w)
        self.dqkv = e(T, 3 * w)
        self.dpre = e(T, 4 * w)
        self.delta = f(max_images * heads * tokens)
        if rank:
            self.u = f(T, rank)       # u = g B^T of the rank > 16 route: one for all sites (dead once its us is formed)
            # The LoRA-gradient reductions trail the dX chain on a side stream, so everything they read is kept per layer:
            # gradient of the block output and dL/d(pre) here, the us vectors and the partial sums in the block's sites.
            if self.targets.mlp:
                self.g_l = [e(T, w) for _ in range(layers)]
                self.dpre_l = [e(T, 4 * w) for _ in range(layers)]
            self.plans = {}                                  # (rows, full backward, block) -> ReducePlan (_reduce_plan)
        if self.targets.attn:
            # attention sites: their reductions read the gradient entering the out-projection (dB of out_proj), dqkv (dB of
            # in_proj) and - where ln_1 is a kernel of its own - its output (dA of in_proj), all three shared or transient in
            # a tower without them: kept per layer here (o, dA of out_proj's operand, already is).  Nothing of this exists
            # with the reference's placement.
            self.g1_l = [e(T, w) for _ in range(layers)]
            self.dqkv_l = [e(T, 3 * w) for _ in range(layers)]
            self.h_l = [e(T, w) for _ in range(layers)]

    def route(self, rows: int) -> Route:
        """Which fused kernels serve this tower at `rows` rows (decided once per row count, after the weights are loaded)."""
        if rows not in self.routes:
            self.routes[rows] = tower_route(self.width, self.heads, self.L, self.causal, self.rank, self.dtype,
                                            self.blocks[0].packed is not None, rows, self.sw, targets=self.targets)
        return self.routes[rows]

    def layer(self, i: int, rows: int) -> _LayerBufs:
        """Block i's share of the stash (everything the backward pass reads), cut to `rows`."""
        fc, proj = self.sites[i] if self.sites else (None, None)
        ain, aout = self.asites[i] if self.asites else (None, None)
        h = self.h_l[i] if self.asites else self.h
        tts = lambda s: (s.t, s.ts) if s else (None, None)
        return _LayerBufs(self.x[i][:rows], self.xm[i][:rows], self.qkv[i][:rows], self.o[i][:rows], h[:rows],
                          self.h2[i][:rows], self.pre[i][:rows], self.act[i][:rows], self.x[i + 1][:rows], self.lse[i],
                          self.st1[i], self.st2[i], self.rowp[i] if self.rowp is not None else None,
                          self.rowp[i + 1] if self.rowp is not None else None,
                          self.rowp2[i] if self.rowp2 is not None else None,
                          in_proj=tts(ain), out_proj=tts(aout), c_fc=tts(fc), c_proj=tts(proj))


class _InferWorkspace:
    """Buffers of the forward-only evaluation pass (FairLoRAEngine.infer) for up to `max_images` ViT images.  Nothing is
    kept for a backward pass, so one set of layer buffers serves every block - the residual stream ping-pongs between two
    buffers - and the size does not depend on the depth of the tower: (2 + 1 + 3 + 1 + 2 + 4) x width 16-bit values per token
    row (x twice, xm, qkv, o, h / h2, the activation) against ~20 x width per row AND LAYER in the training stash.  It shares
    nothing writable with that stash: patch columns, embeddings, features, head and transport buffers are its own too.
    Attribute names follow the engine's, so `_vision_forward` / `_head_forward` take either as their buffer set."""

    def __init__(self, eng: "FairLoRAEngine", max_images: int):
        cfg, v, dtype, dev = eng.cfg, eng.cfg.vision, eng.dtype, eng.device
        self.max_images = max_images
        T, w, P, r = max_images * v.tokens, v.width, v.grid * v.grid, cfg.lora.rank
        f32 = torch.float32
        e = lambda *s: torch.zeros(*s, device=dev, dtype=dtype)
        f = lambda *s: torch.zeros(*s, device=dev, dtype=f32)
        self.xs = (e(T, w), e(T, w))
        self.xm, self.qkv, self.o, self.h, self.h2, self.act = e(T, w), e(T, 3 * w), e(T, w), e(T, w), e(T, w), e(T, 4 * w)
        fold = _can_fold(r, dtype)                        # the partial row sums of the LayerNorm folds
        self.rowps = (f(8 * T * 2), f(8 * T * 2)) if fold else None
        self.rowp2 = f(8 * T * 2) if fold else None
        # rank > 16: the down projections are launches of their own and t / ts their operands (one pair: c_fc's is dead
        # when c_proj's is formed)
        self.t, self.ts = (f(T, r), f(T, r)) if (r and not eng.fused_rank) else (None, None)
        self.cols = e(max_images * P, 3 * v.patch * v.patch)
        self.patch_out = e(max_images * P, w)
        self.hpost = e(T, w)
        self.post_stats = (None, None)
        self.feat = e(T, v.out_dim)
        self.fbar = f(max_images, v.out_dim)
        self.rnorm = f(T)
        self.logits_img = f(max_images, cfg.n_cls)
        self.attr_i32 = torch.zeros(max_images, device=dev, dtype=torch.int32)
        if eng.is3d:
            H = v.image_size
            self.conv_out = f(max_images, 3, H, H)
            self.mm_part = f(max_images * ops.slice_blocks(H, H) * 2)
            self.mnmx = f(max_images, 2)
            self.mm_cnt = torch.zeros(max_images, 2, device=dev, dtype=torch.int32)
        if eng.ot:
            n = max_images * cfg.n_cls * (v.tokens - 1) * cfg.n_prompts
            self.ot_sim, self.ot_T = f(n), f(n)
            self.ot_errs = f(cfg.ot_max_iter * max_images * cfg.n_cls)
            self.ot_istop = torch.zeros(1, device=dev, dtype=torch.int32)
            self.ot_tsum = f(max_images * cfg.n_cls)

    def layer(self, i: int, rows: int) -> _LayerBufs:
        a, b = self.xs[i & 1], self.xs[(i + 1) & 1]
        rp, tts = self.rowps, (self.t, self.ts)
        return _LayerBufs(a[:rows], self.xm[:rows], self.qkv[:rows], self.o[:rows], self.h[:rows], self.h2[:rows], None,
                          self.act[:rows], b[:rows], rowp=rp[i & 1] if rp else None, rowp_out=rp[(i + 1) & 1] if rp else None,
                          rowp2=self.rowp2, in_proj=tts, out_proj=tts, c_fc=tts, c_proj=tts)

    def nbytes(self) -> int:
        """Bytes of device memory the workspace holds."""
        seen, n = set(), 0
        for val in vars(self).values():
            for t in (val if isinstance(val, tuple) else (val,)):
                if isinstance(t, Tensor) and t.data_ptr() not in seen:
                    seen.add(t.data_ptr())
                    n += t.numel() * t.element_size()
        return n


def _site_fwd(site: Optional[LoraSite], gemm, x, W, out, attr, rps, tts=None, ln=False, **k) -> None:
    """A linear of a block that may carry no site: the plain product, or the site's (LoraSite.fwd)."""
    if site is None:
        gemm(x, W, out, **k)
    else:
        site.fwd(x, W, out, attr, rps, gemm=gemm, tts=tts, ln=ln, **k)


def _site_bwd(site: Optional[LoraSite], gemm, g, Wt, dx, attr, rps, lgrad=None, down=True, **k) -> None:
    """... and its dX product (LoraSite.bwd)."""
    if site is None:
        gemm(g, Wt, dx, **k)
    else:
        site.bwd(g, Wt, dx, attr, rps, gemm=gemm, lgrad=lgrad, down=down, **k)


class ClipEngine:
    """HIP execution engine for CustomCLIP(+FairLoRA) training and inference: everything that does not depend on which
    image tower is attached - the flat parameter buffer, the text tower, the logits and transport heads, the loss, the fp16
    scale state, streams and events, launch recording and replay, the optimizers and the captured step.  An image tower is
    a subclass (FairLoRAEngine: ViT, RN50Engine in engine_rn.py) that supplies the hooks below; the base allocates from
    cfg.vision only `tokens` and `out_dim` (feat, dfeat, rnorm, the head and transport buffers), which every vision
    config carries.

    The tower contract (TOWER_HOOKS).  A hook without a default raises NotImplementedError here:

      hook                                          called from                                        default
      _init_vision(max_images)                      __init__, before load_frozen: the tower's          none
                                                    buffers, its streams and events (ev_layer)
      _load_vision_frozen(sd, put)                  load_frozen                                        none
      _init_vision_late()                           __init__, after load_frozen; must leave            none
                                                    self.sops and self.pack_plan
      _load_inputs(image, attr, label) -> (b, S)    forward, forward_backward (not replayed)           none
      _vision_forward(b, S, has_attr, wait=None)    forward, _step_body; ends in _head_forward         none
      _vision_backward(b, S, has_attr)              _step_body; dfeat -> params.grad                   none
      _after_plan(b, S)                             forward_backward, between the plan (recorded,      no-op
                                                    replayed or eager) and unscale_check
      inference() / infer(image, attr)              trainer, evaluator                                 nullcontext(self) /
                                                                                                       forward(image, attr),
                                                                                                       infer_ws None

    A tower that extends the step itself overrides `_step_body` / `forward_backward` and calls super()."""

    # (name, has a default here) of every hook of the contract above, in the table's order
    TOWER_HOOKS = (("_init_vision", False), ("_load_vision_frozen", False), ("_init_vision_late", False),
                   ("_load_inputs", False), ("_vision_forward", False), ("_vision_backward", False), ("_after_plan", True),
                   ("inference", True), ("infer", True))
    infer_ws = None                                   # a forward-only workspace, where the tower has one

    @property
    def grad_scale(self) -> float:
        """fp16 mode: the factor on dloss/dlogits in front of the backward pass, taken out of the fp32 gradients behind it.
        It lives in DEVICE memory (``scale_state``, ffm_loss_scale in include/ffm_hip.h) and moves by itself: an overflowed
        backward pass skips its SGD step and halves it.  Reading it synchronises; 1.0 in the other storage types."""
        return float(self.scale_state[0]) if self.scale_state is not None else 1.0

    @grad_scale.setter
    def grad_scale(self, value: float) -> None:
        value = float(value)
        if not (value > 0.0) or value != value or value == float("inf"):
            raise ValueError(f"grad_scale must be a positive finite number, got {value!r}")
        if self.scale_state is None:
            if value != 1.0:
                raise ValueError("grad_scale exists in the IEEE-half mode only")
            return
        # recorded plans read the scale through the state's address: nothing to re-record
        self.scale_state[:2].copy_(torch.tensor([value, 1.0 / value]))
        self.scale_state[5:6].fill_(max(value, float(self.scale_state[5])))

    def overflow_steps(self) -> int:
        """fp16 mode: training steps skipped so far because their scaled gradients left half's range (host sync)."""
        return int(self.scale_state[4]) if self.scale_state is not None else 0

    def __init__(self, cfg: ModelCfg, state_dict: Dict[str, Tensor], dtype=torch.bfloat16, max_images: int = 32,
                 device: str = "cuda:0", max_infer_images: Optional[int] = None):
        """max_images sizes the training stash (forward / forward_backward), max_infer_images (default: max_images) the
        workspace of the forward-only pass (infer) of a tower that has one."""
        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} needs an MI355X GPU; there is no CPU path")
        from . import _lib
        _lib.load()                                   # fail loudly if the HIP library is missing
        if cfg.vision.head_dim != 64 or cfg.text.width // cfg.text.heads != 64:
            raise ValueError("attention kernels are built for head_dim 64 (all CLIP towers)")
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.max_images = max_images
        v, t = cfg.vision, cfg.text
        # what the tower hooks below and the step read: set before any of them runs
        self.sw = Switches.from_env()
        # FairLoRA down projections ride inside the GEMMs (FFM_EPI_RANKOP) when the rank fits one MFMA tile
        self.fused_rank = 0 < cfg.lora.rank <= 16
        self.pack_plan = None                         # rank operands of the fused products (_init_vision_late)
        self._pack_event = None
        self.pk_out: Dict[str, Tensor] = {}           # frozen weights outside the blocks in MFMA-fragment order
        self.use_replay = True                        # replay recorded launch plans (host-side "graph")
        self.params = FlatParams(cfg, self.device)
        self.params.load(state_dict)
        self.n_text = cfg.n_prompts * cfg.n_cls
        # Text tower: the mask is causal and only the EOT row of each prompt is read (clip/model.py:562-568,
        # trainers/GLP_OT_SVLoRA.py:62-64), so tokens after the last EOT position influence neither the features nor
        # the ctx gradient.  The tower runs on the first max(eot)+1 tokens of the 77 (10 for the four FairFedMed
        # prompts): bit-identical rows, 7.7x fewer of them, and far less interference with the vision chain.
        self.txt_len = min(t.context_length, max(cfg.eot) + 1)
        assert self.txt_len >= 1 + cfg.n_ctx
        # the text-tail kernels index x[eot_row[p]] without a range check (csrc/text.hip): an EOT position outside the
        # rows the tower keeps would read another prompt's row
        if not all(0 <= int(e) < self.txt_len for e in cfg.eot):
            raise ValueError(f"EOT positions {list(cfg.eot)} must lie inside the {self.txt_len} text rows that are kept "
                             f"(context_length {t.context_length})")
        # ... and ALWAYS in float32, also in the bf16 throughput mode: the two classes' prompts differ in a few tokens, so
        # the logit difference l1 - l0 = e^ls <f, t1 - t0> rides on the small difference of two nearly equal text features,
        # and 2^-9 roundings of the text activations AND of the text weights land on it many times amplified.  Measured on
        # the tiny model (tools/auc_diag.py, AUC after equal rounds against the reference): text tower in bf16 0.0026 off,
        # f32 activations on bf16 weights 0.0020, all f32 0.0005.  Beside a bf16 vision tower the 40-row products run on
        # the bf16 matrix cores as hi/lo pairs (FFM_F32_X3, csrc/gemm_skinny.hip) instead of the 16x slower f32 MFMA.
        self.txt = _Stack(t.width, t.heads, t.layers, self.txt_len, self.n_text, True, 0, torch.float32, self.device,
                          self.sw, x3=(_is16(dtype)))
        dev, f32 = self.device, torch.float32
        self._init_vision(max_images)                 # the tower's buffers (the contract in the class docstring)
        self.load_frozen(state_dict)
        self._init_vision_late()
        self.feat = torch.zeros(max_images * v.tokens, v.out_dim, device=dev, dtype=dtype)
        self.dfeat = torch.zeros_like(self.feat)
        self.fbar = torch.zeros(max_images, v.out_dim, device=dev, dtype=f32)
        self.rnorm = torch.zeros(max_images * v.tokens, device=dev, dtype=f32)
        self.logits_img = torch.zeros(max_images, cfg.n_cls, device=dev, dtype=f32)
        self.dlogits_img = torch.zeros_like(self.logits_img)
        self.logits = torch.zeros(max_images, cfg.n_cls, device=dev, dtype=f32)
        self.prob = torch.zeros_like(self.logits)
        self.loss = torch.zeros(1, device=dev, dtype=f32)
        self.finite = torch.ones(1, device=dev, dtype=torch.int32)
        # IEEE-half storage: dloss/dlogits is scaled by 2^k before the backward pass (every backward kernel is linear in
        # the incoming gradient) and the factor comes out of the fp32 gradient buffer in front of the SGD step.  Unscaled,
        # the 16-bit activation gradients of ViT-B/16 sit in half's subnormals (2.8 % error on the lora_S gradient norms
        # at batch 8; 0.3 % scaled: tests/test_engine_gpu.py).  Round 6: the scale is DYNAMIC and device-resident
        # (ops.loss_scale / unscale_check / sgd_momentum_gated): a backward pass whose scaled gradients overflow skips its
        # SGD step and halves the scale - no host sync, recorded plans stay valid - instead of raising; after
        # FFM_F16_GROWTH_INTERVAL (2000) good steps it doubles again, up to the initial value FFM_F16_GRAD_SCALE (4096).
        self.scale_state = None
        if dtype == torch.float16:
            s0 = self.sw.f16_grad_scale
            self.scale_state = torch.tensor([s0, 1.0 / s0, 1.0, 0.0, 0.0, s0, self.sw.f16_growth_interval, 1.0],
                                            device=dev, dtype=f32)
        self.dtbar = torch.zeros(cfg.n_cls, v.out_dim, device=dev, dtype=f32)
        self.attr_i32 = torch.zeros(max_images, device=dev, dtype=torch.int32)
        self.label_buf = torch.zeros(max_images, device=dev, dtype=torch.int64)
        self._counts_buf = None                       # enable_step_counts()
        # set_fairness(): lambda and with_grad of the loss's group-confidence-gap term; {cls, F} and {m_g, n_g} per group
        self._fair_lam, self._fair_grad, self._fair_step = 0.0, False, False
        self._drift = None                            # set_drift(): a drift.DriftCorrector applied behind every backward pass
        self.loss_terms = torch.zeros(2, device=dev, dtype=f32)
        self.group_conf = torch.zeros(ops.MAX_GROUPS, 2, device=dev, dtype=f32)
        self.tbar_buf = torch.zeros(cfg.n_cls, v.out_dim, device=dev, dtype=f32)
        self.ot = cfg.ot if cfg.ot != "None" else None
        if self.ot:
            # Sinkhorn / COT logits heads (trainers/GLP_OT_SVLoRA.py:615-675, 713-757; csrc/head_ot.hip)
            if self.ot not in ops.OT_MODES:
                raise NotImplementedError(cfg.ot)
            P, M, N = max_images * cfg.n_cls, v.tokens - 1, cfg.n_prompts
            self.dtn = torch.zeros(N * cfg.n_cls, v.out_dim, device=dev, dtype=f32)
            self.ot_sim = torch.zeros(P * M * N, device=dev, dtype=f32)
            self.ot_T = torch.zeros_like(self.ot_sim)
            self.ot_errs = torch.zeros(cfg.ot_max_iter * P, device=dev, dtype=f32)
            self.ot_istop = torch.zeros(1, device=dev, dtype=torch.int32)
            self.ot_tsum = torch.zeros(P, device=dev, dtype=f32)
            self.ot_dtn_part = torch.zeros(max_images * N * cfg.n_cls * v.out_dim, device=dev, dtype=f32)
        self.step_plans: Dict[tuple, list] = {}
        # the two ends of the text tower (csrc/text.hip): absolute EOT row of every prompt, the un-normalised / normalised
        # text features, 1 / norm and ln_final's statistics kept for the way back, the projection's input gradient
        self.eot_rows = torch.tensor([i * self.txt_len + cfg.eot[i % cfg.n_cls] for i in range(self.n_text)],
                                     device=dev, dtype=torch.int32)
        self.tf_buf = torch.zeros(self.n_text, v.out_dim, device=dev, dtype=f32)
        self.tn_all = torch.zeros(self.n_text, v.out_dim, device=dev, dtype=f32)
        self.t_rnorm = torch.zeros(self.n_text, device=dev, dtype=f32)
        self.t_stats = torch.zeros(self.n_text, 2, device=dev, dtype=f32)
        self.t_dy = torch.zeros(self.n_text, t.width, device=dev, dtype=f32)
        if self.ot:
            self.tn_buf = self.tn_all                     # the transport heads read every prompt's normalised feature
        # The text tower (308 token rows) is latency-bound and independent of the vision tower until the
        # logits head, so it runs on its own HIP stream beside it (forward and backward).
        self.side = self._side0 = torch.cuda.Stream(device=self.device)
        self.grad_stream = self._grad0 = torch.cuda.Stream(device=self.device)
        self.ev_grads = torch.cuda.Event()
        self.ev_tail = torch.cuda.Event()
        self.ev_tail0 = torch.cuda.Event()
        self.ev_text_fwd = torch.cuda.Event()
        self.ev_head_bwd = torch.cuda.Event()
        self.ev_text_bwd = torch.cuda.Event()
        self.ev_start = torch.cuda.Event()
        self.ev_pack = torch.cuda.Event()
        self.max_infer_images = max_images if max_infer_images is None else int(max_infer_images)

    # -------------------------------------------------------- tower contract --
    def _init_vision(self, max_images: int) -> None:
        raise NotImplementedError

    def _load_vision_frozen(self, sd: Dict[str, Tensor], put) -> None:
        raise NotImplementedError

    def _init_vision_late(self) -> None:
        raise NotImplementedError

    def _load_inputs(self, image: Tensor, attr: Optional[Tensor], label: Optional[Tensor]) -> Tuple[int, int]:
        raise NotImplementedError

    def _vision_forward(self, b: int, S: int, has_attr: bool, wait=None) -> None:
        raise NotImplementedError

    def _vision_backward(self, b: int, S: int, has_attr: bool) -> None:
        raise NotImplementedError

    def _after_plan(self, b: int, S: int) -> None:
        """What a step launches outside its plan, behind it: it may read the caller's tensors (no static address) and writes
        params.grad in front of unscale_check."""

    def inference(self):
        """``with eng.inference():`` - an evaluation session.  Without a forward-only pass a session changes nothing, so
        that a trainer treats every tower alike."""
        return contextlib.nullcontext(self)

    def infer(self, image: Tensor, attr: Optional[Tensor] = None) -> Tensor:
        """forward()'s logits [B, n_cls]; a tower with a forward-only pass overrides it."""
        return self.forward(image, attr)

    # ------------------------------------------------------------ weights --
    def _w(self, x: Tensor, dtype=None) -> Tensor:
        return ops.cast_from_f32(x.to(self.device, torch.float32).contiguous(), dtype or self.dtype)

    def _wt(self, x: Tensor, dtype=None) -> Tensor:
        return ops.transpose_cast(x.to(self.device, torch.float32).contiguous(), dtype or self.dtype)

    def _f(self, x: Tensor) -> Tensor:
        return x.to(self.device, torch.float32).contiguous().clone()

    def _load_stack(self, stack: _Stack, sd, prefix: str, lora: bool) -> None:
        old = stack.blocks if stack.blocks else None
        W = lambda x: self._w(x, stack.dtype)
        WT = lambda x: self._wt(x, stack.dtype)
        stack.blocks = []
        for i in range(stack.layers):
            p = f"{prefix}transformer.resblocks.{i}."
            fc = "mlp.c_fc.original_linear." if lora else "mlp.c_fc."
            pj = "mlp.c_proj.original_linear." if lora else "mlp.c_proj."
            blk = _Block(
                w_in=W(sd[p + "attn.in_proj_weight"]), w_in_t=WT(sd[p + "attn.in_proj_weight"]),
                b_in=self._f(sd[p + "attn.in_proj_bias"]),
                w_out=W(sd[p + "attn.out_proj.weight"]), w_out_t=WT(sd[p + "attn.out_proj.weight"]),
                b_out=self._f(sd[p + "attn.out_proj.bias"]),
                ln1_w=self._f(sd[p + "ln_1.weight"]), ln1_b=self._f(sd[p + "ln_1.bias"]),
                ln2_w=self._f(sd[p + "ln_2.weight"]), ln2_b=self._f(sd[p + "ln_2.bias"]),
                w_fc=W(sd[p + fc + "weight"]), w_fc_t=WT(sd[p + fc + "weight"]),
                b_fc=self._f(sd[p + fc + "bias"]),
                w_proj=W(sd[p + pj + "weight"]), w_proj_t=WT(sd[p + pj + "weight"]),
                b_proj=self._f(sd[p + pj + "bias"]),
            )
            if lora and _is16(stack.dtype):
                w32 = sd[p + "attn.in_proj_weight"].to(self.device, torch.float32)
                g1, b1 = blk.ln1_w, blk.ln1_b
                blk.w_in_ln = W(w32 * g1[None, :])
                blk.c_in = blk.w_in_ln.float().sum(1).contiguous()        # row sums of the weight AS ROUNDED
                blk.d_in = (w32 @ b1 + blk.b_in).contiguous()
                wf32 = sd[p + fc + "weight"].to(self.device, torch.float32)
                blk.w_fc_ln = W(wf32 * blk.ln2_w[None, :])
                blk.c_fc = blk.w_fc_ln.float().sum(1).contiguous()
                blk.d_fc = (wf32 @ blk.ln2_b + blk.b_fc).contiguous()
            if old is not None:
                # keep the device addresses stable (recorded launch plans hold raw pointers): refresh in place
                for name, val in vars(blk).items():
                    if isinstance(val, torch.Tensor):
                        getattr(old[i], name).copy_(val)
                blk = old[i]
            if lora and _is16(stack.dtype):
                # frozen weights in MFMA-fragment order for the panel GEMM (csrc/gemm_panel_impl.h)
                if blk.packed is None:
                    blk.packed = {}
                for name in _PACKED:
                    blk.packed[name] = ops.pack_b(getattr(blk, name), blk.packed.get(name))
            stack.blocks.append(blk)

    def load_frozen(self, sd: Dict[str, Tensor]) -> None:
        """(Re)build the compute-dtype copies of every frozen tensor."""
        te = "text_encoder."
        self._load_stack(self.txt, sd, te, False)
        def put(name, val):                                       # stable addresses across reloads
            cur = getattr(self, name, None)
            if cur is None:
                setattr(self, name, val)
            elif isinstance(val, tuple):
                for c, n in zip(cur, val):
                    c.copy_(n)
            else:
                cur.copy_(val)

        self._load_vision_frozen(sd, put)
        put("logit_scale", self._f(sd["logit_scale"].reshape(1)))
        # text side constants stay fp32 (tiny): prompt pieces, ln_final, projection
        put("tok_prefix", self._f(sd["prompt_learner.token_prefix"]))
        put("tok_suffix", self._f(sd["prompt_learner.token_suffix"]))
        put("txt_pos", self._f(sd[te + "positional_embedding"]))
        put("lnfinal", (self._f(sd[te + "ln_final.weight"]), self._f(sd[te + "ln_final.bias"])))
        put("text_proj", self._f(sd[te + "text_projection"]))

    # -------------------------------------------------------------- tower --
    def _stack_forward(self, st: _Stack, rows: int, images: int, attr: Optional[Tensor], rows_per_sample: int,
                       bufs=None) -> Tensor:
        """The tower input is in layer 0's `x`; returns the tower output view.  bufs: the provider of every block's
        `_LayerBufs` - the tower's own stash (default: training and forward()) or an `_InferWorkspace`, whose sets have no
        pre-activation, no rank vectors and no statistics: the same launches in the same order, fewer stores."""
        gemm = st.gemm
        bufs = st if bufs is None else bufs
        out = lb = sfc = None
        rt = st.route(rows)
        fold, fold2 = rt.ln1, rt.ln2

        def lin(site, a, w, y, tts, **k):
            _site_fwd(site, gemm, a, w, y, attr, rows_per_sample, tts=tts, **k)

        def fc(a, w, **k):
            # c_fc + QuickGELU of the current block: pre-activation and activation (the backward reads both), or the
            # activation alone
            if lb.pre is None:
                lin(sfc, a, w, lb.act, lb.c_fc, gelu_only=True, **k)
            else:
                lin(sfc, a, w, lb.pre, lb.c_fc, gelu_out=lb.act, **k)
        for i, blk in enumerate(st.blocks):
            lb = bufs.layer(i, rows)
            x, xm, qkv, o, h, h2, act = lb.x, lb.xm, lb.qkv, lb.o, lb.h, lb.h2, lb.act
            # the block's four linears, each with its site or None (attention sites alone: plain c_fc / c_proj)
            ain, aout = st.asites[i] if st.asites else (None, None)
            sfc, sproj = st.sites[i] if st.sites else (None, None)
            if fold:
                # ln_1 rides inside the qkv product: raw rows x gamma-scaled weight, normalised in the epilogue with the
                # row sums the producer of x left behind (block 0: embed_lnpre, else the previous block's c_proj)
                ln = ops.LnIn(lb.rowp, 1 if i == 0 else fold, blk.c_in, lb.st1[0], lb.st1[1], rk=ain and ain.lnrk)
                lin(ain, x, blk.w_in_ln, qkv, lb.in_proj, ln=True, bias=blk.d_in, b_packed=blk.pk("w_in_ln"), ln_in=ln)
            else:
                ops.layernorm_fwd(x, h, blk.ln1_w, blk.ln1_b, lb.st1[0], lb.st1[1])
                lin(ain, h, blk.w_in, qkv, lb.in_proj, bias=blk.b_in, b_packed=blk.pk("w_in"))
            # (an adapted in-projection is the packed one, before q is scaled: the attention kernels scale)
            ops.attention_fwd(qkv, o, lb.lse, images, st.L, st.heads, st.causal)
            # the out-projection: a c_proj-type product with the residual (and, ln_2 folded, its row sums)
            lin(aout, o, blk.w_out, xm, lb.out_proj, bias=blk.b_out, res=x, b_packed=blk.pk("w_out"),
                rowstats=lb.rowp2 if fold2 else None)
            if fold2:
                # ln_2 rides inside the c_fc product (h2 is never written; dA(c_fc) takes the raw rows, _stack_backward)
                ln = ops.LnIn(lb.rowp2, fold2, blk.c_fc, lb.st2[0], lb.st2[1], rk=sfc.lnrk)
                fc(xm, blk.w_fc_ln, ln=True, bias=blk.d_fc, b_packed=blk.pk("w_fc_ln"), ln_in=ln)
            else:
                ops.layernorm_fwd(xm, h2, blk.ln2_w, blk.ln2_b, lb.st2[0], lb.st2[1])
                fc(h2, blk.w_fc, bias=blk.b_fc, b_packed=blk.pk("w_fc"))
            lin(sproj, act, blk.w_proj, lb.x_out, lb.c_proj, bias=blk.b_proj, res=xm, b_packed=blk.pk("w_proj"),
                rowstats=lb.rowp_out if (fold and i + 1 < st.layers) else None)
            out = lb.x_out
        return out

    def _stack_backward(self, st: _Stack, rows: int, images: int, attr: Optional[Tensor], rows_per_sample: int,
                        need_input_grad: bool, grad_in_last: bool = False) -> Tensor:
        """st.g[:rows] holds dL/d(tower output) (a FairLoRA tower with grad_in_last: st.g_l[layers - 1] does - the buffer the
        last block's reductions read - and no copy is made); on return st.g holds dL/d(tower input) (if need_input_grad).
        LoRA gradients are written into params.grad."""
        r = st.rank if st.sites else 0                # (attention sites alone: the MLP's backward is the plain one)
        att = bool(st.asites)
        gemm = st.gemm
        g, do, dh = st.g[:rows], st.do[:rows], st.dh[:rows]
        main = torch.cuda.current_stream(self.device)
        rt = st.route(rows)

        def dX(site, gy, wt, dx, **k):
            _site_bwd(site, gemm, gy, wt, dx, attr, rows_per_sample, **k)
        for i in range(st.layers - 1, -1, -1):
            blk = st.blocks[i]
            x, xm, qkv, o = st.x[i][:rows], st.xm[i][:rows], st.qkv[i][:rows], st.o[i][:rows]
            pre, act, h2 = st.pre[i][:rows], st.act[i][:rows], st.h2[i][:rows]
            # the dX chain ends inside block 0: behind dX(c_proj) - or, with attention sites, behind the attention backward
            # (last_att: block 0 runs its MLP part as every other block does and stops at dqkv)
            last_att = att and (i == 0) and not need_input_grad
            last = (i == 0) and not need_input_grad and not att
            # attention sites: their reductions read dL/d x_mid (dB of out_proj), dqkv (dB of in_proj) and ln_1's output
            # (dA of in_proj) on the side stream - kept per layer, shared by all blocks in a tower without them
            ain, aout = st.asites[i] if att else (None, None)
            g1, dqkv, h = ((st.g1_l[i], st.dqkv_l[i], st.h_l[i]) if att else (st.g1, st.dqkv, st.h))
            g1, dqkv, h = g1[:rows], dqkv[:rows], h[:rows]
            if r:
                # gradient w.r.t. this block's output lives in its own buffer (read later by the side stream)
                gi, dpre = st.g_l[i][:rows], st.dpre_l[i][:rows]
                if i == st.layers - 1 and not grad_in_last:
                    self._glue(lambda gi=gi, g=g: gi.copy_(g))
                sfc, sproj = st.sites[i]
                # ---- critical path: u = g B^T and dX (+ LoRA dx term), dS partials
                if last:
                    # the step's tail: dB(c_proj) needs only gi and the forward's ts2 - it starts beside this block's dX
                    # product instead of behind it
                    self._ev_record(self.ev_tail0, main)
                    self._ev_wait(self.grad_stream, self.ev_tail0)
                    with self._on(self.grad_stream):
                        sproj.grad_B(gi)
                # FFM_EPI_LGRAD: dB(c_fc) = dpre^T ts1 and dA(c_proj) = act^T us2 leave with the dX product of c_proj, which
                # holds dpre and (through pre) act in registers - per row tile, into the buffers the two reduction launches
                # they replace would have filled (77 MB per block that the side stream no longer reads beside the chain)
                lg = rt.lgrad
                # ln_2's backward rides in this block's two dX products (not block 0 of a tower that stops there)
                lnb = 0 if last else rt.ln2_bwd
                dX(sproj, gi, blk.w_proj_t, dpre, lgrad=(sfc.ts[:rows], sfc.pB, sproj.pA) if lg else None, dgelu_aux=pre,
                   b_packed=blk.pk("w_proj_t"), lnb_stat=ops.LnBwdStat(st.lnb_part) if lnb else None)

                def dx_fc(down=True):
                    # dX(c_fc); lnb: it stores dL/d x_mid = LayerNorm backward(g_h) + gi directly - no ffm_layernorm_bwd launch
                    la = ops.LnBwdApply(st.lnb_part, lnb, xm, blk.ln2_w, st.st2[i][0], st.st2[i][1], sfc.lnrk, gi) if lnb else None
                    dX(sfc, dpre, blk.w_fc_t, g1 if lnb else dh, down=down, b_packed=blk.pk("w_fc_t"), lnb_apply=la)
                # c_fc's down projection u1 = dpre B_fc^T rides inside its dX product, or stands alone in front of it: where
                # the chain ends with it, and at rank > 16, where the reductions may start behind it, beside the product
                alone = last or not self.fused_rank
                if not alone:
                    dx_fc()
                else:
                    if last:
                        # the dX chain ends with this down projection: the three reductions that do not need its result
                        # start beside it instead of behind it (the step's tail: 32 + 57 us in a row otherwise)
                        self._ev_record(self.ev_tail, main)
                        self._ev_wait(self.grad_stream, self.ev_tail)
                        with self._on(self.grad_stream):
                            if not lg:
                                sproj.grad_A(act)
                                sfc.grad_B(dpre)
                    sfc.down_bwd(dpre, attr, rows_per_sample)
                # ---- off the critical path: the four rank-r gradient reductions of this block
                def reductions(i=i, sfc=sfc, sproj=sproj, gi=gi, act=act, dpre=dpre, xm=xm, h2=h2, last=last, lg=lg):
                    # (the step's tail - block 0's last reduction and the sum of its partials - on the chain's own stream
                    # instead of behind two cross-stream events: measured, 4.699 -> 4.692 ms per step, nothing; not kept)
                    self._ev_record(self.ev_layer[i], main)
                    self._ev_wait(self.grad_stream, self.ev_layer[i])
                    with self._on(self.grad_stream):
                        if not last:
                            sproj.grad_B(gi)
                            if not lg:
                                sproj.grad_A(act)
                                sfc.grad_B(dpre)
                        if rt.ln2:
                            sfc.grad_A(xm, ln_stats=st.st2[i])
                        else:
                            sfc.grad_A(h2)
                        # this block's six gradient tensors are complete: sum their partials now, behind the four reductions
                        # on the same side stream (one launch per block; only block 0's is left when the dX chain ends -
                        # ONE launch for all 72 tensors at the end sat in the step's tail for ~50 us)
                        self._reduce_plan(st, rows, need_input_grad or att, i).run()
                # red_at: where the side stream may start them (everything they read is kept per layer).  0: behind this
                # block's dX(c_fc) - beside its LayerNorm / out-proj / attention backward; 1: behind its attention backward;
                # 2: behind the whole block - beside the NEXT block's two FairLoRA products, whose main loops live on
                # LDS / L2 operands (the last block's have nothing behind them and always start at once)
                red_at = 0 if last or i == 0 else rt.red_at
                if red_at == 0:
                    reductions()
                if last:
                    break
                if alone:
                    dx_fc(down=False)
                gout = st.g_l[i - 1][:rows] if i > 0 else g
            else:
                # (no MLP sites: the two plain products, from the weights as loaded)
                gi, dpre, gout = g, st.dpre[:rows], g
                lnb = red_at = 0
                gemm(gi, blk.w_proj_t, dpre, dgelu_aux=pre)
                gemm(dpre, blk.w_fc_t, dh)
            if not lnb:
                ops.layernorm_bwd(dh, xm, blk.ln2_w, st.st2[i][0], st.st2[i][1], gi, g1)
            # ---- the attention half
            dX(aout, g1, blk.w_out_t, do, b_packed=blk.pk("w_out_t"))
            # ln_1's backward: its two row sums leave with the attention backward (two partial rows per head), and the dX
            # product of the in-projection stores dL/d x = LayerNorm backward(g_h) + g1 directly (never with an adapted
            # in-projection: tower_route keeps the fold off there, and ffm_layernorm_bwd runs)
            lnb1 = rt.ln1_bwd
            ops.attention_bwd(qkv, o, do, st.lse[i], st.delta, dqkv, images, st.L, st.heads, st.causal,
                              ln_stat=(blk.c_in, blk.d_in, st.lnb_part) if lnb1 else None)
            if red_at == 1:
                reductions()
            if last_att:
                # the chain ends at dqkv: the in-projection takes the stand-alone down projection for us and the dS partials,
                # as block 0's c_fc does in a tower without attention sites
                ain.down_bwd(dqkv, attr, rows_per_sample)
            else:
                la = ops.LnBwdApply(st.lnb_part, lnb1, x, blk.ln1_w, st.st1[i][0], st.st1[i][1], None, g1) if lnb1 else None
                dX(ain, dqkv, blk.w_in_t, gout if lnb1 else dh, b_packed=blk.pk("w_in_t"), lnb_apply=la)
                if not lnb1:
                    ops.layernorm_bwd(dh, x, blk.ln1_w, st.st1[i][0], st.st1[i][1], g1, gout)
            if red_at == 2:
                reductions()
            if att:
                # the attention sites' four reductions: everything they read is the block's own (g1_l, dqkv_l, o, h_l or the
                # raw rows x; us and the partials in the sites), so they trail the chain on the side stream behind one event
                self._ev_record(self.ev_attn[i], main)
                self._ev_wait(self.grad_stream, self.ev_attn[i])
                with self._on(self.grad_stream):
                    aout.grad_B(g1)
                    aout.grad_A(o)
                    ain.grad_B(dqkv)
                    if rt.ln1:
                        ain.grad_A(x, ln_stats=st.st1[i])     # ln_1 was folded into the qkv product: dA from the raw rows
                    else:
                        ain.grad_A(h)
                    self._reduce_plan(st, rows, not last_att, i, attn=True).run()
            if last_att:
                break
        if r or att:
            if self.sops.glob:
                self._glue(self.sops.finish, self.grad_stream)     # dS_eff -> dS, dS_global
            self._ev_record(self.ev_grads, self.grad_stream)
            self._ev_wait(main, self.ev_grads)
        return g

    def _reduce_plan(self, st: _Stack, rows: int, full_bwd: bool, layer: int, attn: bool = False):
        """Descriptor table (built once per row count and block) that sums into params.grad the partials of the block's MLP
        sites (c_fc, c_proj) or - attn - of its attention sites (in_proj, out_proj).  full_bwd: the dX chain runs through
        block 0's first site too (False: it ends in front of that site's dX product)."""
        key = (rows, full_bwd, layer) + (("attn",) if attn else ())
        if key not in st.plans:
            (a, b), pk = (st.asites if attn else st.sites)[layer], st.blocks[layer].packed is not None
            # (FFM_EPI_LGRAD: dA(c_proj) and dB(c_fc) hold one partial per row tile of the dX product of c_proj)
            nlg = None if attn else (st.route(rows).lgrad or None)
            # dS partial rows: those of the dX product that carries the down projection (c_proj's also the dGELU); block 0's
            # first site has no dX product where the chain ends there, and takes the stand-alone kernel
            bb, ba, bs = b.reduce_entries(rows, b.ds_rows(rows, pk, dgelu=not attn), splits_A=nlg)
            ab, aa, as_ = a.reduce_entries(rows, a.ds_rows(rows, pk, gemm=layer > 0 or full_bwd), splits_B=nlg)
            st.plans[key] = ops.ReducePlan([bs, as_, bb, ba, ab, aa], self.device)
        return st.plans[key]

    # ------------------------------------------------------------ replay --
    # A training step is a fixed sequence of C launches over static buffers plus a few host-side
    # actions (event record/wait, the PyTorch glue at the ends of the text tower).  The helpers below
    # execute an action and, while a recording is active, also append it to the replay plan.
    def _ev_record(self, ev, stream) -> None:
        ev.record(stream)
        ops.record_callable(lambda: ev.record(stream))

    def _ev_wait(self, stream, ev) -> None:
        stream.wait_event(ev)
        ops.record_callable(lambda: stream.wait_event(ev))

    def _glue(self, fn, stream=None) -> None:
        def run():
            if stream is None:
                fn()
            else:
                with torch.cuda.stream(stream):
                    fn()
        run()
        ops.record_callable(run)

    class _on:
        """Make `stream` current for the C launches issued inside (their stream pointer is baked into the
        recorded launch, so nothing is recorded for the context itself)."""

        def __init__(self, stream):
            self.ctx = torch.cuda.stream(stream)

        def __enter__(self):
            return self.ctx.__enter__()

        def __exit__(self, *a):
            return self.ctx.__exit__(*a)

    # --------------------------------------------------------------- text --
    def _text_forward(self, with_grad: bool = True, stream=None) -> None:
        """prompts = [prefix, ctx, suffix] + pos -> text tower -> EOT gather, ln_final, projection, normalise (, mean over
        the prompts) -> tbar_buf [n_cls, D], or with a transport head every prompt's normalised feature tn_buf [N*n_cls, D]
        (trainers/GLP_OT_SVLoRA.py:131-152, 55-66, 709-718): HIP kernels end to end (csrc/text.hip)."""
        cfg = self.cfg
        rows = self.n_text * self.txt_len
        ops.text_embed(self.tok_prefix, self.params.view("prompt_learner.ctx"), self.tok_suffix, self.txt_pos, self.txt.x[0],
                       cfg.n_cls, self.txt_len)
        self._stack_forward(self.txt, rows, self.n_text, None, self.txt_len)
        ops.text_tail_fwd(self.txt.x[self.txt.layers], self.eot_rows, self.lnfinal[0], self.lnfinal[1], self.text_proj, self.tf_buf,
                          self.tn_all, self.t_rnorm, self.t_stats, None if self.ot else self.tbar_buf, cfg.n_prompts, cfg.n_cls)

    def _text_backward(self, stream=None) -> None:
        """dtbar (or dtn) -> gradient of the tower's EOT rows -> tower backward -> d ctx."""
        cfg = self.cfg
        rows = self.n_text * self.txt_len
        ops.text_tail_bwd(self.txt.x[self.txt.layers], self.eot_rows, self.lnfinal[0], self.text_proj, self.tn_all, self.t_rnorm,
                          self.t_stats, None if self.ot else self.dtbar, self.dtn if self.ot else None, self.t_dy, self.txt.g,
                          cfg.n_prompts, cfg.n_cls, self.txt_len)
        self._stack_backward(self.txt, rows, self.n_text, None, self.txt_len, True)
        ops.text_ctx_grad(self.txt.g, self.params.view("prompt_learner.ctx", "grad"), cfg.n_cls, self.txt_len)

    # ---------------------------------- the ends every image tower shares --
    def _as_f32(self, image: Tensor, slot: str = "_u8_stage") -> Tensor:
        """uint8 transport (fairfedmed_amd.data, transport="uint8"): expand on the GPU to the float32 batch the
        reference's loader ships - a single SLO / X-ray channel is repeated to 3 (utils/data_utils.py:676-679).  A
        NativeBatch (transport="native") carries stored sizes and its own channel repeat: resized into the same buffer, or -
        one that carries augmentation - cropped, resampled and flipped into it (ops.augment_u8)."""
        native = isinstance(image, NativeBatch)       # transport="native": stored sizes, resized here (ffm_resize_u8)
        if not native and image.dtype != torch.uint8:
            return image
        if native:
            if not image.is_cuda:
                raise TypeError("a NativeBatch must be on the GPU (.to(device))")
            if image.R != self.cfg.vision.image_size:
                raise ValueError(f"the NativeBatch resizes to {image.R}, the tower takes {self.cfg.vision.image_size}")
            b, shape = len(image), (len(image), image.C1 * image.rep, image.R, image.R)
        else:
            if not image.is_cuda or image.dim() != 4:
                raise TypeError("uint8 images must be CUDA tensors [B, C, H, W]")
            b, c1 = image.shape[:2]
            rep = 1 if self.cfg.dim_per_3d_slice else (3 // c1 if c1 in (1, 3) else 1)
            shape = (b, c1 * rep) + tuple(image.shape[2:])
        stage = getattr(self, slot, None)             # (the evaluation pass stages in a buffer of its own)
        if stage is None or stage.shape[0] < b or tuple(stage.shape[1:]) != shape[1:]:
            stage = torch.empty(shape, device=self.device, dtype=torch.float32)
            setattr(self, slot, stage)
        if native and image.augment is not None:      # a training batch with INPUT.TRANSFORMS: every sample from its own box
            boxes = getattr(self, "_aug_boxes", None)
            if boxes is None or boxes.shape[0] < b:
                boxes = self._aug_boxes = torch.empty(b, 8, device=self.device, dtype=torch.int32)
            return ops.augment_u8(image, stage[:b], boxes[:b])
        if native:
            return ops.resize_u8(image, stage[:b])
        return ops.expand_u8(image.contiguous(), stage[:b], rep)

    def _pack_rank_operands(self) -> None:
        """ffm_lora_pack_multi over every adapter (one or two launches) on the CURRENT stream."""
        if self.pack_plan is not None:                # (fused rank only)
            self.pack_plan.run()

    def _rank_operands_ready(self) -> None:
        """In a training step the packing runs at the head of the side stream, beside the patch embedding (27 us off the
        main queue), and the vision chain waits for it here; outside a step (inference) it runs in line."""
        ev = self._pack_event
        if ev is None:
            self._pack_rank_operands()
        else:
            self._ev_wait(torch.cuda.current_stream(self.device), ev)

    def _head_forward(self, rows: int, images: int, L: int, ws=None) -> None:
        cfg = self.cfg
        ws = self if ws is None else ws               # (the text features are the engine's in either case)
        if self.ot:
            ops.ot_head_fwd(ws.feat[:rows], self.tn_buf, self.logit_scale, ws.rnorm, ws.ot_sim, ws.ot_T, ws.ot_errs,
                            ws.ot_istop, ws.ot_tsum, ws.logits_img, images, L, cfg.n_cls, cfg.n_prompts, self.ot,
                            cfg.ot_eps, cfg.ot_thresh, cfg.ot_max_iter, cfg.ot_top_percent)
        else:
            ops.head_fwd(ws.feat[:rows], self.tbar_buf, self.logit_scale, ws.fbar, ws.rnorm, ws.logits_img,
                         images, L, cfg.n_cls)

    def _head_backward(self, rows: int, images: int, L: int) -> None:
        cfg = self.cfg
        if self.ot:
            P = cfg.n_prompts * cfg.n_cls
            ops.ot_head_bwd(self.feat[:rows], self.tn_buf, self.logit_scale, self.rnorm, self.ot_T, self.dlogits_img,
                            self.dfeat[:rows], self.ot_dtn_part, images, L, cfg.n_cls, cfg.n_prompts)
            ops.reduce_partials(self.ot_dtn_part, images, P * self.cfg.vision.out_dim, self.dtn.view(-1))
        else:
            ops.head_bwd(self.feat[:rows], self.tbar_buf, self.logit_scale, self.fbar, self.rnorm, self.dlogits_img,
                         self.dfeat[:rows], self.dtbar, images, L, cfg.n_cls)

    # ---------------------------------------------------------------- API --
    @torch.no_grad()
    def forward(self, image: Tensor, attr: Optional[Tensor] = None) -> Tensor:
        """CustomCLIP.forward(image, attr) -> logits [B, n_cls] (inference)."""
        if self.sops.type != "FairLoRA":
            attr = None                               # LoRALinear / SVLoRALinear.forward ignore attr (:241, :307)
        b, S = self._load_inputs(image, attr, None)
        self._text_forward(False)
        self._vision_forward(b, S, attr is not None)
        return self.logits_img[:b * S].view(b, S, -1).mean(1)

    def _step_body(self, b: int, S: int, has_attr: bool) -> None:
        cfg, v = self.cfg, self.cfg.vision
        main = torch.cuda.current_stream(self.device)
        images, L = b * S, v.tokens
        rows = images * L
        a32 = self.attr_i32[:b] if has_attr else None
        self._ev_record(self.ev_start, main)
        self._ev_wait(self.side, self.ev_start)           # parameters of the previous step are final
        with self._on(self.side):
            self._pack_rank_operands()
            self._ev_record(self.ev_pack, self.side)
            self._text_forward(True, self.side)
        self._ev_record(self.ev_text_fwd, self.side)
        self._pack_event = self.ev_pack
        try:
            self._vision_forward(b, S, has_attr, wait=self.ev_text_fwd)
        finally:
            self._pack_event = None
        if self._fair_step:
            # set_fairness: CE + lambda * the confidence gap between the groups of the batch (attr_i32: one entry per sample /
            # volume, loaded for the loss even where the adapters take no attribute)
            ops.ce_fair_loss(self.logits_img, self.label_buf, self.attr_i32, self.logits, self.prob, self.loss,
                             self.loss_terms, self.group_conf, self.dlogits_img, self.finite, b, S, cfg.n_cls,
                             self._fair_groups(), self._fair_lam, self._fair_grad)
        else:
            ops.ce_loss(self.logits_img, self.label_buf, self.logits, self.prob, self.loss, self.dlogits_img,
                        self.finite, b, S, cfg.n_cls)
        if self.scale_state is not None:
            ops.loss_scale(self.dlogits_img[:b * S], self.scale_state)
        self._head_backward(rows, images, L)
        self._ev_record(self.ev_head_bwd, main)
        self._ev_wait(self.side, self.ev_head_bwd)
        with self._on(self.side):
            if self._counts_buf is not None:
                # the batch's evaluator counts for the trainer's per-step summary (enable_step_counts): prob is final, and
                # beside the backward pass the 20 us launch costs the chain nothing (behind the SGD step it sat between steps)
                ops.eval_counts(self.prob[:b], self.label_buf[:b], None, 0, method="pairs", out=self._counts_buf)
            self._text_backward(self.side)
        self._ev_record(self.ev_text_bwd, self.side)
        self._vision_backward(b, S, has_attr)
        self._ev_wait(main, self.ev_text_bwd)

    def forward_backward(self, image: Tensor, attr: Optional[Tensor], label: Tensor) -> Dict[str, Tensor]:
        """Forward, CE loss, backward; gradients of every trainable tensor land in params.grad.
        Returns device tensors (no host sync): loss [1], logits [B,n_cls], prob [B,n_cls], finite [1].
        The first call for a batch shape records the step's launch plan; later calls replay it.
        After set_fairness(lam != 0) and with an attribute, loss is CE + lam * F and the result also carries loss_terms [2] =
        {CE, F} and group_conf [G, 2] = {m_g, n_g}; without an attribute there is no term (as in the reference)."""
        # the loss's term reads the attribute for every adapter type (the reference applies it to LoRA / SVLoRA runs too,
        # trainers/GLP_OT_SVLoRA.py:928-948); the rank products of those types still run without one
        fair = self._fair_lam != 0.0 and attr is not None
        loss_attr = attr if fair else None
        if self.sops.type != "FairLoRA":
            attr = None
        with torch.no_grad():
            b, S = self._load_inputs(image, attr if attr is not None else loss_attr, label)
            key = (b, S, attr is not None, torch.cuda.current_stream(self.device).cuda_stream) + (("fair",) if fair else ())
            self._fair_step = fair
            plan = self.step_plans.get(key) if self.use_replay else None
            if plan is not None:
                for f in plan:
                    f()
            elif self.use_replay:
                plan = []
                with ops.record(plan):
                    self._step_body(b, S, attr is not None)
                self.step_plans[key] = plan
            else:
                self._step_body(b, S, attr is not None)
            self._after_plan(b, S)
            if self.scale_state is not None:
                ops.unscale_check(self.params.grad, self.scale_state)
            if self._drift is not None:                 # set_drift: on true-scale gradients, outside the recorded plan
                self._drift.apply(self.params.grad, self.params.flat, self.scale_state)
        out = {"loss": self.loss, "logits": self.logits[:b], "prob": self.prob[:b], "finite": self.finite}
        if self._counts_buf is not None:
            out["counts"] = self._counts_buf          # ffm_eval_counts of (prob, label): rows {unknown, all}
        if fair:
            out["loss_terms"], out["group_conf"] = self.loss_terms, self.group_conf[:self._fair_groups()]
        return out

    @torch.no_grad()
    def sgd_step(self, lr: float, momentum: float, weight_decay: float, repeats: int = 1) -> None:
        """optim.step(), `repeats` times on the gradients of the last forward_backward (one launch)."""
        p = self.params
        if self.scale_state is not None:                # fp16: skipped when the gradients overflowed; the scale then halves
            ops.sgd_momentum_gated(p.flat, p.grad, p.momentum, lr, momentum, weight_decay, p.steps == 0, repeats, self.scale_state)
        else:
            ops.sgd_momentum(p.flat, p.grad, p.momentum, lr, momentum, weight_decay, p.steps == 0, repeats)
        p.steps += repeats

    @torch.no_grad()
    def optim_step(self, spec, lr: float, repeats: int = 1) -> None:
        """optim.step() of adam / adamw / amsgrad / rmsprop / radam (fairfedmed_amd.optim.OptimSpec), `repeats` times on the
        gradients of the last forward_backward at the step numbers steps+1 .. steps+repeats, in one launch.  fp16: gated on the
        gradient-scale state, with the step count and the running powers in device memory (ffm_optim_step_dev) - on an
        overflowed step nothing moves but the scale, and the next good step applies the next step number."""
        p = self.params
        p.set_optim_rows(spec.rows)
        if self.scale_state is not None or p.optim_desc is not None:       # (a captured step's counter block stays the truth)
            self.optim_desc_dev(spec, lr)
            ops.optim_step_dev(p.flat, p.grad, p.optim_state, spec.kind, p.optim_desc, repeats, self.scale_state)
        else:
            ops.optim_step(p.flat, p.grad, p.optim_state, spec.kind, spec.desc(lr, p.steps), repeats)
        p.steps += repeats

    def optim_desc_dev(self, spec, lr: float) -> Tensor:
        """The device-resident ffm_optim_desc: created at the host's step count, afterwards only its lr is written."""
        p = self.params
        if p.optim_desc is None:
            p.optim_desc = torch.tensor(spec.desc_values(lr, p.steps), dtype=torch.float64, device=self.device)
            p.optim_desc_lr = lr
        elif p.optim_desc_lr != lr:
            p.optim_desc[0:1].fill_(lr)
            p.optim_desc_lr = lr
        return p.optim_desc

    def set_optim_steps(self, spec, lr: float, steps: int) -> None:
        """Position the optimizer at `steps` applications (a loaded checkpoint, a state handed on by another rank)."""
        p = self.params
        p.steps = int(steps)
        if p.optim_desc is not None:
            p.optim_desc.copy_(torch.tensor(spec.desc_values(lr, p.steps), dtype=torch.float64))
            p.optim_desc_lr = lr

    def optim_steps(self) -> int:
        """Optimizer applications made so far: the device counter where there is one (it does not move on a skipped fp16
        step; reading it synchronises), the host count otherwise."""
        p = self.params
        return int(p.optim_desc[9]) if p.optim_desc is not None else p.steps

    def enable_step_counts(self, on: bool = True) -> None:
        """Binary tasks: every training step also leaves ffm_eval_counts(prob, label) in out["counts"] (int64 [2, 10]: the
        integers behind the reference's per-step accuracy / AUC summary, trainers/GLP_OT_SVLoRA.py:959-970), computed on the
        side stream beside the backward pass."""
        want = on and self.cfg.n_cls == 2
        if want != (self._counts_buf is not None):
            self._counts_buf = torch.zeros(2, ops.EVAL_SLOTS, device=self.device, dtype=torch.int64) if want else None
            self.step_plans.clear()

    def set_fairness(self, lam: float, with_grad: bool = False) -> None:
        """TRAINER.LAMBDA_FAIRNESS on the device: with lam != 0 a training step that is given an attribute computes its loss
        with ffm_ce_fair_loss - CE + lam * F, F the mean absolute deviation of the groups' mean (1 - p[label]) over the groups
        present in the batch (trainers/GLP_OT_SVLoRA.py:928-948) - for every adapter type; lam == 0 is ffm_ce_loss and
        today's plans.  with_grad False (default) is the reference: the term is built from detached values and moves the
        reported loss only.  with_grad True is an extension beyond the reference: the term's gradient joins dloss/dlogits
        and training changes.  Both scalars are baked into recorded launches, so the plans are dropped here, and a
        captured step (capture_train_step) keeps the values it was captured with: call this BEFORE the capture."""
        lam, with_grad = float(lam), bool(with_grad)
        if (lam, with_grad) != (self._fair_lam, self._fair_grad):
            self._fair_lam, self._fair_grad = lam, with_grad
            self.step_plans.clear()

    def set_drift(self, corrector) -> None:
        """Client-drift correction of the local step (fairfedmed_amd.drift.DriftCorrector; an
        extension beyond the reference): with a corrector, every forward_backward ends in one more launch - ffm_drift_correct
        on params.grad, behind the plan and (fp16) behind unscale_check, so it sees true-scale gradients and is skipped with
        an overflowed step - in front of whichever optimizer step follows; None (the default) launches nothing.  The launch
        is not part of the recorded plans, so they stay as they are.  A captured step (capture_train_step) contains the
        launch if it was captured after this call, with the corrector's buffers by address and FedProx's mu baked in: call
        this BEFORE the capture, as set_fairness.  The reported loss stays the task loss."""
        self._drift = corrector

    def _fair_groups(self) -> int:
        """Groups the loss's term looks for: the adapters' for FairLoRA (an attribute beyond them could not pass through
        FairLoRALinear), every index the library knows for the types that carry no groups (num_groups is 1 there)."""
        return self.cfg.lora.num_groups if self.sops.type == "FairLoRA" else ops.MAX_GROUPS

    def set_overlap(self, on: bool) -> None:
        """on: text tower and LoRA-gradient reductions run on their own streams beside the vision chain
        (default).  off: everything on the caller's stream, one kernel at a time (clean per-kernel timings)."""
        cur = torch.cuda.current_stream(self.device)
        if on:
            self.side, self.grad_stream = self._side0, self._grad0
        else:
            self.side = self.grad_stream = cur
        self.step_plans.clear()

    # ------------------------------------------------------------- graph --
    def capture_train_step(self, batch_size: int, lr: float, momentum: float, weight_decay: float,
                           repeats: int = 1, optimizer=None) -> "GraphedStep":
        """Capture forward + backward + SGD (all three streams) into one hipGraph.  set_fairness must precede the capture
        (the loss kernel and its scalars are part of the graph).  A step then costs the
        host one graph launch instead of ~450 Python->C calls (the eager loop is host-bound at ~7 ms).  A replay trains
        as forward_backward + sgd_step(lr, momentum, weight_decay, repeats) does, fp16 gradient-scale gating included.
        optimizer: an OptimSpec (fairfedmed_amd.optim) - the body then ends in ffm_optim_step_dev and a replay trains as
        forward_backward + optim_step(optimizer, lr, repeats) does (momentum / weight_decay come from the spec)."""
        return GraphedStep(self, batch_size, lr, momentum, weight_decay, repeats, optimizer)

    def trainable_state(self) -> Dict[str, Tensor]:
        return {k: self.params.view(k) for k in self.params.keys}


class FairLoRAEngine(ClipEngine):
    """ClipEngine with CLIP's VisionTransformer as the image tower: patch embedding (behind the 3D slice front end, where
    the config has one), the `_Stack` of vision blocks, ln_post and the projection - and the forward-only pass (`infer`) on a
    workspace of its own."""

    def __init__(self, cfg: ModelCfg, state_dict: Dict[str, Tensor], dtype=torch.bfloat16, max_images: int = 32,
                 device: str = "cuda:0", max_infer_images: Optional[int] = None):
        """max_infer_images (default: max_images) sizes the depth-independent workspace of the forward-only pass (infer)."""
        super().__init__(cfg, state_dict, dtype, max_images, device, max_infer_images)
        self._in_session = False
        self._init_infer()

    # ----------------------------------------------------------------- setup --
    def _init_vision(self, max_images: int) -> None:
        cfg, v, dtype, dev = self.cfg, self.cfg.vision, self.dtype, self.device
        self.vis = _Stack(v.width, v.heads, v.layers, v.tokens, max_images, False, cfg.lora.rank, dtype, dev, self.sw,
                          targets=Targets.of(cfg.lora))
        P = v.grid * v.grid
        self.cols = torch.zeros(max_images * P, 3 * v.patch * v.patch, device=dev, dtype=dtype)
        self.patch_out = torch.zeros(max_images * P, v.width, device=dev, dtype=dtype)
        self.hpost = torch.zeros(max_images * v.tokens, v.width, device=dev, dtype=dtype)
        self.post_stats = (torch.zeros(max_images * v.tokens, device=dev), torch.zeros(max_images * v.tokens, device=dev))
        f32 = torch.float32
        self.is3d = cfg.dim_per_3d_slice > 0
        if self.is3d:
            D, H = cfg.dim_per_3d_slice, v.image_size
            nblk = ops.slice_blocks(H, H)
            self.conv_out = torch.zeros(max_images, 3, H, H, device=dev, dtype=f32)
            self.dconv = torch.zeros_like(self.conv_out)
            self.mm_part = torch.zeros(max_images * nblk * 2, device=dev, dtype=f32)
            self.mnmx = torch.zeros(max_images, 2, device=dev, dtype=f32)
            self.mm_cnt = torch.zeros(max_images, 2, device=dev, dtype=torch.int32)
            self.ab_part = torch.zeros(max_images * ops.slice_bwd_ab_blocks() * 2, device=dev, dtype=f32)
            self.gmm = torch.zeros(max_images, 2, device=dev, dtype=f32)
            self.wpart = torch.zeros(max_images * ops.slice_wgrad_blocks(H, H) * (3 * D * 25 + 3), device=dev, dtype=f32)
            self.dcols = torch.zeros_like(self.cols)
            self.dpatch = torch.zeros_like(self.patch_out)
        # _stack_backward: one event per block for its MLP sites' reductions, one more for the attention sites'
        self.ev_layer = [torch.cuda.Event() for _ in range(v.layers)]
        if Targets.of(cfg.lora).attn:
            self.ev_attn = [torch.cuda.Event() for _ in range(v.layers)]

    def _init_vision_late(self) -> None:
        """After the frozen weights are loaded: the tower's LoRA sites and the table that packs their rank operands."""
        cfg, v, dtype, dev = self.cfg, self.cfg.vision, self.dtype, self.device
        ie = "image_encoder.transformer.resblocks."
        tg = self.vis.targets
        names = (["attn.in_proj_lora.", "attn.out_proj_lora."] if tg.attn else []) + (["mlp.c_fc.", "mlp.c_proj."] if tg.mlp else [])
        self.sops = SOperands(self.params, [f"{ie}{i}.{n}" for i in range(v.layers) for n in names], cfg, dev)
        st, w, r, h16, T = self.vis, v.width, cfg.lora.rank, _is16(dtype), self.vis.max_rows
        if not r:
            return
        for i, blk in enumerate(st.blocks):
            if tg.mlp:
                # c_fc has ln_2 folded into it (Route.ln2): its rank operand gamma-scaled too, and - ln_2's backward fold
                # (Route.ln2_bwd) - the rank operand of dX(c_fc) carries W gamma and W beta + b as rows 14 / 15: its t[14] / t[15]
                # are the two row sums against those vectors, out of the matrix cores; every consumer masks the slots beyond r
                fc = LoraSite(self, f"{ie}{i}.mlp.c_fc.", w, 4 * w, T, u=st.u, wide=h16, ln=(blk.ln2_w, blk.ln2_b) if h16 else None,
                              row1415=(blk.c_fc, blk.d_fc) if (h16 and blk.c_fc is not None and r <= 14) else None)
                proj = LoraSite(self, f"{ie}{i}.mlp.c_proj.", 4 * w, w, T, u=st.u, wide=h16)
                st.sites.append((fc, proj))
            if tg.attn:
                # the in-projection takes ln_1 folded into the qkv product (Route.ln1) as c_fc takes ln_2; ln_1's backward
                # is never folded for it (tower_route), so its dX product carries no row sums
                ain = LoraSite(self, f"{ie}{i}.attn.in_proj_lora.", w, 3 * w, T, u=st.u, wide=h16,
                               ln=(blk.ln1_w, blk.ln1_b) if h16 else None)
                aout = LoraSite(self, f"{ie}{i}.attn.out_proj_lora.", w, w, T, u=st.u, wide=h16)
                st.asites.append((ain, aout))
        # dS partials: one size for the tower, the largest of ffm_lora_down's blocks and of the row tiles of either kernel
        # ffm_gemm_nt may pick for the dX products (c_proj's carries the dGELU)
        last = (st.sites[-1] if tg.mlp else ()) + (st.asites[-1] if tg.attn else ())
        nb = max([ops.lora_down_blocks_max(T, s.N, r, dtype) for s in last]
                 + [s.ds_tiles(T, p, dgelu=s.prefix.endswith("mlp.c_proj.")) for s in last for p in (False, True)])
        for s in (s for pair in st.sites + st.asites for s in pair):
            s.alloc_ds(nb * 8 * r)
        if self.fused_rank:
            # one table for all blocks, in the order (fc A, proj A, fc B, proj B, fc A with ln_2) per block; behind them the
            # attention sites' (in A, out A, in B, out B, in A with ln_1) per block
            ent = []
            for fc, proj in st.sites + st.asites:
                (fa, fb, *fln), (pa, pb) = fc.pack_entries(), proj.pack_entries()
                ent += [fa, pa, fb, pb, *fln]
            self.pack_plan = ops.PackPlan(ent, dtype, dev)

    def _init_infer(self) -> None:
        """The evaluation pass's workspace."""
        if self.max_infer_images < 1:
            raise ValueError(f"max_infer_images must be positive, got {self.max_infer_images}")
        self.infer_ws = _InferWorkspace(self, self.max_infer_images)

    def _load_vision_frozen(self, sd: Dict[str, Tensor], put) -> None:
        cfg, v = self.cfg, self.cfg.vision
        ie = "image_encoder."
        self._load_stack(self.vis, sd, ie, True)
        put("conv_w", self._w(sd[ie + "conv1.weight"].reshape(v.width, -1)))
        if cfg.dim_per_3d_slice:
            put("conv_w_t", self._wt(sd[ie + "conv1.weight"].reshape(v.width, -1)))   # dX of the patch embedding
        put("cls", self._w(sd[ie + "class_embedding"]))
        put("pos", self._w(sd[ie + "positional_embedding"]))
        put("lnpre", (self._f(sd[ie + "ln_pre.weight"]), self._f(sd[ie + "ln_pre.bias"])))
        put("lnpost", (self._f(sd[ie + "ln_post.weight"]), self._f(sd[ie + "ln_post.bias"])))
        put("proj", self._w(sd[ie + "proj"]))                     # [width, out]: B operand of dh = df proj^T
        put("proj_t", self._wt(sd[ie + "proj"]))                  # [out, width]: B operand of f = h proj
        # the three frozen weights outside the blocks in MFMA-fragment order too (16-bit modes): patch embedding and the
        # two products of the final projection take the panel kernel where their shape fills the chip
        if _is16(self.dtype) and self.sw.pack_out:
            for name in ("conv_w", "proj", "proj_t"):
                w = getattr(self, name)
                if w.shape[0] % 16 == 0 and w.shape[1] % 32 == 0:
                    self.pk_out[name] = ops.pack_b(w, self.pk_out.get(name))

    # ---------------------------------------------------------------- inputs --
    def _check_batch(self, image: Tensor, limit: Optional[int] = None, what: str = "max_images") -> Tuple[int, int]:
        cfg, v = self.cfg, self.cfg.vision
        limit = self.max_images if limit is None else limit
        if not image.is_cuda or image.dtype != torch.float32:
            raise TypeError("image must be a float32 CUDA tensor of raw 0..255 values")
        b, c, h, w = image.shape
        D = cfg.dim_per_3d_slice
        if h != v.image_size or w != v.image_size or (not D and c != 3) or (D and c % D):
            raise ValueError(f"expected [B,{'S*%d' % D if D else 3},{v.image_size},{v.image_size}], "
                             f"got {tuple(image.shape)}")
        S = c // D if D else 1                       # slices per sample: the ViT batch is b*S (:683-684)
        if b * S > limit:
            raise ValueError(f"{b * S} ViT images exceed the engine's {what}={limit}")
        return b, S

    def _load_inputs(self, image: Tensor, attr: Optional[Tensor], label: Optional[Tensor], ws=None) -> Tuple[int, int]:
        """Per-step inputs -> static buffers (these three launches are the only ones not replayed).  ws: the evaluation
        pass's workspace instead of the engine's own (training) buffers."""
        cfg, v = self.cfg, self.cfg.vision
        if ws is None:
            image = self._as_f32(image)
            b, S = self._check_batch(image)
            ws = self
        else:
            image = self._as_f32(image, "_u8_stage_infer")
            b, S = self._check_batch(image, ws.max_images, "max_infer_images")
        images = b * S
        P = v.grid * v.grid
        if self.is3d:
            # trainable 5x5 slice conv + per-image min-max (trainers/GLP_OT_SVLoRA.py:681-690), then the patches
            image = image.contiguous()
            if ws is self:
                self._image = image                   # (the backward of the slice convolution reads it)
            ops.slice_conv_fwd(image, self.params.view("proj_per_3d_slice.weight"),
                               self.params.view("proj_per_3d_slice.bias"), ws.conv_out[:images], ws.mm_part,
                               ws.mnmx, ws.mm_cnt, cfg.dim_per_3d_slice)
            ops.patchify_minmax(ws.conv_out[:images], ws.mnmx, ws.mm_cnt, ws.cols[:images * P], v.patch,
                                cfg.pixel_mean, cfg.pixel_std)
        else:
            ops.patchify(image.contiguous(), ws.cols[:images * P], v.patch, cfg.pixel_mean, cfg.pixel_std)
        if attr is not None:
            ws.attr_i32[:b].copy_(attr)
        if label is not None:
            self.label_buf[:b].copy_(label)
        return b, S

    # ---------------------------------------------------------------- forward --
    def _vision_forward(self, b: int, S: int, has_attr: bool, wait=None, ws=None) -> None:
        """Patch embedding -> tower -> ln_post, projection -> logits head.  ws None: on the engine's own buffers and the
        tower's stash (training, forward()), S_eff and the rank operands refreshed on the way.  ws an `_InferWorkspace`: the
        same launches on the workspace; whoever calls has refreshed S_eff and the rank operands (infer / inference)."""
        cfg, v = self.cfg, self.cfg.vision
        images = b * S
        P, L = v.grid * v.grid, v.tokens
        rows = images * L
        train = ws is None
        ws = self if train else ws
        bufs = self.vis if train else ws
        a32 = ws.attr_i32[:b] if has_attr else None
        if train and self.sops.glob:
            self._glue(self.sops.prepare)             # S_eff = S + S_global
        ops.gemm_nt(ws.cols[:images * P], self.conv_w, ws.patch_out[:images * P], b_packed=self.pk_out.get("conv_w"))
        lb0 = bufs.layer(0, rows)
        ops.embed_lnpre(ws.patch_out[:images * P], self.cls, self.pos, self.lnpre[0], self.lnpre[1],
                        lb0.x, images, L, rowstat=lb0.rowp)
        if train:
            self._rank_operands_ready()               # LoRA matrices -> GEMM rank operands (they change every step)
        out = self._stack_forward(self.vis, rows, images, a32, L * S, bufs)
        ops.layernorm_fwd(out, ws.hpost[:rows], self.lnpost[0], self.lnpost[1], ws.post_stats[0], ws.post_stats[1])
        ops.gemm_nt(ws.hpost[:rows], self.proj_t, ws.feat[:rows], b_packed=self.pk_out.get("proj_t"))
        if wait is not None:
            self._ev_wait(torch.cuda.current_stream(self.device), wait)     # text features ready
        self._head_forward(rows, images, L, ws)

    # --------------------------------------------------------------- backward --
    def _vision_backward(self, b: int, S: int, has_attr: bool) -> None:
        """dfeat -> gradients of every trainable tensor of the image side (params.grad)."""
        cfg, v = self.cfg, self.cfg.vision
        images, L = b * S, v.tokens
        rows = images * L
        a32 = self.attr_i32[:b] if has_attr else None
        ops.gemm_nt(self.dfeat[:rows], self.proj, self.vis.dh[:rows], b_packed=self.pk_out.get("proj"))
        # (straight into the buffer the last block's LoRA-gradient reductions read: no copy on the main stream)
        gl = bool(self.vis.sites)
        ops.layernorm_bwd(self.vis.dh[:rows], self.vis.x[v.layers][:rows], self.lnpost[0], self.post_stats[0],
                          self.post_stats[1], None, (self.vis.g_l[v.layers - 1] if gl else self.vis.g)[:rows])
        self._stack_backward(self.vis, rows, images, a32, L * S, self.is3d, grad_in_last=gl)
        if self.is3d:
            # dL/d(tokens) -> ln_pre / pos-add backward -> dX of the patch embedding (columns of the patches)
            P = v.grid * v.grid
            ops.embed_lnpre_bwd(self.vis.g[:rows], self.patch_out[:images * P], self.pos, self.lnpre[0],
                                self.dpatch[:images * P], images, L)
            ops.gemm_nt(self.dpatch[:images * P], self.conv_w_t, self.dcols[:images * P])

    def _after_plan(self, b: int, S: int) -> None:
        """The 3D front end's tail: the slice convolution's backward reads the caller's image (`_image`), so it is launched
        on every step, not replayed."""
        if self.is3d:
            images, P, D = b * S, self.cfg.vision.grid ** 2, self.cfg.dim_per_3d_slice
            ops.slice_bwd(self.dcols[:images * P], self._image, self.conv_out[:images], self.mnmx, self.mm_cnt,
                          self.dconv[:images], self.ab_part, self.gmm, self.wpart, D, self.cfg.vision.patch,
                          self.cfg.pixel_std)
            nw = 3 * D * 25 + 3
            off = self.params.offsets["proj_per_3d_slice.weight"][0]
            assert self.params.offsets["proj_per_3d_slice.bias"][0] == off + nw - 3
            nblk = ops.slice_wgrad_blocks(self.cfg.vision.image_size, self.cfg.vision.image_size)
            ops.reduce_partials(self.wpart, images * nblk, nw, self.params.grad[off:off + nw])

    # -------------------------------------------------------------- evaluation --
    def _infer_prepare(self) -> None:
        """What an evaluation needs from the CURRENT parameters besides the vision pass: the rank operands of the FairLoRA
        products, S_eff (GLOBAL_S) and the text features."""
        self._pack_rank_operands()
        if self.sops.glob:
            self.sops.prepare()
        self._text_forward(False)

    def inference(self):
        """``with eng.inference():`` - an evaluation session.  On entry the rank operands are packed from the current
        parameters, S_eff is refreshed and the text tower runs ONCE; inside, `infer` runs the vision tower and the head
        only.  The session is the contract: the parameters must not be stepped (sgd_step, a captured step, load) inside it -
        nothing looks for stale operands.  Sessions do not nest usefully (an inner one prepares again)."""
        eng = self

        class _Session:
            def __enter__(self):
                with torch.no_grad():
                    eng._infer_prepare()
                self.prev, eng._in_session = eng._in_session, True
                return eng

            def __exit__(self, *a):
                eng._in_session = self.prev
                return False
        return _Session()

    @torch.no_grad()
    def infer(self, image: Tensor, attr: Optional[Tensor] = None) -> Tensor:
        """forward()'s logits [B, n_cls], bit for bit, by the forward-only pass: the same launches in the same order on the
        inference workspace (up to max_infer_images ViT images), with nothing stored for a backward pass - c_fc leaves the
        activation alone (FFM_EPI_GELU_ONLY), no rank vectors, no log-sum-exp, no LayerNorm statistics.  Gradients,
        momentum, the training stash, the step-count buffers, the fp16 scale state and a captured training step are not
        touched.  Outside an `inference()` session every call prepares the rank operands and the text features itself."""
        if self.sops.type != "FairLoRA":
            attr = None                               # LoRALinear / SVLoRALinear.forward ignore attr (:241, :307)
        ws = self.infer_ws
        b, S = self._load_inputs(image, attr, None, ws=ws)
        if not self._in_session:
            self._infer_prepare()
        self._vision_forward(b, S, attr is not None, ws=ws)
        return ws.logits_img[:b * S].view(b, S, -1).mean(1)


class GraphedStep:
    """One captured training step.  ``run(image, attr, label)`` copies the batch into the static input
    buffers and replays the graph; results are the engine's usual device tensors (loss, logits, prob, finite)."""

    def __init__(self, eng: ClipEngine, batch_size: int, lr: float, momentum: float, weight_decay: float,
                 repeats: int = 1, optimizer=None):
        if not 1 <= repeats <= 16:
            raise ValueError(f"repeats must be 1..16, got {repeats}")
        self.eng = eng
        self.repeats = repeats
        self.spec = optimizer if (optimizer is not None and optimizer.kind != "sgd") else None
        eng.use_replay = False                        # the hipGraph replaces the recorded launch plan
        v, dev = eng.cfg.vision, eng.device
        self.image = torch.zeros(batch_size, 3, v.image_size, v.image_size, device=dev)
        self.attr = torch.zeros(batch_size, device=dev, dtype=torch.int64)
        self.label = torch.zeros(batch_size, device=dev, dtype=torch.int64)
        p = eng.params
        # SGD reads {lr, momentum, weight_decay} from hp; an optimizer spec reads the device-resident ffm_optim_desc instead
        self.hp = torch.tensor([lr, momentum, weight_decay], device=dev, dtype=torch.float32) if self.spec is None else None
        if self.spec is not None:
            p.set_optim_rows(self.spec.rows)
        if p.steps == 0:
            p.optim_state.zero_()                     # every state row (SGD: the momentum buffer)
        # everything a body writes that outlives a step: the weights, their momentum and gradients, the loss flag and (fp16)
        # the gradient-scale state, which the gated update moves
        live = [p.flat, p.momentum, p.grad, eng.finite] + ([eng.scale_state] if eng.scale_state is not None else [])
        if self.spec is not None:                     # every state row and the device-resident step count / powers
            live = [p.flat, p.optim_state, p.grad, eng.finite, eng.optim_desc_dev(self.spec, lr)] + live[4:]
        if eng._drift is not None:                    # set_drift: the running gradient sum and its step count
            live = live + eng._drift.live()
        keep, steps = [t.clone() for t in live], p.steps

        def restore():
            for t, k in zip(live, keep):
                t.copy_(k)
            p.steps = steps

        # warm-up off the default stream (sets kernel attributes, sizes the allocator), then restore the state
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                self._body()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        restore()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._body()
        restore()
        torch.cuda.synchronize(dev)

    def _body(self):
        out = self.eng.forward_backward(self.image, self.attr, self.label)
        with torch.no_grad():
            p = self.eng.params
            # fp16: skipped when the gradients overflowed, then the scale moves (as sgd_step's gated update)
            if self.spec is not None:
                ops.optim_step_dev(p.flat, p.grad, p.optim_state, self.spec.kind, p.optim_desc, self.repeats,
                                   self.eng.scale_state)
            else:
                ops.sgd_momentum_dev(p.flat, p.grad, p.momentum, self.hp, self.repeats, self.eng.scale_state)
        return out

    def set_lr(self, lr: float) -> None:
        if self.spec is not None:
            self.eng.optim_desc_dev(self.spec, lr)
        else:
            self.hp[0:1].fill_(lr)

    def run(self, image: Optional[Tensor] = None, attr: Optional[Tensor] = None, label: Optional[Tensor] = None):
        if image is not None:
            self.image.copy_(image, non_blocking=True)
        if attr is not None:
            self.attr.copy_(attr, non_blocking=True)
        if label is not None:
            self.label.copy_(label, non_blocking=True)
        self.graph.replay()
        self.eng.params.steps += self.repeats
        return self.out
