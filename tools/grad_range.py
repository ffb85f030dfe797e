#!/usr/bin/env python3
"""Where the gradient operands of the backward kernels live in one IEEE-half training step.

One process, one fp16 `forward_backward` at the default gradient scale (FFM_F16_GRAD_SCALE, 2^12).  The step's first call
runs every launch eagerly (it is being recorded), so each backward entry point of fairfedmed_amd.ops is wrapped for that one
call: the wrapper synchronises the device, reads the gradient operand(s) from the engine's own buffers as the kernel is about
to see them (operands a kernel produces for itself - the `us` of a fused rank product, which FFM_EPI_LGRAD then feeds to the
matrix cores - are read behind the launch), and hands on to the real function.  No kernel is changed or instrumented.

For every (kernel, operand) it prints, over the blocks of the tower: min and max of the rms of the non-zero entries, the
largest |.|, the largest share of entries with |.| < 2^-14 (half's smallest normal; zeros included) and the share of zeros.
The table of docs/experiments.md "fp16: gradient magnitudes by kernel" is this output for

    timeout 600 python tools/grad_range.py --model vit_b16 --batch 32
    timeout 600 python tools/grad_range.py --model vit_tiny --batch 8

and, for the kernels these two never launch, --model vit_b16 --rank 16 --batch 1 --slices 25 / --model vit_tiny --batch 2
--slices 4 (the 3D front end: embed_lnpre_bwd, slice_bwd) and --model rn50 --batch 32 / --model rn_tiny --batch 8 (the RN50 tower).

--json FILE also writes the rows as JSON.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fairfedmed_amd import config as C, ops, synth
from fairfedmed_amd.engine import FairLoRAEngine

TINY = 2.0 ** -14
SITES = []                  # every LoraSite of the engine (filled in main)


class Ranges:
    def __init__(self):
        self.rows = {}            # (kernel, operand) -> list of (rms, max, share_tiny, share_zero, dtype)
        self.backward = False

    def see(self, kernel, operand, t):
        if t is None or not self.backward:
            return
        torch.cuda.synchronize()
        a = t.detach().double().abs().flatten()
        nz = a[a > 0]
        rms = float(nz.pow(2).mean().sqrt()) if nz.numel() else 0.0
        self.rows.setdefault((kernel, operand), []).append(
            (rms, float(a.max()) if a.numel() else 0.0, float((a < TINY).double().mean()), float((a == 0).double().mean()),
             str(t.dtype).replace("torch.", "")))

    def table(self):
        out = []
        for (kernel, operand), v in self.rows.items():
            rms = [x[0] for x in v if x[0] > 0] or [0.0]
            out.append(dict(kernel=kernel, operand=operand, dtype=v[0][4], calls=len(v), rms_min=min(rms), rms_max=max(rms),
                            max=max(x[1] for x in v), tiny=max(x[2] for x in v), zero=max(x[3] for x in v)))
        return out


def lg2(x):
    return "   -inf" if x <= 0 else "%7.2f" % math.log2(x)


def wrap(R):
    """Replace the backward entry points of `ops` by wrappers that report their gradient operands to R."""
    real = {n: getattr(ops, n) for n in ("gemm_nt", "attention_bwd", "layernorm_bwd", "embed_lnpre_bwd", "lora_down", "lora_grad_partial",
                                         "lora_grad_partial_ln", "reduce_partials", "head_bwd", "ot_head_bwd", "text_tail_bwd",
                                         "text_ctx_grad", "slice_bwd", "loss_scale", "ce_loss", "ce_fair_loss", "bn_bwd", "col2im3x3",
                                         "relu_bwd", "avgpool2", "attnpool_tokens", "conv3x3")}
    real_plan_run = ops.ReducePlan.run

    def start(name):
        def f(*a, **k):
            real[name](*a, **k)
            R.backward = True                   # everything behind the loss (and its scaling) is the backward pass
        return f

    def gemm_nt(a, b, out, **k):
        if not R.backward:
            return real["gemm_nt"](a, b, out, **k)
        ro, la = k.get("rankop"), k.get("lnb_apply")
        tower = "text x3" if a.dtype == torch.float32 and k.get("x3") else "panel" if k.get("b_packed") is not None else "128x128"
        if k.get("bnbwd") is not None:
            name = "FFM_EPI_BNBWD" + (" + RankOp" if ro is not None else "")
        elif la is not None:
            name = "FFM_EPI_LNB_APPLY" + (" + RankOp" if ro is not None else "")
        elif ro is not None and ro.lgrad is not None:
            name = "FFM_EPI_LGRAD" + (" + FFM_EPI_LNB_STAT" if k.get("lnb_stat") is not None else "")
        elif ro is not None:
            name = ("proj_dx" if k.get("dgelu_aux") is not None else "fc_dx") + " RankOp(t_fwd, ds_part)"
        elif k.get("ts") is not None:
            name = "ts / lw" + (" + dgelu_aux" if k.get("dgelu_aux") is not None else "")
        else:
            name = "dgelu_aux" if k.get("dgelu_aux") is not None else "plain"
        name = f"gemm_nt dX [{tower}] {name}"
        R.see(name, "a (dL/dy)", a)
        R.see(name, "ts (us)", k.get("ts"))
        if k.get("bnbwd") is not None:
            R.see(name, "res", k.get("res"))
        if la is not None:
            R.see(name, "res", la.res)
            R.see(name, "part (row sums)", la.part[:la.np])
        r = real["gemm_nt"](a, b, out, **k)
        if ro is not None and ro.lgrad is not None:
            R.see(name, "hi + lo operand of dA(c_proj): us, as the launch wrote it", ro.ts_out)
        return r

    def attention_bwd(qkv, o, dout, *a, **k):
        R.see("attention_bwd" + (" (lnstat)" if k.get("ln_stat") is not None else "") + (" f32" if qkv.dtype == torch.float32 else ""),
              "dout", dout)
        return real["attention_bwd"](qkv, o, dout, *a, **k)

    def layernorm_bwd(dy, x, gamma, mean, rstd, res, out):
        R.see("layernorm_bwd" + (" f32" if dy.dtype == torch.float32 else ""), "dy", dy)
        R.see("layernorm_bwd" + (" f32" if dy.dtype == torch.float32 else ""), "res", res)
        return real["layernorm_bwd"](dy, x, gamma, mean, rstd, res, out)

    def embed_lnpre_bwd(dx, *a, **k):
        R.see("embed_lnpre_bwd", "dx", dx)
        return real["embed_lnpre_bwd"](dx, *a, **k)

    def lora_down(x, P, layout_rk, *a, **k):
        if layout_rk:                            # u = g B^T: the backward's down projection
            R.see("lora_down (ds_part)" + (" f32" if x.dtype == torch.float32 else ""), "x (dL/dy)", x)
        return real["lora_down"](x, P, layout_rk, *a, **k)

    def lora_grad_partial(x, v, r, part):
        # dB = g^T ts (LoraSite.grad_B: x is the gradient, v the forward's ts) and dA = x^T us (grad_A: v is the gradient),
        # told apart by whose buffer v is
        f32 = " f32" if x.dtype == torch.float32 else ""
        site = next((s for s in SITES if s.ts.data_ptr() == v.data_ptr()), None)
        if site is not None:
            R.see("lora_grad_partial dB = g^T ts" + f32, "x (dL/dy)", x)
            R.see("lora_grad_partial dB = g^T ts" + f32, "v (the forward's ts: no gradient; fp32, hi + lo)", v)
        else:
            R.see("lora_grad_partial dA = x^T us" + f32, "v (us; fp32, hi + lo)", v)
        return real["lora_grad_partial"](x, v, r, part)

    def lora_grad_partial_ln(x, v, *a, **k):
        R.see("lora_grad_partial_ln", "v (us, fp32, hi + lo)", v)
        return real["lora_grad_partial_ln"](x, v, *a, **k)

    def reduce_partials(part, nsplit, n, out, *a, **k):
        R.see("reduce_partials", "part", part.flatten()[:nsplit * n])
        return real["reduce_partials"](part, nsplit, n, out, *a, **k)

    def plan_run(self):
        for e in self.keep:
            R.see("reduce_partials (ReducePlan)", "part", e[0].flatten()[:e[1] * e[2]])
        return real_plan_run(self)

    def head_bwd(f, tbar, ls, fbar, rnorm, dl, *a, **k):
        R.see("head_bwd", "dlogits_img", dl)
        return real["head_bwd"](f, tbar, ls, fbar, rnorm, dl, *a, **k)

    def ot_head_bwd(f, tn, ls, rnorm, T, dl, *a, **k):
        R.see("ot_head_bwd", "dlogits_img", dl)
        return real["ot_head_bwd"](f, tn, ls, rnorm, T, dl, *a, **k)

    def text_tail_bwd(x, eot, lnw, proj, tn, rn, st, dtbar, dtn, *a, **k):
        R.see("text_tail_bwd f32", "dtbar / dtn", dtbar if dtbar is not None else dtn)
        return real["text_tail_bwd"](x, eot, lnw, proj, tn, rn, st, dtbar, dtn, *a, **k)

    def text_ctx_grad(g, *a, **k):
        R.see("text_ctx_grad f32", "g", g)
        return real["text_ctx_grad"](g, *a, **k)

    def slice_bwd(dcols, *a, **k):
        R.see("slice_bwd", "dcols", dcols)
        return real["slice_bwd"](dcols, *a, **k)

    # the RN50 tower (fairfedmed_amd/engine_rn.py)
    def bn_bwd(dy, *a, **k):
        R.see("bn_bwd" + (" (column sums from the producer)" if k.get("part_rows") else ""), "dy", dy)
        return real["bn_bwd"](dy, *a, **k)

    def col2im3x3(dcols, *a, **k):
        R.see("col2im3x3", "dcols", dcols)
        return real["col2im3x3"](dcols, *a, **k)

    def relu_bwd(g, *a, **k):
        R.see("relu_bwd", "g", g)
        return real["relu_bwd"](g, *a, **k)

    def avgpool2(inp, out, B, H, W, backward=False):
        if backward:
            R.see("avgpool2 backward", "d(pooled)", inp)
        return real["avgpool2"](inp, out, B, H, W, backward)

    def attnpool_tokens(inp, pos, out, B, HW, backward=False):
        if backward:
            R.see("attnpool_tokens backward", "d(tokens)", inp)
        return real["attnpool_tokens"](inp, pos, out, B, HW, backward)

    def conv3x3(x, *a, **k):
        R.see("conv3x3 input gradient" + (" + bnbwd" if k.get("bnbwd") is not None else ""), "x (dL/dy)", x)   # (backward phase only)
        return real["conv3x3"](x, *a, **k)

    for n, f in dict(bn_bwd=bn_bwd, col2im3x3=col2im3x3, relu_bwd=relu_bwd, avgpool2=avgpool2, attnpool_tokens=attnpool_tokens,
                     conv3x3=conv3x3).items():
        setattr(ops, n, f)
    for n, f in dict(gemm_nt=gemm_nt, attention_bwd=attention_bwd, layernorm_bwd=layernorm_bwd, embed_lnpre_bwd=embed_lnpre_bwd,
                     lora_down=lora_down, lora_grad_partial=lora_grad_partial, lora_grad_partial_ln=lora_grad_partial_ln,
                     reduce_partials=reduce_partials, head_bwd=head_bwd, ot_head_bwd=ot_head_bwd, text_tail_bwd=text_tail_bwd,
                     text_ctx_grad=text_ctx_grad, slice_bwd=slice_bwd, ce_loss=start("ce_loss"), ce_fair_loss=start("ce_fair_loss"),
                     loss_scale=start("loss_scale")).items():
        setattr(ops, n, f)
    ops.ReducePlan.run = plan_run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vit_b16", choices=["vit_b16", "vit_tiny", "rn50", "rn_tiny"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--slices", type=int, default=0, help="3D OCT front end with this many slices per volume (0: 2D images)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rn = a.model.startswith("rn")
    mcfg = getattr(C, a.model)(rank=a.rank)
    kw = {}
    if a.slices:
        import dataclasses
        mcfg = dataclasses.replace(mcfg, dim_per_3d_slice=8)
        kw = dict(slices=a.slices, signal=0.2)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    b = synth.make_batch(mcfg, a.batch, seed=1234, **kw)
    if rn:
        from fairfedmed_amd.engine_rn import create_engine
        eng = create_engine(mcfg, sd, dtype=torch.float16, max_images=a.batch)
    else:
        eng = FairLoRAEngine(mcfg, sd, dtype=torch.float16, max_images=a.batch * max(a.slices, 1))
    for tower in (getattr(eng, "vis", None), getattr(eng, "txt", None)):
        for pair in (list(getattr(tower, "sites", [])) + list(getattr(tower, "asites", []))) if tower is not None else []:
            SITES.extend(pair)
    R = Ranges()
    wrap(R)
    out = eng.forward_backward(b["img"].cuda(), b["attrs"].t()[0].contiguous().cuda(), b["label"].cuda())
    torch.cuda.synchronize()
    rows = R.table()
    print(f"# {a.model} batch {a.batch} rank {a.rank} float16, gradient scale {eng.grad_scale:g}, loss {float(out['loss']):.4f}, "
          f"finite {int(out['finite'])}")
    print("| kernel | operand | type | calls | log2 rms min | log2 rms max | log2 max | share < 2^-14 | share = 0 |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['kernel']} | {r['operand']} | {r['dtype']} | {r['calls']} | {lg2(r['rms_min'])} | {lg2(r['rms_max'])} | {lg2(r['max'])} "
              f"| {r['tiny']:.4f} | {r['zero']:.4f} |")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(model=a.model, batch=a.batch, rank=a.rank, scale=eng.grad_scale, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
