"""Sinkhorn / COT logits heads on the GPU: csrc/head_ot.hip through the engine against the
oracle and the goldens produced by the imported reference (tests/golden/ot.npz), and its kernels called directly at
full size and at their limits against the float64 restatement of tests/ot_reference.py."""
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch

from fairfedmed_amd import config as C
from fairfedmed_amd import synth

pytestmark = pytest.mark.gpu


def cos(got, ref):
    got = torch.as_tensor(got).double().cpu().flatten()
    ref = torch.as_tensor(ref).double().cpu().flatten()
    return float(torch.dot(got, ref) / (got.norm() * ref.norm()).clamp_min(1e-300))


def rel(got, ref):
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def to_dev(batch):
    return batch["img"].cuda(), batch["attrs"].t()[0].cuda(), batch["label"].cuda()


@pytest.mark.parametrize("ot,top", [("Sinkhorn", 1.0), ("COT", 0.8)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_ot_head_step_vs_reference_golden_and_oracle(golden_dir, ot, top, dtype):
    from oracle import fairlora_oracle as O
    from fairfedmed_amd.engine import FairLoRAEngine
    gold = np.load(os.path.join(golden_dir, "ot.npz"))
    meta = json.load(open(os.path.join(golden_dir, "ot.json")))
    tag = f"ot_{ot.lower()}"
    mcfg = dataclasses.replace(C.vit_tiny(rank=4), ot=ot, ot_top_percent=top)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    batch = synth.make_batch(mcfg, 8, seed=1234)
    keys = synth.trainable_keys(mcfg)
    eng = FairLoRAEngine(mcfg, sd, dtype=dtype, max_images=8)
    out = eng.forward_backward(*to_dev(batch))
    f32 = dtype == torch.float32
    assert int(out["finite"]) == 1
    assert rel(out["logits"], gold[f"{tag}.logits"]) < (2e-5 if f32 else 3e-2)
    l0 = meta[f"{tag}.loss0"]
    assert abs(float(out["loss"]) - l0) <= (1e-5 if f32 else 1e-2) * abs(l0)
    loss, logits, grads = O.loss_and_grads(sd, batch, mcfg, keys)
    for k in keys:
        g, ref = eng.params.view(k, "grad"), grads[k]
        if float(ref.abs().max()) == 0.0:
            assert float(g.abs().max()) < 1e-12, k
        elif f32:
            assert rel(g, ref) < 2e-3 and rel(g, gold[f"{tag}.grad.{k}"]) < 2e-3, (k, rel(g, ref))
        else:
            assert cos(g, ref) > 0.985, (k, cos(g, ref))
    assert rel(eng.forward(batch["img"].cuda(), batch["attrs"].t()[0].cuda()), out["logits"]) < 1e-6
    if f32:                                                            # three SGD steps on the reference's trajectory
        for i, ref in enumerate(meta[f"{tag}.traj"]):
            o = out if i == 0 else eng.forward_backward(*to_dev(batch))
            eng.sgd_step(1e-3, 0.9, 5e-4, repeats=2)                   # shared optimizer, two names (quirk 9)
            assert abs(float(o["loss"]) - ref["loss"]) <= 1e-4 * abs(ref["loss"]), (i, float(o["loss"]), ref)


@pytest.mark.parametrize("ot", ["Sinkhorn", "COT"])
def test_ot_head_on_the_resnet_tower_and_no_early_stop(ot):
    """The heads on the RN tower's attention-pool tokens (4 tokens, 256-d), and a threshold that is never met (all
    max_iter iterations run), against the oracle."""
    from oracle import fairlora_oracle as O
    from fairfedmed_amd.engine_rn import create_engine
    import copy
    mcfg = dataclasses.replace(C.rn_tiny(rank=4, num_groups=2), ot=ot, ot_thresh=0.0, ot_max_iter=7, ot_top_percent=0.7)
    sd = synth.make_state_dict(mcfg, seed=2, lora_init="random")
    batch = synth.make_batch(mcfg, 5, seed=9)
    keys = synth.trainable_keys(mcfg)
    eng = create_engine(mcfg, sd, dtype=torch.float32, max_images=5)
    out = eng.forward_backward(*to_dev(batch))
    loss, logits, grads = O.loss_and_grads(copy.deepcopy(sd), batch, mcfg, keys)
    assert rel(out["logits"], logits) < 5e-5 and abs(float(out["loss"]) - float(loss)) <= 2e-5 * abs(float(loss))
    assert int(eng.ot_istop) == 6
    for k in keys:
        if float(grads[k].abs().max()) > 0:
            assert cos(eng.params.view(k, "grad"), grads[k]) > 1 - 1e-4, k


def test_trainer_selects_the_ot_head():
    from tests.test_trainer_gpu import make_cfg
    from fairfedmed_amd.trainer import GLP_OT_SVLoRA, SyntheticFedData
    mcfg = C.vit_tiny(rank=4)
    cfg = make_cfg(prec="fp32")
    cfg.TRAINER.GLP_OT.OT, cfg.TRAINER.GLP_OT.EPS, cfg.TRAINER.GLP_OT.THRESH = "COT", 0.1, 1e-3
    cfg.TRAINER.GLP_OT.MAX_ITER, cfg.TRAINER.GLP_OT.TOP_PERCENT = 100, 0.8
    tr = GLP_OT_SVLoRA(cfg, data=SyntheticFedData(mcfg, 1, 2, 1, 8))
    assert tr.engine.ot == "COT" and tr.engine.cfg.ot_top_percent == 0.8
    tr.num_batches, tr.batch_idx = 10, 0
    s = tr.forward_backward(synth.make_batch(mcfg, 8, seed=3))
    assert np.isfinite(s["loss"])
    cfg.TRAINER.GLP_OT.OT = "Wasserstein"
    with pytest.raises(NotImplementedError):
        GLP_OT_SVLoRA(cfg, data=SyntheticFedData(mcfg, 1, 1, 1, 8))


@pytest.mark.parametrize("ot", ["Sinkhorn", "COT"])
def test_ot_head_with_the_3d_oct_front_end(ot):
    """3D OCT: every slice group is an image of the transport problem and the logits are averaged over the slices
    afterwards (trainers/GLP_OT_SVLoRA.py:752-754); the stopping test runs over all B * S * n_cls problems."""
    from oracle import fairlora_oracle as O
    from fairfedmed_amd.engine import FairLoRAEngine
    mcfg = dataclasses.replace(C.vit_tiny_3d(rank=4, dim_per_3d_slice=4), ot=ot, ot_top_percent=0.9)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    batch = synth.make_batch(mcfg, 4, seed=21)                       # 4 volumes x 2 slice groups = 8 ViT images
    keys = synth.trainable_keys(mcfg)
    eng = FairLoRAEngine(mcfg, sd, dtype=torch.float32, max_images=8)
    out = eng.forward_backward(*to_dev(batch))
    loss, logits, grads = O.loss_and_grads(sd, batch, mcfg, keys)
    assert rel(out["logits"], logits) < 3e-5 and abs(float(out["loss"]) - float(loss)) <= 2e-5 * abs(float(loss))
    for k in keys:
        if float(grads[k].abs().max()) > 0:
            assert rel(eng.params.view(k, "grad"), grads[k]) < 3e-3, (k, rel(eng.params.view(k, "grad"), grads[k]))


# ---------------------------------------------------------------------------------------------------------------------
# Kernel level: ops.ot_head_fwd / ops.ot_head_bwd against the float64 restatement of tests/ot_reference.py, computed
# from the STORED inputs (16-bit f upcast, float32 tn and logit_scale), so that what is left is the kernels' float32
# arithmetic and the 16-bit rounding of df.
#
# Tolerances of T, logits / tsum, errs, df and dtn_part come from the reference alone: e32 is the error of the same
# restatement run in float32 on the host (same inputs, the float64 run's iteration count) against float64, and the bound
# is 8 * e32 with a floor of 2^-22 of the scale (the factor covers the kernels' wave-tree reduction order and expf ulps;
# the floor an e32 that is lucky on one input).  T and dtn_part are scaled per problem / per image (e32 is the largest
# per-group error over that group's scale); a logit's scale is exp(ls) * sum |T * sim|, the scale of its sum.
# sim and rnorm carry the analytic bounds of a D-term dot product.
# ---------------------------------------------------------------------------------------------------------------------
OT_SHAPES = [                    # (B images, L tokens, D, N prompts, n_cls)
    (8, 197, 512, 2, 2),         # ViT-B/16 as trained: M = 196, four waves, the last with 4 live lanes
    (4, 50, 1024, 2, 2),         # RN50 attention pool: D = 1024, all four chunks per lane
    (2, 257, 260, 8, 8),         # every limit at once: M = 256, N = 8, n_cls = 8; 65 chunks, only lane 0 holds two
    (3, 65, 4, 1, 3),            # M = 64: one full wave, no dead lanes; D = 4; N = 1
    (5, 66, 256, 3, 1),          # M = 65: the second wave has one live lane
    (130, 17, 128, 2, 2),        # 260 problems, more than the stop kernel's 256 threads
    (2, 2, 64, 2, 2),            # M = 1
    (1, 197, 512, 2, 1),         # one problem: COT at top_percent 1.5 checks the clamp to 1
]
OT_REPEAT = (0, 2)               # run twice with different poison values: outputs bitwise identical
# rounding of a 16-bit df: |fl(x) - x| <= u |x| with the unit roundoff u = 2^-p of a p-bit significand (bf16 p = 8,
# f16 p = 11), and <= half the subnormal spacing (2^-25) below f16's normal range (6.1e-5)
OT_U16 = {torch.float32: (0.0, 0.0), torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25)}
OT_SENT, OT_TAIL = -4242.0, 37
OT_RATIOS = {}                   # (quantity, dtype) -> worst kernel error / e32 (e32 floored at 2^-25 of the scale, so
                                 # that a pass is a ratio <= 8), printed per case


def _ot_kernel_cases():
    for si, shape in enumerate(OT_SHAPES):
        modes = [("Sinkhorn", 1.0), ("COT", 1.0), ("COT", 0.8)] + ([("COT", 1.5)] if shape[0] * shape[4] == 1 else [])
        for mode, top in modes:
            for eps in ([0.1, 0.05] if si == 0 else [0.1]):
                yield pytest.param(si, mode, top, eps, id=f"{'x'.join(map(str, shape))}-{mode}{top:g}-eps{eps:g}")


def _ot_regimes(R, fr, tnr, ls, shape, mode, eps, top):
    """thresh, max_iter and the expected istop of the stopping regimes (a)-(d), from the reference's own means.  (b)
    asserts its margin and floor conditions here, before any kernel runs."""
    B, L, D, N, n_cls = shape
    probe = R.head(fr, tnr, ls, n_cls, N, mode, eps, 0.0, 12, top)
    m = probe.means
    reg = {"a": (2.0 * m[0], 12, 0), "c": (0.0, 12, 11), "d": (1e-3, 1, 0)}
    if L - 1 >= 16 and N >= 2:
        k = 1
        thresh = math.sqrt(m[k] * m[k + 1])
        assert all(m[j] >= 1.5 * thresh for j in range(k + 1)) and m[k + 1] <= thresh / 1.5, ("margin", m[:k + 2], thresh)
        assert m[k + 1] >= 100 * 2.0 ** -23 * probe.itmax[k + 1], ("floor", m[k + 1], probe.itmax[k + 1])
        reg["b"] = (thresh, 12, k + 1)
    else:
        assert L - 1 == 1 or N == 1                      # only M = 1 / N = 1 (one-iteration convergence) leave out (b)
    return reg


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _ot_run(ops, fs, tn32, ls_t, dl, shape, mode, eps, thresh, max_iter, top, poison):
    """Both entry points on NaN- (or `poison`-) filled outputs, each followed by a tail of sentinels.  Asserts the
    tails are untouched and every element the contract defines is finite; returns the outputs on the host."""
    B, L, D, N, n_cls = shape
    P, M = B * n_cls, L - 1
    sizes = {"rnorm": B * L, "sim": P * M * N, "T": P * M * N, "errs": max_iter * P, "tsum": P, "logits": P,
             "dtn": B * n_cls * N * D, "df": B * L * D, "istop": 1}
    bufs = {}
    for k, n in sizes.items():
        dt = fs.dtype if k == "df" else torch.int32 if k == "istop" else torch.float32
        bufs[k] = torch.full((n + OT_TAIL,), OT_SENT if k != "istop" else -31337, dtype=dt, device="cuda")
        bufs[k][:n] = (poison if k != "istop" else (-7 if math.isnan(poison) else 99999))
    tails = {k: bufs[k][n:].clone() for k, n in sizes.items()}
    v = {k: bufs[k][:n] for k, n in sizes.items()}
    f2 = fs.view(B * L, D)
    ops.ot_head_fwd(f2, tn32, ls_t, v["rnorm"], v["sim"], v["T"], v["errs"], v["istop"], v["tsum"], v["logits"], B, L,
                    n_cls, N, mode, eps, thresh, max_iter, top)
    ops.ot_head_bwd(f2, tn32, ls_t, v["rnorm"], v["T"], dl, v["df"].view(B * L, D), v["dtn"], B, L, n_cls, N)
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert torch.equal(_bits(bufs[k][n:]), _bits(tails[k])), f"{k}: write past the end of the output"
        assert bool(torch.isfinite(v[k].float()).all()), f"{k}: an element of the output was not written (or not finite)"
    return {k: t.cpu() for k, t in v.items()}


def _ot_bound(name, dtype, got, ref, ref32, u=(0.0, 0.0), scale=None):
    """|got - ref| <= max(8 e32, 2^-22 scale) (+ the rounding u |ref| + h of a 16-bit output), over one tensor."""
    ref32 = ref32.double()
    e32 = float((ref32 - ref).abs().max())
    scale = float(ref.abs().max()) if scale is None else scale
    err = (got - ref).abs()
    tol = max(8.0 * e32, 2.0 ** -22 * scale)
    rnd = u[0] * ref.abs() + u[1]
    bad = err > tol + rnd
    assert not bool(bad.any()), (name, float(err.max()), tol, e32, int(bad.sum()))
    ratio = float((err - rnd).clamp_min(0).max()) / (tol / 8)
    OT_RATIOS[(name, str(dtype))] = max(OT_RATIOS.get((name, str(dtype)), 0.0), ratio)
    return ratio


def _ot_bound_groups(name, dtype, got, ref, ref32, scale):
    """The same per group (leading index): errors over the group's scale, e32 the largest such ratio of the float32 run."""
    ref32 = ref32.double()
    dims = tuple(range(1, ref.dim()))
    per = lambda x: x.abs().amax(dim=dims) if dims else x.abs()
    e32 = float((per(ref32 - ref) / scale).max())
    err = per(got - ref) / scale
    tol = max(8.0 * e32, 2.0 ** -22)
    assert bool((err <= tol).all()), (name, float(err.max()), tol, e32, int((err > tol).sum()))
    ratio = float(err.max()) / (tol / 8)
    OT_RATIOS[(name, str(dtype))] = max(OT_RATIOS.get((name, str(dtype)), 0.0), ratio)
    return ratio


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("si,mode,top,eps", list(_ot_kernel_cases()))
def test_ot_head_kernels_vs_float64_restatement(si, mode, top, eps, dtype):
    """ffm_ot_head_fwd / ffm_ot_head_bwd at full size and at the kernels' limits (OT_SHAPES), Sinkhorn and COT, in every
    storage dtype, in four stopping regimes: (a) stop at iteration 0, (b) at iteration 2, (c) never (istop = max_iter - 1
    = 11), (d) max_iter = 1.  Checked: istop exactly; rnorm and sim to the dot-product bound; errs rows 0..istop
    (leaving out rows whose change is below 100 float32 ulps of the iterate - rounding noise past convergence); T and the
    logits per problem; df (class-token rows exactly 0) and the per-image dtn partials against float64 autograd with the
    kernel's own T; no write past any output and none left unwritten; bitwise repeatability on OT_REPEAT.

    Worst measured kernel error / e32 on the MI355X (f32 / bf16 / f16; the bound is 8; docs/experiments.md E13):
    T 2.33 / 2.01 / 2.00, logits 2.66 / 3.36 / 1.80, tsum 3.33 / 2.36 / 1.74, errs 1.23 / 4.35 / 2.67, df 2.03 / 0.07 /
    0.05 (beyond the 16-bit rounding), dtn_part 2.47 / 2.56 / 2.83.

    The 16-bit df allowance is the formats' unit roundoff (OT_U16: 2^-8 bf16, 2^-11 f16, plus 2^-25 in f16's subnormal
    range).  A df that is the float32 reference correctly rounded to 16 bits exceeds a 2^-9 / 2^-12 allowance on every
    16-bit case."""
    from fairfedmed_amd import ops
    from tests import ot_reference as R
    shape = OT_SHAPES[si]
    B, L, D, N, n_cls = shape
    P, M = B * n_cls, L - 1
    f64, tn64 = R.clip_like_inputs(B, L, D, N, n_cls, seed=100 + si)
    fs = f64.to(dtype)
    tn32 = tn64.float()
    fr, tnr = fs.double(), tn32.double()                     # what the kernels read
    ls_t = torch.tensor([math.log(1 / 0.07)], dtype=torch.float32)
    ls = float(ls_t)
    dl = torch.randn(P, generator=torch.Generator().manual_seed(7 + si), dtype=torch.float64).float()
    fs_d, tn_d, ls_d, dl_d = fs.cuda(), tn32.cuda(), ls_t.cuda(), dl.cuda()
    for regime, (thresh, max_iter, expect) in _ot_regimes(R, fr, tnr, ls, shape, mode, eps, top).items():
        ref = R.head(fr, tnr, ls, n_cls, N, mode, eps, thresh, max_iter, top)
        assert ref.istop == expect, (regime, ref.istop, ref.means)
        ref32 = R.head(fs.float(), tn32, ls, n_cls, N, mode, eps, thresh, max_iter, top, iters=ref.istop + 1,
                       dtype=torch.float32)
        o = _ot_run(ops, fs_d, tn_d, ls_d, dl_d, shape, mode, eps, thresh, max_iter, top, float("nan"))
        assert int(o["istop"][0]) == ref.istop, (regime, int(o["istop"][0]), ref.istop, ref.means)
        rn = o["rnorm"].double().view(B, L)
        assert bool((rn[:, 0] == 0).all())
        assert float((rn[:, 1:] / ref.rnorm[:, 1:] - 1).abs().max()) <= (D + 8) * 2.0 ** -24
        assert float((o["sim"].double().view(P, M, N) - ref.sim).abs().max()) <= 2 * (D + 8) * 2.0 ** -24
        ratios = {}
        rows = [j for j in range(ref.istop + 1) if ref.means[j] >= 100 * 2.0 ** -23 * ref.itmax[j]]
        if rows:
            ratios["errs"] = _ot_bound("errs", dtype, o["errs"].double().view(max_iter, P)[rows], ref.errs[rows],
                                       ref32.errs[rows])
        ratios["T"] = _ot_bound_groups("T", dtype, o["T"].double().view(P, M, N), ref.T, ref32.T,
                                       ref.T.abs().amax(dim=(1, 2)))
        es = math.exp(ls)
        lscale = es * (ref.T * ref.sim).abs().sum(dim=(1, 2))
        ratios["logits"] = _ot_bound_groups("logits", dtype, o["logits"].double(), ref.logits, ref32.logits, lscale)
        ratios["tsum"] = _ot_bound_groups("tsum", dtype, o["tsum"].double(), ref.tsum, ref32.tsum, lscale / es)
        Tk = o["T"].view(P, M, N)
        df64, dtn64 = R.backward(fr, tnr, ls, Tk.double(), dl.double(), n_cls, N)
        df32, dtn32 = R.backward(fs.float(), tn32, ls, Tk, dl, n_cls, N, dtype=torch.float32)
        dfk = o["df"].double().view(B, L, D)
        assert bool((dfk[:, 0] == 0).all())
        ratios["df"] = _ot_bound("df", dtype, dfk[:, 1:], df64[:, 1:], df32[:, 1:], u=OT_U16[dtype])
        ratios["dtn_part"] = _ot_bound_groups("dtn_part", dtype, o["dtn"].double().view(B, N * n_cls, D), dtn64, dtn32,
                                              dtn64.abs().amax(dim=(1, 2)))
        print("ot-kernel", shape, mode, top, eps, str(dtype), regime, "istop", ref.istop,
              " ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
        if si in OT_REPEAT:
            o2 = _ot_run(ops, fs_d, tn_d, ls_d, dl_d, shape, mode, eps, thresh, max_iter, top, 7.25)
            for k in o:
                assert torch.equal(_bits(o[k]), _bits(o2[k])), (regime, k, "differs between two runs")


def test_ot_head_c_abi_rejects_bad_arguments():
    """FFM_EINVAL (-1) from ffm_ot_head_fwd / ffm_ot_head_bwd for every argument outside the kernels' limits, in every
    dtype (the IEEE-half twin carries its own copy of the checks); nothing is launched, so the sentinel-filled outputs
    stay untouched.  Every buffer is large enough for the largest rejected shape."""
    from fairfedmed_amd import _lib as L
    lib = L.load()
    st = L.stream_ptr()
    n = 1 << 20
    inp = {dt: torch.full((n,), 0.1, dtype=dt, device="cuda") for dt in (torch.float32, torch.bfloat16, torch.float16)}
    tn, ls = torch.full((n,), 0.1, device="cuda"), torch.zeros(4, device="cuda")
    outs = [torch.full((n,), OT_SENT, device="cuda") for _ in range(7)]
    istop = torch.full((64,), -31337, dtype=torch.int32, device="cuda")
    dfs = {dt: torch.full((n,), OT_SENT, dtype=dt, device="cuda") for dt in inp}
    ok = dict(B=1, L=5, D=8, n_cls=2, N=2)
    shapes_bad = [dict(L=258), dict(L=1), dict(D=6), dict(D=1028), dict(N=9), dict(n_cls=9), dict(B=0)]

    def fwd(dt, code=None, null=None, mode=1, eps=0.1, max_iter=4, **kw):
        a = dict(ok, **kw)
        p = [L.ptr(inp[dt]), L.ptr(tn), L.ptr(ls), L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(outs[3]),
             L.ptr(istop), L.ptr(outs[4]), L.ptr(outs[5])]
        if null is not None:
            p[null] = None
        return lib.ffm_ot_head_fwd(*p, a["B"], a["L"], a["D"], a["n_cls"], a["N"], mode, eps, 1e-3, max_iter, 1.0,
                                   L.dtype_code(dt) if code is None else code, st)

    def bwd(dt, code=None, null=None, **kw):
        a = dict(ok, **kw)
        p = [L.ptr(inp[dt]), L.ptr(tn), L.ptr(ls), L.ptr(outs[0]), L.ptr(outs[2]), L.ptr(outs[5]), L.ptr(dfs[dt]),
             L.ptr(outs[6])]
        if null is not None:
            p[null] = None
        return lib.ffm_ot_head_bwd(*p, a["B"], a["L"], a["D"], a["n_cls"], a["N"], L.dtype_code(dt) if code is None else code, st)

    # inputs (f, tn, logit_scale, rnorm and T of the backward) read nothing in a rejected call, so the backward's
    # rnorm / T / dlogits are the sentinel-filled forward outputs: they must stay untouched as well
    for dt in inp:
        for kw in shapes_bad:
            assert fwd(dt, **kw) == -1, (dt, kw)
            assert bwd(dt, **kw) == -1, (dt, kw)
        for i in range(10):
            assert fwd(dt, null=i) == -1, (dt, "fwd NULL", i)
        for i in range(8):
            assert bwd(dt, null=i) == -1, (dt, "bwd NULL", i)
        for kw in [dict(mode=0), dict(mode=3), dict(eps=0.0), dict(eps=-0.1), dict(max_iter=0), dict(max_iter=-1)]:
            assert fwd(dt, **kw) == -1, (dt, kw)
    for code in (7, -1, L.F32_X3):
        assert fwd(torch.float32, code=code) == -1 and bwd(torch.float32, code=code) == -1, code
    torch.cuda.synchronize()
    for t in outs + list(dfs.values()):
        assert bool((t == torch.full_like(t, OT_SENT)).all())
    assert bool((istop == -31337).all())
    for dt in inp:                                           # and the same arguments with every value legal do run
        assert fwd(dt) == 0 and bwd(dt) == 0, dt
    torch.cuda.synchronize()
