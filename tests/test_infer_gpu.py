"""The forward-only evaluation path on the GPU: the FFM_EPI_GELU_ONLY epilogue, FairLoRAEngine.infer / inference,
CustomCLIP.infer and GLP_OT_SVLoRA.test().

The standard throughout is BIT equality with the training forward: infer() runs the same products in the same order on the
same tiles and differs only in what it stores (same accumulator, same rounding, same function), so torch.equal is the right
bound and a mismatch is a finding (a wrong wait count in the new epilogue would show here), not noise.  One case is pinned
to the oracle as well, with the tolerances of tests/test_engine_gpu.py, so that the new path does not hang on forward().
"""
import dataclasses
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from fairfedmed_amd import _lib as E
from fairfedmed_amd import config as C
from fairfedmed_amd import synth

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
LR, MU, WD = 1e-2, 0.9, 5e-4


def to_dev(batch):
    return batch["img"].cuda(), batch["attrs"].t()[0].contiguous().cuda(), batch["label"].cuda()


def rel(got, ref):
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def vit_images(mcfg, bs, slices=2):
    return bs * slices if mcfg.dim_per_3d_slice else bs


def make_engine(mcfg, sd, dtype, max_images, **kw):
    from fairfedmed_amd.engine import FairLoRAEngine
    return FairLoRAEngine(mcfg, sd, dtype=dtype, max_images=max_images, **kw)


# ------------------------------------------------------------------------------------------------ kernel --
SENTINEL = 1024.0                      # (exact in every storage type)


def _gelu_pair(monkeypatch, a, w, **kw):
    """(c2 of the two-output call, out of the GELU_ONLY call, the sentinel buffer whose address rode in c2's place)."""
    from fairfedmed_amd import ops
    M, N = a.shape[0], w.shape[0]
    pre = torch.full((M, N), float("nan"), device="cuda", dtype=a.dtype)
    act = torch.full((M, N), float("nan"), device="cuda", dtype=a.dtype)
    ops.gemm_nt(a, w, pre, gelu_out=act, **kw)
    only = torch.full((M, N), float("nan"), device="cuda", dtype=a.dtype)
    sent = torch.full((M, N), SENTINEL, device="cuda", dtype=a.dtype)
    orig = E.GemmArgs

    def with_c2(*fields):
        g = orig(*fields)
        assert g.flags & E.EPI_GELU_ONLY and not g.c2
        g.c2 = sent.data_ptr()                     # a live buffer where c2 would go: it must come back untouched
        return g
    monkeypatch.setattr(E, "GemmArgs", with_c2)
    ops.gemm_nt(a, w, only, gelu_only=True, **kw)
    monkeypatch.setattr(E, "GemmArgs", orig)
    torch.cuda.synchronize()
    return act, only, sent


def _check_pair(act, only, sent):
    assert bool(torch.isfinite(act.float()).all())
    assert torch.equal(only, act)
    assert bool((sent == SENTINEL).all())


@pytest.mark.parametrize("lnin", [False, True], ids=["plain", "lnin"])
@pytest.mark.parametrize("M", [6304, 19700], ids=["bs32", "bs100"])
@DTYPES
def test_gelu_only_equals_c2_at_the_c_fc_shapes(monkeypatch, dtype, M, lnin):
    """c_fc of ViT-B/16 (N 3072, K 768, rank 8, RANKOP) at 32 and at 100 images.  16-bit: frozen weight packed - the panel
    kernel's FairLoRA tiles, with and without ln_2 folded in.  float32 has no packed weights and no LayerNorm fold
    (FFM_EPI_LNIN is FFM_EUNSUP there, with or without the new bit): its `lnin` case runs the same product unfolded, on the
    128x128 kernel like the plain one."""
    from fairfedmed_amd import ops
    N, K, r, G, rps = 3072, 768, 8, 3, 197
    h16 = dtype != torch.float32
    g = torch.Generator(device="cuda").manual_seed(11)
    x = (0.5 + torch.randn(M, K, device="cuda", generator=g)).to(dtype)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(dtype)
    bias = torch.randn(N, device="cuda", generator=g)
    rk = torch.zeros(16, K, device="cuda", dtype=dtype)
    rk[:r] = (torch.randn(r, K, device="cuda", generator=g) * K ** -0.5).to(dtype)
    S = 1 + 0.3 * torch.randn(G, r, device="cuda", generator=g)
    lw = torch.randn(r, N, device="cuda", generator=g) * 0.1
    attr = torch.randint(0, G, (M // rps,), device="cuda", generator=g).int()
    ro = ops.RankOp(rk, S, attr, rps, 0.25, 0.7)
    kw = dict(bias=bias, lw=lw, rankop=ro, b_packed=ops.pack_b(w) if h16 else None)
    if lnin and h16:
        xf = x.float()
        part = torch.stack([xf.sum(1), (xf * xf).sum(1)], 1)[None].contiguous()
        kw["ln_in"] = ops.LnIn(part, 1, w.float().sum(1).contiguous(), None, None,
                               rk=0.1 * torch.randn(32, device="cuda", generator=g))
    fl = E.EPI_BIAS | E.EPI_LORA | E.EPI_GELU | E.EPI_RANKOP | (E.EPI_LNIN if "ln_in" in kw else 0)
    assert (ops.gemm_tile_shape(M, N, K, fl, r, dtype, h16)[0] >= 0) == h16          # panel kernel / 128x128 kernel
    _check_pair(*_gelu_pair(monkeypatch, x, w, **kw))


@pytest.mark.parametrize("lora", ["none", "ts", "rankop"])
@DTYPES
def test_gelu_only_equals_c2_on_ragged_128x128_tiles(monkeypatch, dtype, lora):
    """A small shape whose M and N are not multiples of the tile, on the 128x128 kernel: BIAS | GELU, BIAS | LORA | GELU
    with the rank vectors given (ts) and formed in-kernel (RANKOP) - its three FFM_EPI_GELU instantiations."""
    from fairfedmed_amd import ops
    M, N, K, r, G, rps = 300, 200, 192, 4, 3, 50
    g = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn(M, K, device="cuda", generator=g).to(dtype)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(dtype)
    kw = dict(bias=torch.randn(N, device="cuda", generator=g))
    if lora != "none":
        kw["lw"] = torch.randn(r, N, device="cuda", generator=g) * 0.1
    if lora == "ts":
        kw["ts"] = torch.randn(M, r, device="cuda", generator=g)
    if lora == "rankop":
        rk = torch.zeros(16, K, device="cuda", dtype=dtype)
        rk[:r] = (torch.randn(r, K, device="cuda", generator=g) * K ** -0.5).to(dtype)
        S = 1 + 0.3 * torch.randn(G, r, device="cuda", generator=g)
        attr = torch.randint(0, G, (M // rps,), device="cuda", generator=g).int()
        kw["rankop"] = ops.RankOp(rk, S, attr, rps, 0.25, 0.7)
    _check_pair(*_gelu_pair(monkeypatch, x, w, **kw))


def test_ops_refuse_a_second_output_with_gelu_only():
    from fairfedmed_amd import ops
    a = torch.zeros(128, 128, device="cuda")
    with pytest.raises(AssertionError):
        ops.gemm_nt(a, a, torch.empty_like(a), bias=torch.zeros(128, device="cuda"), gelu_out=torch.empty_like(a),
                    gelu_only=True)


def test_attention_fwd_without_lse():
    from fairfedmed_amd import ops
    B, Lt, heads = 3, 50, 2
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        g = torch.Generator(device="cuda").manual_seed(13)
        qkv = torch.randn(B * Lt, 3 * heads * 64, device="cuda", generator=g).to(dtype)
        o1, o2 = torch.empty(B * Lt, heads * 64, device="cuda", dtype=dtype), torch.empty(B * Lt, heads * 64, device="cuda", dtype=dtype)
        ops.attention_fwd(qkv, o1, torch.empty(B * heads * Lt, device="cuda"), B, Lt, heads)
        ops.attention_fwd(qkv, o2, None, B, Lt, heads)
        assert torch.equal(o1, o2)


# ------------------------------------------------------------------------------------------------ engine --
TINY = [
    ("tiny_r4", C.vit_tiny(rank=4), 8, "random"),
    ("tiny_r8g2", C.vit_tiny(rank=8, num_groups=2), 6, "random"),
    ("tiny_refinit", C.vit_tiny(rank=4), 8, "reference"),
    ("tiny3d_r4", C.vit_tiny_3d(rank=4, dim_per_3d_slice=4), 6, "random"),
    ("tiny_globals", C.vit_tiny_lora("FairLoRA", True), 8, "random"),
    ("tiny_svlora", C.vit_tiny_lora("SVLoRA", False), 8, "random"),
    ("tiny_svlora_globals", C.vit_tiny_lora("SVLoRA", True), 8, "random"),
    ("tiny_lora", C.vit_tiny_lora("LoRA", False), 8, "random"),
]


def _infer_equals_forward(eng, img, attr):
    want = eng.forward(img, attr).clone()
    assert bool(torch.isfinite(want).all())
    outside = eng.infer(img, attr).clone()
    with eng.inference():
        inside = [eng.infer(img, attr).clone() for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(outside, want)
    assert torch.equal(inside[0], want) and torch.equal(inside[1], want)
    assert torch.equal(eng.forward(img, attr), want)            # ... and forward() still answers the same afterwards
    return want


@pytest.mark.parametrize("tag,mcfg,bs,init", TINY, ids=[t[0] for t in TINY])
@DTYPES
def test_infer_equals_forward_on_the_tiny_configurations(tag, mcfg, bs, init, dtype):
    sd = synth.make_state_dict(mcfg, seed=1, lora_init=init)
    img, attr, _ = to_dev(synth.make_batch(mcfg, bs, seed=1234))
    eng = make_engine(mcfg, sd, dtype, vit_images(mcfg, bs))
    _infer_equals_forward(eng, img, attr)


@pytest.mark.parametrize("ot,top", [("Sinkhorn", 1.0), ("COT", 0.8)])
@DTYPES
def test_infer_equals_forward_with_the_transport_heads(ot, top, dtype):
    mcfg = dataclasses.replace(C.vit_tiny(rank=4), ot=ot, ot_top_percent=top)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    img, attr, _ = to_dev(synth.make_batch(mcfg, 8, seed=1234))
    _infer_equals_forward(make_engine(mcfg, sd, dtype, 8), img, attr)


def test_infer_equals_forward_with_rank_above_16():
    """rank 24: the down projections are launches of their own and the workspace holds their one t / ts pair."""
    mcfg = C.vit_tiny(rank=24)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    img, attr, _ = to_dev(synth.make_batch(mcfg, 8, seed=1234))
    for dtype in (torch.float32, torch.bfloat16):
        _infer_equals_forward(make_engine(mcfg, sd, dtype, 8), img, attr)


def test_infer_equals_forward_uint8_transport():
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    img, attr, _ = to_dev(synth.make_batch(mcfg, 8, seed=1234))
    u8 = img.clamp(0, 255).round().to(torch.uint8)
    eng = make_engine(mcfg, sd, torch.bfloat16, 8)
    assert torch.equal(eng.infer(u8, attr), eng.forward(u8, attr))


def test_infer_equals_forward_vit_b16_at_100_images():
    """The evaluation batch of the reference (TEST.BATCH_SIZE 100): 19 700 token rows, the 208x384 tile at several rounds."""
    mcfg = C.vit_b16(rank=8)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    img, attr, _ = to_dev(synth.make_batch(mcfg, 100, seed=5, signal=0.2))
    eng = make_engine(mcfg, sd, torch.bfloat16, 100)
    _infer_equals_forward(eng, img, attr)


@DTYPES
def test_infer_equals_forward_full_size_3d_oct(dtype):
    mcfg = dataclasses.replace(C.vit_b16(rank=16), dim_per_3d_slice=8)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    B, S = 1, 25
    img, attr, _ = to_dev(synth.make_batch(mcfg, B, seed=3, slices=S, signal=0.2))
    eng = make_engine(mcfg, sd, dtype, B * S)
    _infer_equals_forward(eng, img, attr)


@DTYPES
def test_infer_against_the_oracle(dtype):
    """Independently of forward(): the oracle's logits, tolerances of test_tiny_step_vs_oracle_and_golden."""
    from oracle import fairlora_oracle as O
    mcfg = C.vit_tiny(rank=8, num_groups=2)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    batch = synth.make_batch(mcfg, 6, seed=1234)
    _, logits, _ = O.loss_and_grads(sd, batch, mcfg, synth.trainable_keys(mcfg))
    eng = make_engine(mcfg, sd, dtype, 6)
    img, attr, _ = to_dev(batch)
    with eng.inference():
        got = eng.infer(img, attr)
    f32, f16 = dtype == torch.float32, dtype == torch.float16
    assert rel(got, logits) < (1e-5 if f32 else 4e-3 if f16 else 2e-2)


def test_rn50_infer_is_forward():
    from fairfedmed_amd.engine_rn import create_engine
    mcfg = C.rn_tiny(rank=4, num_groups=2)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    img, attr, _ = to_dev(synth.make_batch(mcfg, 6, seed=1234))
    eng = create_engine(mcfg, sd, dtype=torch.bfloat16, max_images=6)
    assert eng.infer_ws is None                                  # no ViT workspace
    want = eng.forward(img, attr).clone()
    with eng.inference() as e:
        assert e is eng
        assert torch.equal(eng.infer(img, attr), want)
    assert torch.equal(eng.infer(img, attr), want)


# --------------------------------------------------------------------------------------------- workspace --
def test_workspace_is_sized_apart_from_the_training_stash():
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    img, attr, _ = to_dev(synth.make_batch(mcfg, 41, seed=77))
    small = make_engine(mcfg, sd, torch.bfloat16, 8, max_infer_images=40)
    big = make_engine(mcfg, sd, torch.bfloat16, 40)
    assert small.max_images == 8 and small.max_infer_images == 40 and big.max_infer_images == 40
    assert torch.equal(small.infer(img[:40], attr[:40]), big.forward(img[:40], attr[:40]))
    with pytest.raises(ValueError):
        small.forward(img[:40], attr[:40])
    with pytest.raises(ValueError):
        small.infer(img, attr)
    # ... and still trains at its own batch size, and infers small batches
    assert torch.equal(small.infer(img[:8], attr[:8]), small.forward(img[:8], attr[:8]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_workspace_bytes_do_not_depend_on_depth(dtype):
    import gc
    base = C.vit_tiny(rank=4)
    sizes, stash = [], []
    for layers in (2, 12):
        mcfg = dataclasses.replace(base, vision=dataclasses.replace(base.vision, layers=layers))
        sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
        gc.collect()                                             # engines of earlier tests hold reference cycles: free them
        torch.cuda.synchronize()                                 # before counting, not somewhere inside the constructor
        before = torch.cuda.memory_allocated()
        eng = make_engine(mcfg, sd, dtype, 8)
        stash.append(torch.cuda.memory_allocated() - before)
        sizes.append(eng.infer_ws.nbytes())
        del eng
    assert sizes[0] == sizes[1] > 0
    assert stash[1] > stash[0]                                   # (the training stash does grow: the measure is alive)


# ------------------------------------------------------------------------------------------ interference --
def _state(eng):
    p = eng.params
    out = {"flat": p.flat.clone(), "momentum": p.momentum.clone(), "grad": p.grad.clone(), "finite": eng.finite.clone()}
    if eng.scale_state is not None:
        out["scale_state"] = eng.scale_state.clone()
    return out


def _same_state(a, b):
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert a.params.steps == b.params.steps


def _fresh_forward(eng, mcfg, sd, dtype, bs, img, attr):
    """forward() of a new engine loaded with eng's current trainable tensors."""
    sd2 = dict(sd)
    sd2.update({k: v.detach().cpu().clone() for k, v in eng.trainable_state().items()})
    return make_engine(mcfg, sd2, dtype, bs).forward(img, attr).clone()


@pytest.mark.parametrize("mode", ["eager-bf16", "eager-f32", "graph-bf16", "eager-f16-scaled", "graph-f16-scaled"])
def test_infer_does_not_disturb_training(mode):
    """forward_backward(A); infer(B); sgd_step == the same without infer(B), to the bit: gradients, weights, momentum,
    (fp16) the gradient-scale state - eagerly and under the captured step.  Afterwards a NEW session sees the stepped
    parameters (rank operands and text features are not stale)."""
    how, dt = mode.split("-")[0], mode.split("-")[1]
    dtype = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}[dt]
    mcfg, bs = C.vit_tiny_lora("FairLoRA", True), 8             # GLOBAL_S: S_eff is one of the things a session prepares
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    A = to_dev(synth.make_batch(mcfg, bs, seed=40, signal=0.2))
    A2 = to_dev(synth.make_batch(mcfg, bs, seed=41, signal=0.2))
    Bi, Ba, _ = to_dev(synth.make_batch(mcfg, bs, seed=42, signal=0.2))
    plain, mixed = make_engine(mcfg, sd, dtype, bs), make_engine(mcfg, sd, dtype, bs)
    for e in (plain, mixed):
        e.enable_step_counts()
    if dtype == torch.float16:
        assert mixed.scale_state is not None and mixed.grad_scale > 1.0
    if how == "graph":
        sp, sm = plain.capture_train_step(bs, LR, MU, WD), mixed.capture_train_step(bs, LR, MU, WD)
        sp.run(*A)
        out = sm.run(*A)
        counts = out["counts"].clone()
        with mixed.inference():
            mixed.infer(Bi, Ba)
        mixed.infer(Bi, Ba)
        assert torch.equal(out["counts"], counts)
        _same_state(plain, mixed)
        sp.run(*A2)
        sm.run(*A2)                                              # the captured step still replays correctly
        _same_state(plain, mixed)
    else:
        plain.forward_backward(*A)
        out = mixed.forward_backward(*A)
        counts, loss = out["counts"].clone(), out["loss"].clone()
        mixed.infer(Bi, Ba)
        with mixed.inference():
            mixed.infer(Bi, Ba)
        assert torch.equal(out["counts"], counts) and torch.equal(out["loss"], loss)
        _same_state(plain, mixed)                                # gradients included
        plain.sgd_step(LR, MU, WD)
        mixed.sgd_step(LR, MU, WD)
        _same_state(plain, mixed)
        plain.forward_backward(*A2)                              # the recorded plan replays on an untouched stash
        mixed.forward_backward(*A2)
        _same_state(plain, mixed)
        plain.sgd_step(LR, MU, WD)
        mixed.sgd_step(LR, MU, WD)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(mixed.params.flat).all()) and not torch.equal(mixed.params.flat.cpu(),
                                                                              make_engine(mcfg, sd, dtype, bs).params.flat.cpu())
    with mixed.inference():
        got = mixed.infer(Bi, Ba).clone()
    assert torch.equal(got, _fresh_forward(mixed, mcfg, sd, dtype, bs, Bi, Ba))
    assert torch.equal(mixed.infer(Bi, Ba), got)


# ------------------------------------------------------------------------------------------------ trainer --
def _trainer_cfg(mcfg, prec, train_bs, test_bs, data, sd):
    return NS(
        SEED=1, OUTPUT_DIR="", VERBOSE=False,
        INPUT=NS(PIXEL_MEAN=list(C.CLIP_PIXEL_MEAN), PIXEL_STD=list(C.CLIP_PIXEL_STD), SIZE=(mcfg.vision.image_size,) * 2),
        DATASET=NS(NAME="FairFedMed", ATTRIBUTES=["race"], ATTRIBUTE_TYPE="race"),
        MODEL=NS(BACKBONE=NS(NAME="tiny"), GEOMETRY=mcfg, STATE_DICT=sd),
        TRAINER=NS(NAME="GLP_OT_SVLoRA", LAMBDA_FAIRNESS=0.0,
                   GLP_OT=NS(N=2, N_CTX=4, PREC=prec, OT="None"),
                   GLP_OT_LORA=NS(RANK=mcfg.lora.rank, ALPHA=2.0, TYPE="FairLoRA", GLOBAL_S=False, DISABLE_ATTR=False,
                                  UNFREEZE_IMAGE_ENCODER=True)),
        OPTIM=NS(NAME="sgd", LR=1e-3, MOMENTUM=0.9, WEIGHT_DECAY=5e-4, LR_SCHEDULER="single_step", STEPSIZE=2,
                 GAMMA=0.1, MAX_EPOCH=1),
        DATALOADER=NS(TRAIN_X=NS(BATCH_SIZE=train_bs)), TEST=NS(BATCH_SIZE=test_bs, NO_TEST=True),
        TRAIN=NS(METRICS_EVERY=1, CHECKPOINT_FREQ=0), DATA=data,
    )


def _hand_written_test(tr, idx):
    """trainer.test() as it stood before the evaluation pass: engine.forward per batch, then the same metric calls."""
    from fairfedmed_amd import ops
    from fairfedmed_amd.metrics import basic_from_counts, comprehensive_scores_from_counts
    probs, labels, attrs_all = [], [], []
    for batch in tr.fed_test_loader_x_dict[idx]:
        image, label, attrs, attr = tr.parse_batch_test(batch)
        probs.append(torch.softmax(tr.engine.forward(image, attr), -1))
        labels.append(label)
        attrs_all.append(attrs)
    prob_d, y_d = torch.cat(probs).float().contiguous(), torch.cat(labels).contiguous()
    attrs_d = torch.cat(attrs_all, dim=1)
    assert prob_d.shape[1] == 2
    tables = torch.stack([ops.eval_counts(prob_d, y_d, attrs_d[a].contiguous(), 8)
                          for a in range(attrs_d.shape[0])]).cpu().numpy()
    res = basic_from_counts(tables[0])
    last = {"accuracy": res[0], "error_rate": res[1]}
    if tables[0][-1][0] > 0 and tables[0][-1][1] > 0:
        last.update(comprehensive_scores_from_counts(tables))
    return res, last


def _equal_results(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _equal_results(a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _equal_results(x, y)
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (a, b)


@pytest.mark.parametrize("model,prec", [("tiny", "fp32"), ("tiny", "bf16"), ("tiny", "fp16"), ("vitb16", "bf16")])
def test_trainer_test_is_unchanged_and_runs_the_text_tower_once(monkeypatch, model, prec):
    from fairfedmed_amd import ops
    from fairfedmed_amd.registry import build_trainer
    from fairfedmed_amd.trainer import SyntheticFedData
    import fairfedmed_amd.trainer  # noqa: F401
    mcfg = C.vit_tiny(rank=4) if model == "tiny" else C.vit_b16(rank=8)
    data = SyntheticFedData(mcfg, num_clients=1, train_batches=1, test_batches=2, batch_size=32, test_batch_size=100,
                            signal=0.4)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    tr = build_trainer(_trainer_cfg(mcfg, prec, 32, 100, data, sd))
    assert tr.engine.max_images == 100 and len(tr.fed_test_loader_x_dict[0]) >= 2
    # a step first, so that the evaluation sees parameters that moved since the engine was built
    tr.num_batches, tr.batch_idx = 10 ** 9, 0
    tr.forward_backward(next(iter(tr.fed_train_loader_x_dict[0])))
    want_res, want_last = _hand_written_test(tr, 0)
    calls = {"text_embed": 0, "infer": 0, "forward": 0}
    for name, obj, attr in (("text_embed", ops, "text_embed"), ("infer", tr.engine, "infer"), ("forward", tr.engine, "forward")):
        orig = getattr(obj, attr)

        def counted(*a, _orig=orig, _name=name, **k):
            calls[_name] += 1
            return _orig(*a, **k)
        monkeypatch.setattr(obj, attr, counted)
    res = tr.test(idx=0)
    assert calls == {"text_embed": 1, "infer": 2, "forward": 0}
    assert len(res) == 4
    _equal_results(list(res), list(want_res))
    _equal_results(tr.last_results, want_last)
    assert "accuracy" in tr.last_results and len(tr.last_results) > 2       # the fairness block is there
