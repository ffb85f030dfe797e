"""The fairness term of the loss on the GPU (ffm_ce_fair_loss, engine.set_fairness, TRAINER.LAMBDA_FAIRNESS /
FAIRNESS_GRAD): the kernel against float64 autograd through the un-detached term, its bit-level properties beside
ffm_ce_loss, the engines (ViT fp32 against the oracle, SVLoRA, 16-bit storage, the RN50 trunk), the captured step, the
trainer's device summary and the reference trainer's own reported losses (tests/golden/fairness_loss.json).

Bounds: 2e-5 relative on losses and 2e-5 * max|ref| on dlogits are the project's fp32 bounds (tests/test_kernels_gpu.py);
rel < 2e-3 on parameter gradients is tests/test_edge_gpu.py's for the same comparison.  Every compared input keeps
min_g |m_g - M| >= 1e-4 (asserted in float64, never skipped), so no sign of the term's gradient can flip on rounding."""
import dataclasses
import functools
import json
import os

import pytest
import torch

from fairfedmed_amd import config as C
from fairfedmed_amd import synth
from tests import fairness_ref as R

pytestmark = pytest.mark.gpu

LAM = R.LAMBDA


def rel(got, ref):
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------------- kernel -------
def run_kernel(logits_img, y, a, G, S, lam=LAM, with_grad=True, gstat=True):
    from fairfedmed_amd import ops
    nb, C_ = len(y), logits_img.shape[1]
    li = logits_img.float().contiguous().cuda()
    o = {"logits": torch.full((nb, C_), 7.0, device="cuda"), "prob": torch.full((nb, C_), 7.0, device="cuda"),
         "loss": torch.full((1,), 7.0, device="cuda"), "terms": torch.full((2,), 7.0, device="cuda"),
         "gstat": torch.full((G, 2), 7.0, device="cuda") if gstat else None,
         "dl": torch.full((nb * S, C_), 7.0, device="cuda"), "fin": torch.zeros(1, device="cuda", dtype=torch.int32)}
    ops.ce_fair_loss(li, y.cuda(), a.to(torch.int32).cuda(), o["logits"], o["prob"], o["loss"], o["terms"], o["gstat"],
                     o["dl"], o["fin"], nb, S, C_, G, lam, with_grad)
    torch.cuda.synchronize()
    return o


def run_ce(logits_img, y, S):
    from fairfedmed_amd import ops
    nb, C_ = len(y), logits_img.shape[1]
    li = logits_img.float().contiguous().cuda()
    o = {"logits": torch.zeros(nb, C_, device="cuda"), "prob": torch.zeros(nb, C_, device="cuda"),
         "loss": torch.zeros(1, device="cuda"), "dl": torch.zeros(nb * S, C_, device="cuda"),
         "fin": torch.zeros(1, device="cuda", dtype=torch.int32)}
    ops.ce_loss(li, y.cuda(), o["logits"], o["prob"], o["loss"], o["dl"], o["fin"], nb, S, C_)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("case", R.all_kernel_inputs(), ids=lambda c: c[0])
def test_kernel_matches_float64_autograd(case):
    _, logits_img, y, a, G, S = case
    nb = len(y)
    z = R.slice_mean(logits_img, nb, S)
    assert R.min_gap(z, y, a, G) >= R.MIN_GAP
    loss, cls, F, dz = R.autograd_ref(z, y, a, G, LAM)
    o = run_kernel(logits_img, y, a, G, S)
    got = {"loss": float(o["loss"]), "cls": float(o["terms"][0]), "F": float(o["terms"][1])}
    dl_ref = (dz / S)[:, None, :].expand(nb, S, dz.shape[1]).reshape(nb * S, -1)
    err = float((o["dl"].double().cpu() - dl_ref).abs().max())
    print(case[0], got, "ref", float(loss), float(cls), float(F), "dlogits max abs err", err, "of", float(dl_ref.abs().max()))
    assert int(o["fin"]) == 1
    assert abs(got["loss"] - float(loss)) <= 2e-5 * abs(float(loss))
    assert abs(got["cls"] - float(cls)) <= 2e-5 * abs(float(cls))
    assert abs(got["F"] - float(F)) <= 2e-5 * abs(float(F))
    assert err <= 2e-5 * float(dl_ref.abs().max())
    assert float(o["loss"]) == float(o["terms"][0] + LAM * o["terms"][1])       # (0.5 * F is exact: fused or not, the same sum)
    # gstat: m_g and n_g of every group, m_g = 0 where a group is absent
    present, m, _, _ = R.group_stats(z, y, a, G)
    gs = o["gstat"].double().cpu()
    assert gs[:, 1].tolist() == [float((a == g).sum()) for g in range(G)]
    assert float((gs[present, 0] - m).abs().max()) <= 2e-5
    assert all(float(gs[g, 0]) == 0.0 for g in range(G) if g not in present)


def test_without_the_gradient_it_is_ce_loss_bit_for_bit():
    for _, logits_img, y, a, G, S in R.all_kernel_inputs():
        o, ce = run_kernel(logits_img, y, a, G, S, with_grad=False, gstat=False), run_ce(logits_img, y, S)
        for k in ("logits", "prob", "dl"):
            assert torch.equal(o[k], ce[k]), k
        assert torch.equal(o["terms"][0:1], ce["loss"]) and float(o["terms"][1]) > 0 and float(o["loss"]) > float(ce["loss"])
        on = run_kernel(logits_img, y, a, G, S, with_grad=True)
        assert torch.equal(on["logits"], ce["logits"]) and torch.equal(on["prob"], ce["prob"])
        assert torch.equal(on["loss"], o["loss"]) and not torch.equal(on["dl"], ce["dl"])


@pytest.mark.parametrize("attr_value", [1, -1, 5], ids=["one_group", "all_unknown", "all_beyond_G"])
def test_no_second_group_means_no_term(attr_value):
    """One present group, or no sample inside [0, G): F == 0 exactly and the gradient is ffm_ce_loss's, grad on."""
    _, logits_img, y, _, G, S = R.all_kernel_inputs()[3]
    a = torch.full((len(y),), attr_value)
    o, ce = run_kernel(logits_img, y, a, G, S, with_grad=True), run_ce(logits_img, y, S)
    assert float(o["terms"][1]) == 0.0 and torch.equal(o["loss"], ce["loss"]) and torch.equal(o["dl"], ce["dl"])
    n = o["gstat"][:, 1].tolist()
    assert n == ([0.0, float(len(y)), 0.0] if attr_value == 1 else [0.0, 0.0, 0.0])


def test_a_sample_outside_the_groups_takes_part_in_the_cross_entropy_only():
    _, logits_img, y, a, G, S = R.all_kernel_inputs()[0]
    a = a.clone()
    a[0], a[1] = -1, G
    z = R.slice_mean(logits_img, len(y), S)
    assert R.min_gap(z, y, a, G) >= R.MIN_GAP
    loss, _, F, dz = R.autograd_ref(z, y, a, G, LAM)
    o, ce = run_kernel(logits_img, y, a, G, S), run_ce(logits_img, y, S)
    assert torch.equal(o["dl"][:2], ce["dl"][:2]) and not torch.equal(o["dl"][2:], ce["dl"][2:])
    assert abs(float(o["terms"][1]) - float(F)) <= 2e-5 * float(F) and rel(o["dl"], dz) <= 2e-5
    assert int(o["gstat"][:, 1].sum()) == len(y) - 2


def test_two_runs_are_bit_identical():
    for _, logits_img, y, a, G, S in R.all_kernel_inputs()[3:5] + R.all_kernel_inputs()[-1:]:
        r1, r2 = run_kernel(logits_img, y, a, G, S), run_kernel(logits_img, y, a, G, S)
        for k in ("logits", "prob", "loss", "terms", "gstat", "dl", "fin"):
            assert torch.equal(r1[k], r2[k]), k


def test_a_non_finite_loss_clears_the_flag():
    _, logits_img, y, a, G, S = R.all_kernel_inputs()[0]
    bad = logits_img.clone()
    bad[0, 0] = float("nan")
    assert int(run_kernel(bad, y, a, G, S)["fin"]) == 0


# ------------------------------------------------------------------------------------------------------ engines -------
BS = 8


def batch_on_gpu(batch):
    return batch["img"].cuda(), batch["attrs"].t()[0].contiguous().cuda(), batch["label"].cuda()


@functools.lru_cache(maxsize=None)
def vit_case():
    """vit_tiny(rank=4), batch 8: the first batch seed whose oracle logits keep the sign precondition, and the oracle's
    loss / gradients of CE + LAM * F with the term in the graph (computed once, shared, never modified)."""
    from oracle import fairlora_oracle as O
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    keys = synth.trainable_keys(mcfg)
    G = mcfg.lora.num_groups
    for seed in range(11, 31):
        batch = synth.make_batch(mcfg, BS, seed=seed)
        attr = batch["attrs"].t()[0]
        with torch.no_grad():
            logits = O.clip_logits(dict(sd), batch["img"], attr, mcfg)
        if R.min_gap(logits, batch["label"], attr, G) >= R.MIN_GAP:
            break
    work, leaves = dict(sd), {}
    for k in keys:
        leaves[k] = sd[k].detach().clone().requires_grad_(True)
        work[k] = leaves[k]
    logits = O.clip_logits(work, batch["img"], attr, mcfg)
    cls = torch.nn.functional.cross_entropy(logits, batch["label"])
    F = R.fair_term(logits, batch["label"], attr, G)
    (cls + LAM * F).backward()
    grads = {k: (leaves[k].grad if leaves[k].grad is not None else torch.zeros_like(leaves[k])).detach() for k in keys}
    return {"mcfg": mcfg, "sd": sd, "keys": keys, "batch": batch, "seed": seed, "logits": logits.detach(),
            "cls": float(cls.detach()), "F": float(F.detach()), "loss": float((cls + LAM * F).detach()), "grads": grads}


def host_total(prob, label, attr, G, cls):
    """cls + LAM * F from probabilities (float64 on the host): the reference's formula on what the engine returned."""
    p = prob.double().cpu()
    c = p[torch.arange(len(label)), label.cpu()]
    a = attr.cpu()
    m = torch.stack([1 - c[a == g].mean() for g in range(G) if bool((a == g).any())])
    return float(cls) + LAM * float((m - m.mean()).abs().mean())


def test_vit_engine_matches_the_oracle_with_the_term_in_the_graph():
    from fairfedmed_amd.engine import FairLoRAEngine
    vc = vit_case()
    mcfg, sd, keys, batch = vc["mcfg"], vc["sd"], vc["keys"], vc["batch"]
    attr = batch["attrs"].t()[0]
    assert R.min_gap(vc["logits"], batch["label"], attr, mcfg.lora.num_groups) >= R.MIN_GAP and vc["F"] > 0
    img, a, y = batch_on_gpu(batch)
    plain = FairLoRAEngine(mcfg, sd, dtype=torch.float32, max_images=BS)
    o0 = plain.forward_backward(img, a, y)
    assert "loss_terms" not in o0 and "group_conf" not in o0
    g0, loss0 = plain.params.grad.clone(), float(o0["loss"])
    eng = FairLoRAEngine(mcfg, sd, dtype=torch.float32, max_images=BS)
    eng.set_fairness(LAM, True)
    for rep in range(2):                                           # recorded, then replayed
        out = eng.forward_backward(img, a, y)
        print("engine", float(out["loss"]), out["loss_terms"].tolist(), "oracle", vc["loss"], vc["cls"], vc["F"])
        assert int(out["finite"]) == 1
        assert abs(float(out["loss"]) - vc["loss"]) <= 2e-5 * abs(vc["loss"])
        assert abs(float(out["loss_terms"][0]) - vc["cls"]) <= 2e-5 * abs(vc["cls"])
        assert abs(float(out["loss_terms"][1]) - vc["F"]) <= 2e-5 * abs(vc["F"])
        assert float(out["loss_terms"][0]) == loss0
        assert tuple(out["group_conf"].shape) == (mcfg.lora.num_groups, 2) and int(out["group_conf"][:, 1].sum()) == BS
        for k in keys:
            g, ref = eng.params.view(k, "grad"), vc["grads"][k]
            if float(ref.abs().max()) == 0.0:
                assert float(g.abs().max()) < 1e-12, k
            else:
                assert rel(g, ref) < 2e-3, (k, rel(g, ref))
        assert not torch.equal(eng.params.grad, g0)
    # detached (the reference): the loss moves, the gradients are those of lambda = 0 to the bit
    eng.set_fairness(LAM, False)
    assert eng.step_plans == {}
    out = eng.forward_backward(img, a, y)
    assert abs(float(out["loss"]) - vc["loss"]) <= 2e-5 * abs(vc["loss"]) and torch.equal(eng.params.grad, g0)
    # no attribute, no term
    eng.set_fairness(LAM, True)
    out = eng.forward_backward(img, None, y)
    assert "loss_terms" not in out


def test_svlora_engine_applies_the_term_too():
    """LoRA / SVLoRA adapters take no attribute (one group), the loss still does: the reference adds the term for every
    adapter type."""
    from fairfedmed_amd.engine import FairLoRAEngine
    base = C.vit_tiny(rank=4)
    mcfg = dataclasses.replace(base, lora=dataclasses.replace(base.lora, lora_type="SVLoRA", num_groups=1))
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    img, a, y = batch_on_gpu(vit_case()["batch"])
    plain = FairLoRAEngine(mcfg, sd, dtype=torch.float32, max_images=BS)
    o0 = plain.forward_backward(img, a, y)
    loss0, g0, prob0 = float(o0["loss"]), plain.params.grad.clone(), o0["prob"].clone()
    eng = FairLoRAEngine(mcfg, sd, dtype=torch.float32, max_images=BS)
    eng.set_fairness(LAM, True)
    out = eng.forward_backward(img, a, y)
    assert torch.equal(out["prob"], prob0) and float(out["loss_terms"][0]) == loss0
    want = host_total(out["prob"], y, a, 8, loss0)
    assert want > loss0 and abs(float(out["loss"]) - want) <= 2e-5 * want
    assert int(out["finite"]) == 1 and not torch.equal(eng.params.grad, g0)
    assert out["group_conf"][:, 1].tolist() == [float((a == g).sum()) for g in range(8)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_16_bit_step_with_the_term(dtype):
    from fairfedmed_amd.engine import FairLoRAEngine
    vc = vit_case()
    img, a, y = batch_on_gpu(vc["batch"])
    plain = FairLoRAEngine(vc["mcfg"], vc["sd"], dtype=dtype, max_images=BS)
    plain.forward_backward(img, a, y)
    eng = FairLoRAEngine(vc["mcfg"], vc["sd"], dtype=dtype, max_images=BS)
    eng.set_fairness(LAM, True)
    out = eng.forward_backward(img, a, y)
    eng.sgd_step(1e-2, 0.9, 5e-4, repeats=2)
    torch.cuda.synchronize()
    assert int(out["finite"]) == 1 and eng.overflow_steps() == 0
    assert bool(torch.isfinite(eng.params.grad).all()) and not torch.equal(eng.params.grad, plain.params.grad)
    want = host_total(out["prob"], y, a, vc["mcfg"].lora.num_groups, float(out["loss_terms"][0]))
    assert abs(float(out["loss"]) - want) <= 2e-5 * want


def test_rn_engine_with_the_term():
    from fairfedmed_amd.engine_rn import create_engine
    mcfg = C.rn_tiny(rank=4, num_groups=2)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    img, a, y = batch_on_gpu(synth.make_batch(mcfg, 6, seed=1234))
    plain = create_engine(mcfg, sd, dtype=torch.float32, max_images=6)
    o0 = plain.forward_backward(img, a, y)
    loss0, g0 = float(o0["loss"]), plain.params.grad.clone()
    eng = create_engine(mcfg, sd, dtype=torch.float32, max_images=6)
    eng.set_fairness(LAM, True)
    out = eng.forward_backward(img, a, y)
    assert len(torch.unique(a)) == 2 and float(out["loss_terms"][0]) == loss0
    want = host_total(out["prob"], y, a, 2, loss0)
    assert want > loss0 and abs(float(out["loss"]) - want) <= 2e-5 * want
    assert int(out["finite"]) == 1 and not torch.equal(eng.params.grad, g0)


def test_captured_step_with_the_term_equals_the_eager_steps():
    """set_fairness precedes the capture; two replays train exactly as two eager forward_backward + sgd_step do."""
    from fairfedmed_amd.engine import FairLoRAEngine
    vc = vit_case()
    mcfg, sd = vc["mcfg"], vc["sd"]
    batches = [batch_on_gpu(vc["batch"]), batch_on_gpu(synth.make_batch(mcfg, BS, seed=41, signal=0.2))]
    eager, graphed, plain = (FairLoRAEngine(mcfg, sd, dtype=torch.float32, max_images=BS) for _ in range(3))
    for e in (eager, graphed):
        e.set_fairness(LAM, True)
    step = graphed.capture_train_step(BS, 1e-2, 0.9, 5e-4, repeats=2)
    for img, a, y in batches:
        le = eager.forward_backward(img, a, y)["loss"].clone()
        eager.sgd_step(1e-2, 0.9, 5e-4, repeats=2)
        out = step.run(img, a, y)
        lg, terms = out["loss"].clone(), out["loss_terms"].clone()
        torch.cuda.synchronize()
        assert torch.equal(lg, le) and float(terms[1]) > 0 and torch.equal(terms, eager.loss_terms)
        assert torch.equal(graphed.params.flat, eager.params.flat) and torch.equal(graphed.params.momentum, eager.params.momentum)
        plain.forward_backward(img, a, y)
        plain.sgd_step(1e-2, 0.9, 5e-4, repeats=2)
    assert graphed.params.steps == eager.params.steps == 4
    assert not torch.equal(plain.params.flat, eager.params.flat)          # the term did train


# ------------------------------------------------------------------------------------------------------ trainer -------
def make_trainer(lam, sd, mcfg, grad=False, host=False):
    from tests.test_trainer_gpu import make_cfg
    from fairfedmed_amd.trainer import GLP_OT_SVLoRA, SyntheticFedData
    cfg = make_cfg(prec="fp32")
    cfg.TRAINER.LAMBDA_FAIRNESS, cfg.TRAINER.FAIRNESS_GRAD = lam, grad
    cfg.TRAIN.HOST_METRICS = host
    cfg.MODEL.STATE_DICT = sd
    tr = GLP_OT_SVLoRA(cfg, data=SyntheticFedData(mcfg, 1, 1, 1, BS))
    tr.num_batches, tr.batch_idx = 10, 0
    return tr


def test_trainer_reports_the_total_from_the_device_summary():
    from oracle import fairlora_oracle as O
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    batch = synth.make_batch(mcfg, BS, seed=11)
    keys = synth.trainable_keys(mcfg)
    ref_loss, _, _ = O.loss_and_grads(sd, batch, mcfg, keys, lambda_fairness=LAM)
    dev, host, zero = make_trainer(LAM, sd, mcfg), make_trainer(LAM, sd, mcfg, host=True), make_trainer(0.0, sd, mcfg)
    s, sh, s0 = dev.forward_backward(batch), host.forward_backward(batch), zero.forward_backward(batch)
    assert not isinstance(s, dict) and set(s) == {"loss", "acc", "auc"} and isinstance(sh, dict)
    print("trainer", s["loss"], "host checker", sh["loss"], "oracle", float(ref_loss), "lambda 0", s0["loss"])
    assert abs(s["loss"] - float(ref_loss)) <= 2e-5 * abs(float(ref_loss))
    assert abs(sh["loss"] - float(ref_loss)) <= 2e-5 * abs(float(ref_loss))      # the host checker adds the term once
    assert abs(s["acc"] - sh["acc"]) < 1e-9 and abs(s["auc"] - sh["auc"]) < 1e-12
    assert s["loss"] > s0["loss"]
    # FAIRNESS_GRAD off (the default): the reference's detached term - gradients of lambda = 0 to the bit
    assert torch.equal(dev.engine.params.grad, zero.engine.params.grad)
    assert torch.equal(host.engine.params.grad, zero.engine.params.grad)
    on = make_trainer(LAM, sd, mcfg, grad=True)
    son = on.forward_backward(batch)
    assert son["loss"] == s["loss"] and not torch.equal(on.engine.params.grad, zero.engine.params.grad)


def test_trainer_matches_the_reference_trainers_reported_losses(golden_dir):
    """tests/golden/fairness_loss.json: loss.item() of the reference's own forward_backward (make_golden_fairness.py)."""
    gold = json.load(open(os.path.join(golden_dir, "fairness_loss.json")))
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=gold["state_seed"], lora_init=gold["lora_init"])
    assert {c["lambda"] for c in gold["cases"]} == {0.0, 0.5} and len({c["batch_seed"] for c in gold["cases"]}) == 2
    for c in gold["cases"]:
        assert c["batch_size"] == BS
        tr = make_trainer(c["lambda"], sd, mcfg)
        s = tr.forward_backward(synth.make_batch(mcfg, BS, seed=c["batch_seed"]))
        print(c, "->", s["loss"])
        assert abs(s["loss"] - c["loss"]) <= 2e-5 * abs(c["loss"]), (c, s["loss"])
        assert abs(s["acc"] - c["acc"]) < 1e-3 and abs(s["auc"] - c["auc"]) < 1e-9
