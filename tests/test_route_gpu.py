"""The engine launches what its route says (fairfedmed_amd.engine.Route): the no-silent-fallback check.

A change that dropped a row count back onto the unfused kernels would stay inside every numerical tolerance and move only
the step time.  Here one engine with the ViT-B/16 tower's width, heads and tokens (2 layers, the tiny text tower) runs a
training step on each side of the two smallest route boundaries (13 | 14 images: FFM_EPI_LGRAD; 27 | 28: the four
LayerNorm folds), and the launches of the recorded plan are counted by name and, for ffm_gemm_nt, by epilogue flag against
what `_stack_forward` / `_stack_backward` do with the route's fields.
"""
import dataclasses
from collections import Counter

import pytest
import torch

from fairfedmed_amd import _lib as L
from fairfedmed_amd import config as C
from fairfedmed_amd import synth
from tests.test_route_cpu import B16_TABLE, panel_override

pytestmark = pytest.mark.gpu

V_LAYERS, MAX_IMAGES = 2, 28
GEMM_FLAGS = {"lnin": L.EPI_LNIN, "lgrad": L.EPI_LGRAD, "lnb_stat": L.EPI_LNB_STAT, "lnb_apply": L.EPI_LNB_APPLY}
KERNELS = {"attn_bwd_lnstat": "ffm_attention_bwd_lnstat", "attn_bwd": "ffm_attention_bwd", "ln_fwd": "ffm_layernorm_fwd",
           "ln_bwd": "ffm_layernorm_bwd"}


def route_cfg():
    base = C.vit_b16(rank=8)
    return dataclasses.replace(base, vision=dataclasses.replace(base.vision, layers=V_LAYERS), text=C.vit_tiny().text)


def launch_counts(plan) -> dict:
    """Launches of a recorded step plan by class: the kernels of KERNELS by name, ffm_gemm_nt by the flags of its args."""
    n = Counter({k: 0 for k in list(GEMM_FLAGS) + list(KERNELS)})
    by_name = {v: k for k, v in KERNELS.items()}
    for f in plan:
        name = getattr(f, "name", None)
        if name in by_name:
            n[by_name[name]] += 1
        elif name == "ffm_gemm_nt":
            flags = f.args[0]._obj.flags                       # the GemmArgs behind the byref
            for k, bit in GEMM_FLAGS.items():
                n[k] += bool(flags & bit)
    return dict(n)


def expected_counts(rt, lv: int, lt: int) -> dict:
    """What a 2-D step (block 0 ends the dX chain: no backward fold, no attention / LayerNorm backward there) of a tower of
    `lv` FairLoRA blocks launches for route `rt`, beside a text tower of `lt` blocks and ln_post (all unfused)."""
    ln1, ln2, lg, b2, b1 = (bool(x) for x in (rt.ln1, rt.ln2, rt.lgrad, rt.ln2_bwd, rt.ln1_bwd))
    return {"lnin": lv * (ln1 + ln2),
            "lgrad": lv * lg,
            "lnb_stat": (lv - 1) * b2,
            "lnb_apply": (lv - 1) * (b2 + b1),
            "attn_bwd_lnstat": (lv - 1) * b1,
            "attn_bwd": (lv - 1) * (not b1) + lt,
            "ln_fwd": lv * ((not ln1) + (not ln2)) + 1 + 2 * lt,
            "ln_bwd": (lv - 1) * ((not b2) + (not b1)) + 1 + 2 * lt}


def make_engine():
    from fairfedmed_amd.engine import FairLoRAEngine
    mcfg = route_cfg()
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    return mcfg, FairLoRAEngine(mcfg, sd, dtype=torch.bfloat16, max_images=MAX_IMAGES, device="cuda:0")


def step_plan(eng, mcfg, images: int):
    """(the plan recorded by one training step at `images` images, its loss)"""
    batch = synth.make_batch(mcfg, images, seed=1234)
    eng.step_plans.clear()
    out = eng.forward_backward(batch["img"].cuda(), batch["attrs"].t()[0].contiguous().cuda(), batch["label"].cuda())
    torch.cuda.synchronize()
    (plan,) = eng.step_plans.values()
    return plan, float(out["loss"])


@pytest.fixture(scope="module")
def engine():
    return make_engine()


@pytest.mark.parametrize("images", [13, 14, 28])
def test_engine_launches_what_the_route_says(engine, images):
    if panel_override():
        return
    mcfg, eng = engine
    rt = eng.vis.route(images * mcfg.vision.tokens)
    assert dataclasses.astuple(rt) == B16_TABLE[images], "the route of the headline tower at this batch size"
    assert not any(dataclasses.astuple(eng.txt.route(eng.n_text * eng.txt_len))), "the text tower folds nothing"
    plan, loss = step_plan(eng, mcfg, images)
    got, want = launch_counts(plan), expected_counts(rt, V_LAYERS, mcfg.text.layers)
    print(f"images {images}: route {rt}\n  launched {got}\n  expected {want}")
    assert got == want
    assert loss == loss and abs(loss) != float("inf")
