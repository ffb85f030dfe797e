"""The captured training step (FairLoRAEngine.capture_train_step -> GraphedStep) against the eager step it replaces.

Both run the same kernels in the same order (forward_backward's launches, then the SGD update: ffm_sgd_momentum_n /
ffm_sgd_momentum_gated eagerly, ffm_sgd_momentum_dev under the graph, one shared update function), so the standard is the
one of tests/test_engine_gpu.py::test_training_is_bit_reproducible_across_engines_and_streams: loss, weights, momentum,
step count and (fp16) the gradient-scale state BIT-identical after every step.  Capturing leaves no trace on the engine,
and an overflowed fp16 backward pass under the graph is skipped and halves the scale exactly as the eager step does.
"""
import pytest
import torch

from fairfedmed_amd import config as C
from fairfedmed_amd import synth

pytestmark = pytest.mark.gpu

LR, MU, WD = 1e-2, 0.9, 5e-4


def to_dev(batch):
    return batch["img"].cuda(), batch["attrs"].t()[0].contiguous().cuda(), batch["label"].cuda()


def engines(mcfg, sd, dtype, bs, n=2):
    from fairfedmed_amd.engine import FairLoRAEngine
    return [FairLoRAEngine(mcfg, sd, dtype=dtype, max_images=bs) for _ in range(n)]


def state_of(eng):
    p = eng.params
    out = {"flat": p.flat.clone(), "momentum": p.momentum.clone(), "grad": p.grad.clone(), "finite": eng.finite.clone(),
           "steps": p.steps}
    if eng.scale_state is not None:
        out["scale_state"] = eng.scale_state.clone()
    return out


def same(a, b):
    """Bit-identical (a NaN compares equal to itself: weights are checked for finiteness separately)."""
    if isinstance(a, int):
        return a == b
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


PARITY = [("tiny", torch.float32, 1), ("tiny", torch.float32, 2), ("tiny", torch.bfloat16, 1), ("tiny", torch.bfloat16, 2),
          ("tiny", torch.float16, 1), ("tiny", torch.float16, 2),
          ("vitb16_r8_bs32", torch.bfloat16, 2)]           # bench.py's c2, the only config it captures


@pytest.mark.parametrize("model,dtype,repeats", PARITY,
                         ids=[f"{m}-{str(d).split('.')[-1]}-x{r}" for m, d, r in PARITY])
def test_graphed_step_trains_bit_identically_to_the_eager_step(model, dtype, repeats):
    mcfg, bs = (C.vit_tiny(rank=4), 8) if model == "tiny" else (C.vit_b16(rank=8), 32)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    batches = [to_dev(synth.make_batch(mcfg, bs, seed=40 + i, signal=0.2)) for i in range(4)]
    eager, graphed = engines(mcfg, sd, dtype, bs)
    step = graphed.capture_train_step(bs, LR, MU, WD, repeats=repeats)
    lr = LR
    for i, (img, attr, label) in enumerate(batches):
        if i == 2:                                 # the LR schedule moves between replays
            lr = LR / 4
            step.set_lr(lr)
        loss_e = eager.forward_backward(img, attr, label)["loss"].clone()
        eager.sgd_step(lr, MU, WD, repeats=repeats)
        loss_g = step.run(img, attr, label)["loss"].clone()
        torch.cuda.synchronize()
        assert same(loss_g, loss_e), (i, float(loss_g), float(loss_e))
        a, b = state_of(graphed), state_of(eager)
        for k in ("flat", "momentum", "steps") + (("scale_state",) if dtype == torch.float16 else ()):
            assert same(a[k], b[k]), f"step {i}: {k} of the graphed engine differs from the eager one"
        assert bool(torch.isfinite(a["flat"]).all())
    assert graphed.params.steps == 4 * repeats


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("fresh", [True, False], ids=["fresh", "after_a_step"])
def test_capture_leaves_no_trace(dtype, fresh):
    """The warm-up bodies of capture train for real (and in fp16 at an absurd scale they overflow and move the scale):
    weights, momentum, gradients, loss flag, scale state and step count are bitwise what they were before capture."""
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=2, lora_init="random")
    (eng,) = engines(mcfg, sd, dtype, 8, n=1)
    if not fresh:
        eng.forward_backward(*to_dev(synth.make_batch(mcfg, 8, seed=3, signal=0.2)))
        eng.sgd_step(LR, MU, WD, repeats=2)
    if dtype == torch.float16:
        eng.grad_scale = 2.0 ** 30
    torch.cuda.synchronize()
    before = state_of(eng)
    eng.capture_train_step(8, LR, MU, WD, repeats=2)
    torch.cuda.synchronize()
    after = state_of(eng)
    assert before.keys() == after.keys()
    for k in before:
        assert same(after[k], before[k]), f"capture changed {k}"


@pytest.mark.parametrize("repeats,when", [(1, "before"), (2, "before"), (2, "after")],
                         ids=["x1", "x2", "x2-scale_set_after_capture"])
def test_fp16_overflow_under_the_graph_is_skipped_and_halves_the_scale(repeats, when):
    """tests/test_edge_gpu.py::test_fp16_overflow_recovers_by_halving_the_device_resident_scale with a graphed engine beside
    an eager one, both at grad_scale 2^30: every overflowed step leaves weights and momentum bitwise unchanged and halves
    the scale, overflow_steps() counts them, the weights stay finite, and the two trajectories are bit-identical through
    the recovery and two good steps past it.  `after`: the scale is set once the graph exists - the setter writes the device
    tensor the graph reads."""
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    img, attr, label = to_dev(synth.make_batch(mcfg, 8, seed=1234))
    eager, graphed = engines(mcfg, sd, torch.float16, 8)
    eager.grad_scale = 2.0 ** 30
    if when == "before":
        graphed.grad_scale = 2.0 ** 30
    step = graphed.capture_train_step(8, LR, MU, WD, repeats=repeats)
    if when == "after":
        graphed.grad_scale = 2.0 ** 30
    skipped, good = 0, 0
    for i in range(40):
        prev = state_of(graphed)
        eager.forward_backward(img, attr, label)
        eager.sgd_step(LR, MU, WD, repeats=repeats)
        out = step.run(img, attr, label)
        torch.cuda.synchronize()
        now = state_of(graphed)
        assert bool(torch.isfinite(now["flat"]).all()), f"step {i}: non-finite weights under the graph"
        assert int(out["finite"]) == 1, "the loss itself is finite: only the gradient overflowed"
        ref = state_of(eager)
        for k in ("flat", "momentum", "steps", "scale_state"):
            assert same(now[k], ref[k]), f"step {i}: {k} of the graphed engine differs from the eager one"
        if float(now["scale_state"][2]) == 0.0:       # this step overflowed (after the recovery too: the scale sits at the edge)
            skipped += 1
            assert same(now["flat"], prev["flat"]) and same(now["momentum"], prev["momentum"]), "the overflowed step moved"
            assert float(now["scale_state"][0]) == float(prev["scale_state"][0]) / 2
            assert graphed.overflow_steps() == skipped
        else:
            assert not same(now["flat"], prev["flat"])
            good += 1
            if good == 3:                          # the recovery step and two good steps past it
                break
    assert 0 < skipped < 40 and good == 3, (skipped, good)
    assert graphed.grad_scale == 2.0 ** (30 - skipped) == eager.grad_scale
    assert graphed.params.steps == (skipped + good) * repeats
