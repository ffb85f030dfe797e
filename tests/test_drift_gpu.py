"""Client-drift correction on the GPU (csrc/drift.hip, ffm_drift_correct): the kernel bit for bit
against the host twin of fairfedmed_amd/drift.py (which tests/test_drift_cpu.py holds to the float64 formulas) inside guard
bands, the engine's call site under both storage types, the captured step, the fp16 gating, and the one-process driver."""
import pytest
import torch

from fairfedmed_amd import config as C
from fairfedmed_amd import drift as D
from fairfedmed_amd import ops
from fairfedmed_amd import synth
from tests.guarded import _POISON as POISON
from tests.guarded import guard_fixture
from tests.test_drift_cpu import _operands

pytestmark = pytest.mark.gpu

LR, MOM, WD = 1e-2, 0.9, 5e-4
MU = 0.5
SETS = {"anchor": ("anchor",), "c_diff": ("c_diff",), "gsum": ("gsum",), "all": ("anchor", "c_diff", "gsum")}


@pytest.fixture
def g():
    yield from guard_fixture()


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def same(a, b):
    return a.shape == b.shape and bool((bits(a.cpu()) == bits(b.cpu())).all())


_CPU = {}


def cpu_operands(n):
    """(g, p, anchor, c_diff, gsum) on the host, built once per size and never written."""
    if n not in _CPU:
        _CPU[n] = _operands(n, seed=1000 + n % 997)
    return _CPU[n]


def launch(gd, n, which, off, ok=None):
    """One launch on guarded copies of the operands; every float pointer `off` floats behind a 16-byte boundary (0: the
    16-byte path, 1: element by element).  Returns the device tensors and the host twin's results."""
    src = dict(zip(("g", "p", "anchor", "c_diff", "gsum"), cpu_operands(n)))

    def rw(name):                                                     # written by the kernel: between guard bands
        body = gd.out(n + off, name=name)
        t = body[off:]
        t.copy_(src[name])
        return body, t

    def ro(name):                                                     # read only: a NaN in front when it is offset
        t = torch.full((n + off,), float("nan"), device="cuda")[off:]
        t.copy_(src[name])
        return t

    bodies = {}
    bodies["g"], dev_g = rw("g")
    kw, tw = {}, {}
    if "anchor" in which:
        kw.update(p=ro("p"), anchor=ro("anchor"), mu=MU)
        tw.update(p=src["p"], anchor=src["anchor"], mu=MU)
    if "c_diff" in which:
        kw.update(c_diff=ro("c_diff"))
        tw.update(c_diff=src["c_diff"])
    dev_count = None
    if "gsum" in which:
        bodies["gsum"], dev_s = rw("gsum")
        dev_count = gd.out(1, dtype=torch.int64, name="count")
        dev_count.fill_(6)
        kw.update(gsum=dev_s, count=dev_count)
        tw.update(gsum=src["gsum"].clone(), count=torch.tensor([6], dtype=torch.int64))
    st = None
    if ok is not None:
        st = torch.tensor([4096.0, 1 / 4096.0, ok, 0.0, 0.0, 4096.0, 2000.0, 1.0], device="cuda")
        tw.update(scale_state=st.cpu())
    for name, t in list(kw.items()):
        if isinstance(t, torch.Tensor) and t.dtype == torch.float32:
            assert t.data_ptr() % 16 == 4 * off, name
    assert dev_g.data_ptr() % 16 == 4 * off
    ops.drift_correct(dev_g, scale_state=st, **kw)
    twin_g = src["g"].clone()
    D.host_correct(twin_g, **tw)
    for name, body in bodies.items():
        gd.check(defined=slice(off, None), of=body)
        if off:                                                       # the float in front of an offset pointer keeps its poison
            assert int(body[:1].view(torch.int32)) == POISON[torch.float32], name
    if dev_count is not None:
        gd.check(of=dev_count)
    return dev_g, kw, twin_g, tw


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset_one_float"])
@pytest.mark.parametrize("which", list(SETS), ids=list(SETS))
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1021, 4096, 2_097_157])
def test_kernel_equals_the_host_twin(g, n, which, off):
    """n = 2 097 157: five elements past the grid cap of 2048 blocks x 256 threads x 4 floats, so the stride loop runs and its
    last group is a ragged one."""
    dev_g, kw, twin_g, tw = launch(g, n, SETS[which], off)
    assert same(dev_g, twin_g), "g"
    if "gsum" in SETS[which]:
        assert same(kw["gsum"], tw["gsum"]), "gsum"
        assert int(kw["count"]) == int(tw["count"]) == 7
    if which == "gsum":
        assert same(dev_g, cpu_operands(n)[0])                        # the gradient keeps its bits
    for name in ("p", "anchor", "c_diff"):
        if name in kw:
            assert same(kw[name], tw[name]), f"{name} is an input"


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset_one_float"])
@pytest.mark.parametrize("n", [5, 4096])
def test_an_overflowed_step_changes_nothing(g, n, off):
    src = cpu_operands(n)
    dev_g, kw, twin_g, tw = launch(g, n, SETS["all"], off, ok=0.0)
    assert same(dev_g, src[0]) and same(kw["gsum"], src[4]) and int(kw["count"]) == 6
    assert same(twin_g, src[0]) and int(tw["count"]) == 6
    dev_g, kw, twin_g, tw = launch(g, n, SETS["all"], off, ok=1.0)    # the same launch on a good step does move them
    assert same(dev_g, twin_g) and same(kw["gsum"], tw["gsum"]) and int(kw["count"]) == 7
    assert not same(dev_g, src[0])


def test_wrapper_refuses_host_tensors_and_bad_operand_sets():
    x = torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.drift_correct(torch.zeros(8), c_diff=torch.zeros(8))
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.drift_correct(x)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.drift_correct(x, c_diff=x.clone(), gsum=x.clone())
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.drift_correct(x, c_diff=x.clone(), mu=0.5)


# ---------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------
def to_dev(batch):
    return batch["img"].cuda(), batch["attrs"].t()[0].contiguous().cuda(), batch["label"].cuda()


def engines(dtype, n=2, bs=4):
    from fairfedmed_amd.engine import FairLoRAEngine
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    return mcfg, [FairLoRAEngine(mcfg, sd, dtype=dtype, max_images=bs) for _ in range(n)]


def corrector(eng, mode, seed=3):
    """A corrector in the middle of a client-round: a control variate / an anchor that is not trivial."""
    corr = D.DriftCorrector(eng.params.flat, 2, D.DriftCfg(mode, MU if mode == "fedprox" else 0.0))
    gen = torch.Generator().manual_seed(seed)
    n = eng.params.flat.numel()
    if mode == "scaffold":
        corr.c.copy_(torch.randn(n, generator=gen) * 1e-2)
        corr.c_i[1].copy_(torch.randn(n, generator=gen) * 1e-2)
    corr.begin_client(1)
    if mode == "fedprox":
        corr.anchor.add_((torch.randn(n, generator=gen) * 1e-2).cuda())
    return corr


@pytest.mark.parametrize("mode", ["fedprox", "scaffold"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_applies_the_correction_behind_the_backward_pass(dtype, mode):
    mcfg, (plain, eng) = engines(dtype)
    corr = corrector(eng, mode)
    eng.set_drift(corr)
    for i in range(2):                                                # the recording call and a replayed one
        batch = to_dev(synth.make_batch(mcfg, 4, seed=40 + i, signal=0.2))
        before = {k: getattr(corr, k).cpu().clone() for k in ("anchor", "c_diff", "gsum", "count")}
        plain.forward_backward(*batch)
        out = eng.forward_backward(*batch)
        torch.cuda.synchronize()
        want = plain.params.grad.cpu().clone()
        assert bool(want.any())
        if mode == "fedprox":
            D.host_correct(want, p=eng.params.flat.cpu(), anchor=before["anchor"], mu=MU)
        else:
            D.host_correct(want, c_diff=before["c_diff"], gsum=before["gsum"], count=before["count"])
            assert same(corr.gsum, before["gsum"]) and int(corr.count) == i + 1 == int(before["count"])
        assert same(eng.params.grad, want), f"call {i}"
        assert not same(eng.params.grad, plain.params.grad)
        assert same(out["loss"], plain.loss)                          # the reported loss stays the task loss
        assert len(eng.step_plans) == len(plain.step_plans) == 1      # the launch is not part of the recorded plan


@pytest.mark.parametrize("mode", ["fedprox", "scaffold"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_correction_of_zero_leaves_the_gradients(dtype, mode):
    """anchor == flat (the first step of a client-round) and c_diff == 0 (round 0): the gradients equal the uncorrected ones."""
    mcfg, (plain, eng) = engines(dtype)
    corr = D.DriftCorrector(eng.params.flat, 2, D.DriftCfg(mode, MU if mode == "fedprox" else 0.0))
    corr.begin_client(0)
    eng.set_drift(corr)
    batch = to_dev(synth.make_batch(mcfg, 4, seed=40, signal=0.2))
    plain.forward_backward(*batch)
    eng.forward_backward(*batch)
    torch.cuda.synchronize()
    assert torch.equal(eng.params.grad, plain.params.grad) and bool(plain.params.grad.any())
    if mode == "scaffold":
        assert torch.equal(corr.gsum, plain.params.grad) and int(corr.count) == 1
    eng.set_drift(None)
    eng.forward_backward(*batch)
    assert same(eng.params.grad, plain.params.grad)


CAPTURED = [("scaffold", torch.bfloat16, None), ("fedprox", torch.bfloat16, None), ("scaffold", torch.float32, "adam")]


@pytest.mark.parametrize("mode,dtype,opt", CAPTURED, ids=[f"{m}-{str(d).split('.')[-1]}-{o or 'sgd'}" for m, d, o in CAPTURED])
def test_captured_step_contains_the_launch(mode, dtype, opt):
    """Three replays of a step captured after set_drift against three eager forward_backward + optimizer steps."""
    from fairfedmed_amd import optim as O
    spec = O.OptimSpec(kind=opt, weight_decay=WD) if opt else None
    mcfg, (eager, graphed) = engines(dtype)
    ce, cg = corrector(eager, mode), corrector(graphed, mode)
    eager.set_drift(ce)
    graphed.set_drift(cg)
    step = graphed.capture_train_step(4, LR, MOM, WD, repeats=2, optimizer=spec)
    torch.cuda.synchronize()
    assert int(cg.count) == 0 and not bool(cg.gsum.any()), "the capture's warm-up runs left a trace in the running sum"
    for i in range(3):
        batch = to_dev(synth.make_batch(mcfg, 4, seed=50 + i, signal=0.2))
        eager.forward_backward(*batch)
        if spec is None:
            eager.sgd_step(LR, MOM, WD, repeats=2)
        else:
            eager.optim_step(spec, LR, repeats=2)
        step.run(*batch)
        torch.cuda.synchronize()
        assert torch.equal(graphed.params.flat, eager.params.flat), f"step {i}"
        assert torch.equal(cg.gsum, ce.gsum), f"step {i}"
    if mode == "scaffold":
        assert int(cg.count) == 3 == int(ce.count) and bool(cg.gsum.any())
    plain = engines(dtype, n=1)[1][0]                                 # and the correction did enter the trajectory
    for i in range(3):
        plain.forward_backward(*to_dev(synth.make_batch(mcfg, 4, seed=50 + i, signal=0.2)))
        plain.sgd_step(LR, MOM, WD, repeats=2) if spec is None else plain.optim_step(spec, LR, repeats=2)
    assert not torch.equal(plain.params.flat, eager.params.flat)


def test_fp16_overflowed_step_stays_out_of_the_running_sum():
    """grad_scale 2^30 (the method of tests/test_graph_step_gpu.py): the backward pass overflows, unscale_check clears ok, and
    the launch behind it leaves gsum and count as they were; the first good step is counted."""
    mcfg, (eng,) = engines(torch.float16, n=1)
    corr = corrector(eng, "scaffold")
    corr.gsum.copy_(torch.randn(corr.gsum.numel(), generator=torch.Generator().manual_seed(9)))
    eng.set_drift(corr)
    eng.grad_scale = 2.0 ** 30
    batch = to_dev(synth.make_batch(mcfg, 4, seed=1234))
    skipped = good = 0
    for i in range(40):
        s0, k0 = corr.gsum.clone(), int(corr.count)
        eng.forward_backward(*batch)
        ok = float(eng.scale_state[2])
        eng.sgd_step(LR, MOM, WD, repeats=2)
        if ok == 0.0:
            skipped += 1
            assert same(corr.gsum, s0) and int(corr.count) == k0 == 0, f"step {i}"
        else:
            good += 1
            assert not same(corr.gsum, s0) and int(corr.count) == k0 + 1
            assert bool(torch.isfinite(corr.gsum).all())
            break
    assert skipped > 0 and good == 1, (skipped, good)
    assert eng.overflow_steps() == skipped


# ---------------------------------------------------------------------------------------------------------------------
# the one-process driver
# ---------------------------------------------------------------------------------------------------------------------
def fed_trainer():
    from fairfedmed_amd.registry import build_trainer
    from fairfedmed_amd.trainer import SyntheticFedData
    from tests.test_trainer_gpu import make_cfg
    mcfg = C.vit_tiny(rank=4)
    cfg = make_cfg(bs=4)
    cfg.DATASET.USERS = 2
    cfg.TEST.NO_TEST = True
    cfg.TRAIN.METRICS_EVERY = 0
    cfg.DATA = SyntheticFedData(mcfg, 2, 2, 1, 4, signal=0.3)
    cfg.MODEL.STATE_DICT = synth.make_state_dict(mcfg, seed=1, lora_init="reference")
    return mcfg, build_trainer(cfg)


def launches(eng, batch):
    """Library launches of one forward_backward, the plan's included (counted with the replay off)."""
    replay, eng.use_replay = eng.use_replay, False
    seen = []
    try:
        with ops.record(seen):
            eng.forward_backward(*batch)
    finally:
        eng.use_replay = replay
    return len(seen)


def test_driver_runs_scaffold_and_switches_it_off_again():
    from fairfedmed_amd import federated as F
    runs = {}
    for mode, rounds in (("none", 1), ("scaffold", 1), ("none", 2), ("scaffold", 2)):
        mcfg, tr = fed_trainer()
        batch = to_dev(synth.make_batch(mcfg, 4, seed=7, signal=0.2))
        n0 = launches(tr.engine, batch)
        hist = F.run_fedotplora(tr, F.FedArgs(num_users=2, frac=1.0, round=rounds, seed=0, drift=mode), log=lambda *_: None)
        assert tr.engine._drift is None and launches(tr.engine, batch) == n0, "set_drift(None) restores the launch count"
        runs[mode, rounds] = hist
        if mode == "scaffold" and rounds == 2:
            corr = D.DriftCorrector(tr.engine.params.flat, 2, D.DriftCfg("scaffold"))
            tr.engine.set_drift(corr)
            assert launches(tr.engine, batch) == n0 + 1
            tr.engine.set_drift(None)
    flat = lambda h: torch.cat([v.reshape(-1).cpu() for _, v in sorted(h["global_weights"].items())])
    # round 0: every control variate is zero, the kernel adds +0.0
    assert torch.equal(flat(runs["scaffold", 1]), flat(runs["none", 1]))
    assert not torch.equal(flat(runs["scaffold", 2]), flat(runs["none", 2]))
    assert "drift" not in runs["none", 2]
    d = runs["scaffold", 2]["drift"]
    assert len(d) == 2 and all(info["steps"] == {0: 2, 1: 2} for info in d) and d[0]["c_norm"] > 0
