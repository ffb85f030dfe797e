"""Host side of the Adam-family optimizers and the LR-schedule set (no GPU): fairfedmed_amd/optim.py against the LR
sequences recorded from the reference's build_lr_scheduler (tests/golden/optim.json, written by
tests/golden/make_golden_optim.py), and the new C entry points' declarations, exports and argument checks.

Bound for the schedules: 1e-12 relative - both sides are a few dozen double operations; where the recorded LR is exactly
zero (CosineAnnealingLR at odd multiples of T_max) the computed LR must be exactly zero.
"""
import ctypes
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace as NS

import pytest

from fairfedmed_amd import _lib
from fairfedmed_amd import optim as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = json.load(open(os.path.join(ROOT, "tests", "golden", "optim.json")))
NEW = ("ffm_optim_step", "ffm_optim_step_dev", "ffm_optim_state_rows")
KINDS = ["sgd", "adam", "adamw", "amsgrad", "rmsprop", "radam"]


def sched_cfg(rec):
    return NS(LR=rec["lr"], LR_SCHEDULER=rec["kind"], STEPSIZE=rec["stepsize"], GAMMA=rec["gamma"], MAX_EPOCH=rec["max_epoch"],
              **rec["warmup"])


def build(rec):
    group = {"lr": rec["lr"]}
    return group, O.build_lr_schedule(group, sched_cfg(rec))


# -------------------------------------------------------------------------------------------------------- schedules ---
@pytest.mark.parametrize("key", sorted(META["sched"]))
def test_schedule_matches_the_recorded_lr_sequence(key):
    rec = META["sched"][key]
    assert len(rec["lrs"]) == META["sched_steps"] == 24 and "error" not in rec
    group, s = build(rec)
    assert group["lr"] == rec["lr0"], "LR before the first step()"
    for i, want in enumerate(rec["lrs"]):
        got = s.step()
        assert got == group["lr"] and s.last_epoch == i + 1
        if want == 0.0:
            assert got == 0.0, f"{key} step {i + 1}: {got!r}, recorded exactly 0"
        else:
            assert abs(got - want) <= 1e-12 * abs(want), f"{key} step {i + 1}: {got!r} vs recorded {want!r}"


def test_the_recorded_set_covers_every_scheduler_and_warmup():
    kinds = {r["kind"] for r in META["sched"].values()}
    assert kinds == set(O.AVAI_SCHEDS)
    warm = {(r["warmup"].get("WARMUP_TYPE"), r["warmup"].get("WARMUP_RECOUNT", True)) for r in META["sched"].values()
            if r["warmup"]["WARMUP_EPOCH"] > 0}
    assert warm == {("constant", True), ("constant", False), ("linear", True), ("linear", False)}
    assert {r["max_epoch"] for r in META["sched"].values()} == {1, 5}
    # the cosine schedule runs far past T_max and comes back up: the closed form is not what is recorded
    lrs = META["sched"]["cosine|none|1"]["lrs"]
    assert lrs[0] == 0.0 and lrs[1] == 2e-3 and lrs[2] == 0.0


@pytest.mark.parametrize("key", sorted(META["sched"]))
def test_set_lr_epoch_equals_single_steps(key):
    rec = META["sched"][key]
    g1, a = build(rec)
    g2, b = build(rec)
    for n in range(0, 24):
        b.set_lr_epoch(n)
        assert g2["lr"] == g1["lr"] and b.last_epoch == a.last_epoch == n, (key, n)
        a.step()
    b.set_lr_epoch(3)                                # backwards as well
    g3, c = build(rec)
    for _ in range(3):
        c.step()
    assert g2["lr"] == g3["lr"] and b.step() == c.step()


def test_defaults_are_sgd_single_step_without_warmup():
    """A config without NAME / LR_SCHEDULER / WARMUP_* is what the trainer has always run: StepLR's closed form."""
    o = NS(LR=1e-3, MOMENTUM=0.9, WEIGHT_DECAY=5e-4, STEPSIZE=3, GAMMA=0.1, MAX_EPOCH=2)
    spec = O.build_optim_spec(o)
    assert spec.kind == "sgd" and spec.rows == 1 and (spec.momentum, spec.weight_decay) == (0.9, 5e-4)
    group = {"lr": o.LR}
    s = O.build_lr_schedule(group, o)
    assert s.name == "single_step" and s.stepsize == 3 and s.warmup_epoch <= 0 and group["lr"] == 1e-3
    for n in range(1, 12):
        s.step()
        assert group["lr"] == 1e-3 * 0.1 ** (n // 3)          # bit for bit
    s = O.build_lr_schedule({"lr": 1e-3}, NS(LR=1e-3, STEPSIZE=(-1,), GAMMA=0.1, MAX_EPOCH=2))
    assert s.stepsize == 2                                    # stepsize <= 0 -> MAX_EPOCH (lr_scheduler.py:110-111)


def test_unknown_names_raise_the_reference_errors():
    with pytest.raises(ValueError, match=r"optim must be one of \['adam', 'amsgrad', 'sgd', 'rmsprop', 'radam', 'adamw'\], but got lion"):
        O.build_optim_spec(NS(NAME="lion"))
    with pytest.raises(ValueError, match=r"scheduler must be one of \['single_step', 'multi_step', 'cosine'\], but got exp"):
        O.build_lr_schedule({"lr": 1.0}, NS(LR_SCHEDULER="exp", MAX_EPOCH=1))
    with pytest.raises(ValueError):
        O.build_lr_schedule({"lr": 1.0}, NS(MAX_EPOCH=1, WARMUP_EPOCH=2, WARMUP_TYPE="exponential"))
    with pytest.raises(TypeError, match="stepsize must be a list"):
        O.build_lr_schedule({"lr": 1.0}, NS(LR_SCHEDULER="multi_step", STEPSIZE=3, MAX_EPOCH=1))
    O.build_lr_schedule({"lr": 1.0}, NS(MAX_EPOCH=1, WARMUP_EPOCH=-1, WARMUP_TYPE="exponential"))   # unused: not looked at


def test_spec_reads_every_key_with_the_dassl_default():
    spec = O.build_optim_spec(NS(NAME="adamw"))
    assert (spec.beta1, spec.beta2, spec.eps, spec.alpha, spec.momentum, spec.weight_decay) == (0.9, 0.999, 1e-8, 0.99, 0.9, 5e-4)
    spec = O.build_optim_spec(NS(NAME="rmsprop", ADAM_BETA1=0.8, ADAM_BETA2=0.99, RMSPROP_ALPHA=0.9, MOMENTUM=0.0, WEIGHT_DECAY=0.0))
    assert (spec.beta1, spec.beta2, spec.alpha, spec.momentum, spec.weight_decay) == (0.8, 0.99, 0.9, 0.0, 0.0)
    assert [O.OptimSpec(kind=k).rows for k in KINDS] == [1, 2, 2, 3, 2, 2]


def test_powers_are_running_products_never_pow():
    spec = O.OptimSpec(kind="adam", beta1=0.9, beta2=0.999)
    p1 = p2 = 1.0
    for t in range(0, 200):
        assert spec.powers(t) == (p1, p2), t
        p1, p2 = p1 * 0.9, p2 * 0.999
    assert spec.powers(7) == (0.9 * 0.9 * 0.9 * 0.9 * 0.9 * 0.9 * 0.9, spec.powers(7)[1])       # backwards: replayed from 1.0
    assert any(spec.powers(t)[1] != 0.999 ** t for t in range(1, 200)), "pow() and the running product never differed?"
    d = spec.desc(2e-3, 12)
    assert (d.lr, d.beta1, d.beta2, d.eps, d.step) == (2e-3, 0.9, 0.999, 1e-8, 12.0) and (d.pow1, d.pow2) == spec.powers(12)
    assert ctypes.sizeof(d) == 8 * _lib.OPTIM_DESC_WORDS


def test_optim_module_imports_and_runs_without_a_gpu():
    code = ("import sys; import fairfedmed_amd.optim as O; import torch; "
            "g = {'lr': 1.0}; s = O.LRSchedule(g, 'cosine', max_epoch=5); s.step(); "
            "d = O.OptimSpec(kind='radam').desc(1e-3, 4); "
            "assert not torch.cuda.is_initialized(); print('ok', g['lr'], d.step)")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------------ C ABI ---
def test_new_entry_points_are_declared_bound_and_exported():
    from fairfedmed_amd import build as B
    protos = {n: (rt, params) for rt, n, params in B.api_prototypes()}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in protos and name in _lib.SIGNATURES and hasattr(lib, name), name
        rt, params = protos[name]
        assert rt == "int" and len(params) == len(_lib.SIGNATURES[name]), name
    step = [t for t, _ in protos["ffm_optim_step"][1]]
    assert step == ["float*", "const float*", "float*", "int64_t", "int", "const ffm_optim_desc*", "int", "float*", "void*"]
    assert [t for t, _ in protos["ffm_optim_step_dev"][1]] == step[:5] + ["ffm_optim_desc*"] + step[6:]
    assert [a for _, a in protos["ffm_optim_step"][1]][6] == "repeats"
    # the struct is ten doubles, in the order of _lib.OptimDesc
    hdr = re.sub(r"/\*.*?\*/", "", open(B.HEADER).read(), flags=re.S)
    body = hdr[hdr.index("typedef struct ffm_optim_desc {"):hdr.index("} ffm_optim_desc;")].split("{", 1)[1]
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*double", "", decl).split(",")]
    assert fields == [n for n, _ in _lib.OptimDesc._fields_] and all(t is ctypes.c_double for _, t in _lib.OptimDesc._fields_)
    for k, code in _lib.OPTIM_KINDS.items():
        assert re.search(rf"#define FFM_OPTIM_{k.upper()} {code}\b", hdr), k
    # every prototype cites the reference lines it replaces
    raw = open(B.HEADER).read()
    for name in ("ffm_optim_step", "ffm_optim_step_dev"):
        assert "Dassl/dassl/" in raw[raw.index("FFM_OPTIM_ADAM / _AMSGRAD") - 1200:raw.index(f"int {name}(")]


def test_abi_version_is_still_14():
    assert _lib.ABI_VERSION == 14 and _lib.load().ffm_abi_version() == 14
    hdr = open(os.path.join(ROOT, "include", "ffm_hip.h")).read()
    assert re.search(r"#define FFM_ABI_VERSION 14\b", hdr) and "purely additive" in hdr


def test_state_rows():
    lib = _lib.load()
    assert [lib.ffm_optim_state_rows(_lib.OPTIM_KINDS[k]) for k in KINDS] == [1, 2, 2, 3, 2, 2]
    assert lib.ffm_optim_state_rows(6) == -1 and lib.ffm_optim_state_rows(-1) == -1


@pytest.mark.parametrize("fn", ["ffm_optim_step", "ffm_optim_step_dev"])
def test_invalid_arguments_return_einval_before_any_launch(fn):
    """Null pointers, n <= 0, repeats outside 1..16 and an unknown kind: -1 with no GPU in sight (the pointers handed in
    are never dereferenced: they are only compared with NULL)."""
    lib = _lib.load()
    f = getattr(lib, fn)
    d = O.OptimSpec(kind="adam").desc(1e-3, 0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    dp = ctypes.addressof(d)
    good = [p, p, p, 16, _lib.OPTIM_KINDS["adam"], dp, 2, None, None]
    for i in (0, 1, 2, 5):
        a = list(good)
        a[i] = None
        assert f(*a) == -1, (fn, "null argument", i)
    for n in (0, -5):
        assert f(p, p, p, n, 1, dp, 2, None, None) == -1
    for repeats in (0, 17, -1):
        assert f(p, p, p, 16, 1, dp, repeats, None, None) == -1
    for kind in (-1, 6, 99):
        assert f(p, p, p, 16, kind, dp, 2, None, None) == -1


def test_setup_cfg_carries_the_dassl_defaults(tmp_path):
    from fairfedmed_amd import federated_main as FM
    (tmp_path / "tr.yaml").write_text('OPTIM:\n  NAME: "adamw"\n  LR_SCHEDULER: "cosine"\n  WARMUP_EPOCH: 1\n'
                                      '  WARMUP_TYPE: "constant"\n')
    base = ["--root", "DATA/", "--trainer", "GLP_OT_SVLoRA", "--lr", "0.001"]
    o = FM.setup_cfg(FM.build_parser().parse_args(base)).OPTIM
    assert (o.NAME, o.LR_SCHEDULER, o.ADAM_BETA1, o.ADAM_BETA2, o.RMSPROP_ALPHA) == ("sgd", "single_step", 0.9, 0.999, 0.99)
    assert (o.WARMUP_EPOCH, o.WARMUP_TYPE, o.WARMUP_CONS_LR, o.WARMUP_MIN_LR, o.WARMUP_RECOUNT) == (-1, "linear", 1e-5, 1e-5, True)
    o = FM.setup_cfg(FM.build_parser().parse_args(base + ["--config-file", str(tmp_path / "tr.yaml")])).OPTIM
    assert (o.NAME, o.LR_SCHEDULER, o.WARMUP_EPOCH, o.WARMUP_TYPE, o.ADAM_BETA2) == ("adamw", "cosine", 1, "constant", 0.999)
    spec = O.build_optim_spec(o)
    assert spec.kind == "adamw" and spec.rows == 2
