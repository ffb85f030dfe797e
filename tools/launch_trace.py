#!/usr/bin/env python3
"""Canonical launch trace of one training step (or one evaluation pass) per case, for comparing two commits bit for bit:
one line per entry of the recorded plan - the launch's name, every scalar argument, every field of ffm_gemm_nt's struct,
the descriptor entries of the two *_multi launches, host-side callables as `host`.  Every pointer (streams included) is
replaced by the index of its first appearance, so the trace does not depend on where the allocator put a buffer but
does pin which launches share one.  Prints `case sha256` per case; --out DIR also keeps the traces.

    python tools/launch_trace.py [--out DIR] [case ...]
"""
import ctypes as C
import dataclasses
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fairfedmed_amd import _lib as L, config as cfgs, ops, synth
from fairfedmed_amd.engine_rn import create_engine

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def route_cfg():
    """The tower of tests/test_route_gpu.py: ViT-B/16 width / heads / tokens, 2 vision layers, the tiny text tower."""
    base = cfgs.vit_b16(rank=8)
    return dataclasses.replace(base, vision=dataclasses.replace(base.vision, layers=2), text=cfgs.vit_tiny().text)


# case -> (config, dtype, max_images, images, mode[, environment]); mode: train | infer (outside a session) | session (inside one)
CASES = {f"route_{d}_{n}": (route_cfg, d, 28, n, "train") for d, n in (("bf16", 13), ("bf16", 14), ("bf16", 28), ("f16", 28))}
CASES.update({f"tiny_r{r}_{d}": ((lambda r=r: cfgs.vit_tiny(rank=r)), d, 3, 3, "train")
              for r, d in ((4, "f32"), (4, "bf16"), (24, "bf16"))})
CASES.update({"tiny_svlora": (lambda: cfgs.vit_tiny_lora("SVLoRA"), "bf16", 3, 3, "train"),
              "tiny_lora": (lambda: cfgs.vit_tiny_lora("LoRA"), "bf16", 3, 3, "train"),
              "tiny_global_s": (lambda: cfgs.vit_tiny_lora("FairLoRA", global_s=True), "bf16", 3, 3, "train"),
              "tiny_3d": (cfgs.vit_tiny_3d, "bf16", 6, 3, "train")})
CASES.update({f"rn_r{r}_{d}": ((lambda r=r: cfgs.rn_tiny2(rank=r)), d, 3, 3, "train")
              for r, d in ((4, "bf16"), (4, "f32"), (24, "bf16"))})
for _m in ("infer", "session"):
    CASES[f"{_m}_route_28"] = (route_cfg, "bf16", 28, 28, _m)
    CASES[f"{_m}_tiny_r24"] = ((lambda: cfgs.vit_tiny(rank=24)), "bf16", 3, 3, _m)


def on(mk_cfg, targets):
    """The same tower with its adapters on `targets` (LoraCfg.targets: 'attn' / 'mlp+attn')."""
    def mk():
        c = mk_cfg()
        return dataclasses.replace(c, lora=dataclasses.replace(c.lora, targets=targets))
    return mk


# adapters on attn.in_proj / attn.out_proj too ("ma": mlp+attn) or alone ("a": attn)
CASES.update({f"route_ma_bf16_{n}": (on(route_cfg, "mlp+attn"), "bf16", 28, n, "train") for n in (13, 28)})
CASES["route_a_bf16_28"] = (on(route_cfg, "attn"), "bf16", 28, 28, "train")
CASES.update({f"tiny_ma_r{r}_{d}": (on((lambda r=r: cfgs.vit_tiny(rank=r)), "mlp+attn"), d, 3, 3, "train")
              for r, d in ((4, "f32"), (4, "bf16"), (24, "bf16"))})
CASES["tiny_a_r24_bf16"] = (on(lambda: cfgs.vit_tiny(rank=24), "attn"), "bf16", 3, 3, "train")
CASES["tiny_3d_ma"] = (on(cfgs.vit_tiny_3d, "mlp+attn"), "bf16", 6, 3, "train")
# where a block's reductions start (FFM_RED_AT=1|2; by row count only the 19 700-row workload leaves 0), without and with
# attention sites; a sixth element: environment switches for the engine's construction
for _at in "12":
    CASES[f"route_red{_at}_bf16_28"] = (route_cfg, "bf16", 28, 28, "train", {"FFM_RED_AT": _at})
    CASES[f"route_ma_red{_at}_bf16_28"] = (on(route_cfg, "mlp+attn"), "bf16", 28, 28, "train", {"FFM_RED_AT": _at})
for _m in ("infer", "session"):
    CASES[f"{_m}_route_ma_28"] =(on(route_cfg, "mlp+attn"), "bf16", 28, 28, _m)
    CASES[f"{_m}_tiny_ma_r24"] = (on(lambda: cfgs.vit_tiny(rank=24), "mlp+attn"), "bf16", 3, 3, _m)


def record_case(mk_cfg, dtype, max_images, images, mode, env=None):
    mcfg = mk_cfg()
    old = {k: os.environ.get(k) for k in env or {}}
    os.environ.update(env or {})                                # (the engine reads its switches when it is constructed)
    try:
        eng = create_engine(mcfg, synth.make_state_dict(mcfg, seed=1, lora_init="random"), dtype=DT[dtype], max_images=max_images)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    eng.use_replay = False                                      # the engine must not record itself
    b = synth.make_batch(mcfg, images, seed=1234)
    img, attr, label = b["img"].cuda(), b["attrs"].t()[0].contiguous().cuda(), b["label"].cuda()
    plan = []
    if mode == "train":
        with ops.record(plan):
            eng.forward_backward(img, attr, label)
    elif mode == "infer":
        with ops.record(plan):
            eng.infer(img, attr)
    else:
        with eng.inference(), ops.record(plan):
            eng.infer(img, attr)
    torch.cuda.synchronize()
    return plan


class _Table:
    """Marker a wrapped ReducePlan.run / PackPlan.run leaves in the plan in front of its launches: the descriptor entries."""

    def __init__(self, p):
        self.kind, self.keep = type(p).__name__, p.keep


def _wrap(cls):
    run = cls.run

    def traced(self):
        ops.record_callable(_Table(self))
        run(self)
    cls.run = traced


def canonical(plan) -> str:
    seen = {}

    def ptr(p):
        p = p.data_ptr() if isinstance(p, torch.Tensor) else p
        return "null" if not p else "p%d" % seen.setdefault(p, len(seen))

    def val(x):                                                 # a descriptor entry's element
        if isinstance(x, torch.Tensor):
            return ptr(x)
        return "(" + ",".join(val(y) for y in x) + ")" if isinstance(x, (tuple, list)) else repr(x)

    lines = []
    for f in plan:
        if isinstance(f, _Table):
            for ent in f.keep:                                  # PackPlan entries are 3 .. 6 long: padded to the descriptor
                ent = tuple(ent) + (None,) * (6 - len(ent)) if f.kind == "PackPlan" else ent
                lines.append(f"  {f.kind} " + " ".join(val(x) for x in ent))
        elif not isinstance(f, ops._Launch):
            lines.append("host")
        else:
            out = [f.name]
            for a, ty in zip(f.args, f.fn.argtypes):
                if f.name == "ffm_gemm_nt" and hasattr(a, "_obj"):
                    out += [f"{n}={ptr(getattr(a._obj, n)) if t is C.c_void_p else getattr(a._obj, n)!r}"
                            for n, t in L.GemmArgs._fields_]
                elif ty is C.c_void_p:
                    out.append(ptr(a))
                else:
                    out.append(repr(list(a)) if isinstance(a, C.Array) else repr(a))
            lines.append(" ".join(out))
    return "\n".join(lines) + "\n"


def main(argv):
    out_dir = None
    if argv[:1] == ["--out"]:
        out_dir, argv = argv[1], argv[2:]
        os.makedirs(out_dir, exist_ok=True)
    _wrap(ops.ReducePlan)
    _wrap(ops.PackPlan)
    for name in argv or list(CASES):
        text = canonical(record_case(*CASES[name]))
        if out_dir:
            with open(os.path.join(out_dir, name + ".txt"), "w") as fh:
                fh.write(text)
        print(name, hashlib.sha256(text.encode()).hexdigest(), text.count("\n"), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
