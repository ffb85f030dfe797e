#!/usr/bin/env python
"""A short training loop of the ViT-B/16 r=8 engine (bs 32, bf16) that steps every optimizer in turn - three steps of
forward_backward + sgd_step / optim_step(repeats=2) each - for one `rocprofv3 --kernel-trace --stats` run: the launch time
of `optim_kernel<kind>` next to `sgd_n_kernel` at the real trainable buffer (741 952 elements).

    rocprofv3 --kernel-trace --stats -d out -o optim -- python tools/optim_steps.py
    python tools/optim_steps.py --stats out/*/optim_kernel_stats.csv        # the rows of the optimizer kernels
"""
import argparse
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(steps: int) -> None:
    import torch
    from fairfedmed_amd import config as C, synth
    from fairfedmed_amd.engine import FairLoRAEngine
    from fairfedmed_amd.optim import OptimSpec
    mcfg, bs = C.vit_b16(rank=8), 32
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    eng = FairLoRAEngine(mcfg, sd, dtype=torch.bfloat16, max_images=bs)
    b = synth.make_batch(mcfg, bs, seed=3, signal=0.2)
    img, attr, label = b["img"].cuda(), b["attrs"].t()[0].contiguous().cuda(), b["label"].cuda()
    for kind in ("sgd", "adam", "adamw", "amsgrad", "rmsprop", "radam"):
        spec = OptimSpec(kind=kind)
        eng.params.optim_state.zero_()
        eng.params.steps = 0
        for _ in range(steps):
            eng.forward_backward(img, attr, label)
            if kind == "sgd":
                eng.sgd_step(1e-3, 0.9, 5e-4, repeats=2)
            else:
                eng.optim_step(spec, 1e-3, repeats=2)
        torch.cuda.synchronize()
    print("numel", eng.params.numel, "finite", bool(torch.isfinite(eng.params.flat).all()))


def stats(paths) -> None:
    for path in paths:
        for row in csv.DictReader(open(path)):
            if "optim_kernel" in row["Name"] or "sgd_n_kernel" in row["Name"]:
                print(f'{row["Name"][:90]:90s} calls {row["Calls"]:>3s}  avg {float(row["AverageNs"]) / 1e3:7.2f} us  '
                      f'min {float(row["MinNs"]) / 1e3:7.2f}  max {float(row["MaxNs"]) / 1e3:7.2f}')


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--stats", nargs="*")
    a = ap.parse_args()
    stats(a.stats) if a.stats else run(a.steps)
