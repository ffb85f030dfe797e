#!/usr/bin/env python3
"""Device time of the train-time augmentation: events around ops.augment_u8 (the box draw and the
crop / resample / flip, two launches) for 32 stored images -> 224, both filters; beside each, ops.resize_u8 on the same
bytes - the test-time resize, whose filter has other tap counts: context, not a gate.  20 calls after 5 warm-up calls."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from fairfedmed_amd import config as C, data as D, ops

B, R, WARM, CALLS = 32, 224, 5, 20


def timed(fn):
    for _ in range(WARM):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
    return {"min_us": round(us[0], 1), "median_us": round(us[len(us) // 2], 1), "max_us": round(us[-1], 1)}


def main():
    g = np.random.default_rng(0)
    dst = torch.empty(B, 3, R, R, device="cuda")
    boxes = torch.empty(B, 8, device="cuda", dtype=torch.int32)
    for h, w in ((224, 224), (336, 336), (512, 664)):
        samples = [g.integers(0, 256, size=(1, h, w), dtype=np.uint8) for _ in range(B)]
        plain = D.NativeBatch.from_planes(samples, 3, R).to("cuda")
        row = {"stored": [h, w], "images": B, "R": R, "resize_u8": timed(lambda: ops.resize_u8(plain, dst)), "resize_u8_taps": plain.T}
        for f in C.INTERPOLATIONS:
            nb = D.NativeBatch.augmented(samples, 3, R, list(range(B)), 0, 1, C.AugmentCfg(crop=True, flip=True, filter=f)).to("cuda")
            row["augment_u8_" + f] = timed(lambda: ops.augment_u8(nb, dst, boxes))
            whole = D.NativeBatch.augmented(samples, 3, R, list(range(B)), 0, 1, C.AugmentCfg(flip=True, filter=f)).to("cuda")
            row["augment_u8_" + f + "_whole_plane"] = timed(lambda: ops.augment_u8(whole, dst, boxes))
            row["taps_" + f] = ops.augment_taps(max(h, w), R, f)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
