#!/usr/bin/env python
"""Attention forward + backward at B = 32, heads = 12 in bf16 for one `rocprofv3 --kernel-trace --stats` run: L = 256 (the
third-generation kernels, the longest length they serve) next to L = 257, 577 and 1025 (the streaming kernels of
csrc/attention_long.hip), and - in a child process started with FFM_ATTN=v1 - L = 256 on the first-generation kernels,
whose orientation and staging the streaming kernels share.

    rocprofv3 --kernel-trace --stats -d out -o attn -- python tools/attn_long_times.py
    python tools/attn_long_times.py --trace out/*/*_results.db           # (or *kernel_trace.csv) us per kernel and length

The lengths run through the same three kernel names, so the second form reads the per-dispatch trace and tells the lengths
apart by their grids (one block per (b, h, 64-token tile) in the streaming kernels) instead of the per-name statistics.
The first form also prints device-event times of forward and backward (launch gaps included) as a cross-check.
"""
import argparse
import csv
import os
import subprocess
import sys
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, HEADS = 32, 12


def run(lengths, reps: int) -> None:
    import torch
    from fairfedmed_amd import ops
    E = HEADS * 64
    gen = os.environ.get("FFM_ATTN", "default")
    for L in lengths:
        g = torch.Generator(device="cuda").manual_seed(L)
        qkv = torch.randn(B * L, 3 * E, device="cuda", generator=g).bfloat16()
        dout = torch.randn(B * L, E, device="cuda", generator=g).bfloat16()
        out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
        lse, delta = torch.empty(B, HEADS, L, device="cuda"), torch.empty(B, HEADS, L, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        tf = tb = 0.0
        for it in range(reps + 2):                                   # two warm-up rounds
            ev[0].record()
            ops.attention_fwd(qkv, out, lse, B, L, HEADS, False)
            ev[1].record()
            ops.attention_bwd(qkv, out, dout, lse, delta, dqkv, B, L, HEADS, False)
            ev[2].record()
            torch.cuda.synchronize()
            if it >= 2:
                tf += ev[0].elapsed_time(ev[1])
                tb += ev[1].elapsed_time(ev[2])
        scores = B * HEADS * L * L
        ok = bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
        print(f"FFM_ATTN={gen} L={L} blocks_long={B * HEADS * ((L + 63) // 64)} events: fwd {tf / reps * 1e3:8.1f} us "
              f"({tf / reps * 1e6 / scores:.4f} ns/score)  bwd {tb / reps * 1e3:8.1f} us ({tb / reps * 1e6 / scores:.4f} ns/score) "
              f"finite {ok}", flush=True)


def dispatches(path):
    """(kernel name, blocks, microseconds) of every dispatch in a rocprofv3 output file: the kernel-trace CSV or the
    SQLite database (`*_results.db`, view `kernels`) that newer versions write by default."""
    if path.endswith(".db"):
        import sqlite3
        with sqlite3.connect(path) as db:
            for name, dur, grid, wg in db.execute("select name, duration, grid_x, workgroup_x from kernels order by start"):
                yield name, grid // max(wg, 1), dur / 1e3
        return
    for row in csv.DictReader(open(path)):
        wg = int(row.get("Workgroup_Size_X") or row.get("Workgroup_Size") or 1)
        grid = int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0)
        yield row.get("Kernel_Name", ""), grid // max(wg, 1), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3


def trace(paths) -> None:
    """Per trace file: attention kernel, blocks -> calls, mean / min microseconds and, for the streaming kernels (whose grid
    gives L among the lengths this tool runs), picoseconds per score."""
    length_of = {B * HEADS * ((L + 63) // 64): L for L in (257, 577, 1025)}
    for path in paths:
        rows = defaultdict(list)
        for name, blocks, us in dispatches(path):
            if "attn" in name or "al_fwd" in name or "al_bwd" in name:
                short = name.split("(")[0].split("<")[0].split("::")[-1]
                rows[(short[:72], blocks)].append(us)
        print(path)
        for (short, blocks), us in rows.items():
            us = us[2:] if len(us) > 4 else us                        # drop the warm-up rounds
            L = length_of.get(blocks) if "al_" in short else None
            per = f"  L {L}: {sum(us) / len(us) * 1e6 / (B * HEADS * L * L):.2f} ps/score" if L else ""
            print(f"  {short:72s} blocks {blocks:6d}  calls {len(us):3d}  mean {sum(us) / len(us):8.1f} us  min {min(us):8.1f} us{per}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", type=int, nargs="*", default=[256, 257, 577, 1025])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-child", action="store_true", help="skip the FFM_ATTN=v1 child process (L = 256)")
    ap.add_argument("--trace", nargs="+", help="rocprofv3 output files to summarise instead of running")
    a = ap.parse_args()
    if a.trace is not None:
        trace(a.trace)
    else:
        run(a.lengths, a.reps)
        if not a.no_child and "FFM_ATTN" not in os.environ:
            # a fresh process: the generation switch is read once per process
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lengths", "256", "--reps", str(a.reps), "--no-child"],
                               env=dict(os.environ, FFM_ATTN="v1"), timeout=600)
            sys.exit(r.returncode)
