#!/usr/bin/env python3
"""One test()-shaped evaluation pass, timed both ways: ViT-B/16 FairLoRA r = 8, G = 3, bf16, batches of 100 synthetic images
(the reference's TEST.BATCH_SIZE), softmax per batch and the device metrics (ffm_eval_counts) at the end.

  forward leg   engine.forward() per batch - the evaluation pass as it was: the training forward, whole backward stash
                written, text tower per batch;
  infer leg     one inference() session, engine.infer() per batch - the forward-only pass on the depth-independent workspace.

The legs alternate (--pairs, default 3) after a warm-up pass of each and are timed with GPU events; the last line is one JSON
object with images/s of both, every pass's milliseconds, and torch.cuda.memory_allocated of an engine built
(max_images=32, max_infer_images=100) against one built (max_images=100).

    python tools/bench_eval.py [--batches 4] [--pairs 3] [--no-memory]
    python tools/bench_eval.py --leg forward|infer      one leg only (for a rocprofv3 --kernel-trace --stats run)
    python tools/bench_eval.py --bootstrap 1000         also the time TEST.BOOTSTRAP = 1000 adds to one test() ("bootstrap")
    python tools/bench_eval.py --stats <kernel_stats.csv> [...]   c_fc time per call from such runs (no GPU work):
                                                        the GEMM kernels whose epilogue flags hold FFM_EPI_GELU
"""
import argparse
import csv
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

EPI_GELU, EPI_GELU_ONLY = 16, 8192


def c_fc_stats(paths):
    """{file: {kernel: {calls, avg_us}}} for the GEMM kernels of a rocprofv3 kernel_stats CSV whose template flags hold
    FFM_EPI_GELU (gemm_panel_kernel<MF, NF, RK, FL, ...> / gemm_nt_kernel<T, RK, FL, ...>)."""
    out = {}
    for path in paths:
        rows = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                m = re.search(r"gemm_panel_kernel<\s*\d+,\s*\d+,\s*\w+,\s*(\d+)", name) or \
                    re.search(r"gemm_nt_kernel<[^,]+,\s*\w+,\s*(-?\d+)", name)
                if not m or int(m.group(1)) < 0 or not int(m.group(1)) & EPI_GELU:
                    continue
                calls = int(row.get("Calls") or 0)
                total = float(row.get("TotalDurationNs") or 0.0)
                rows[name] = {"calls": calls, "avg_us": total / max(calls, 1) / 1e3,
                              "gelu_only": bool(int(m.group(1)) & EPI_GELU_ONLY)}
        out[path] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch-size", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--leg", choices=["both", "forward", "infer"], default="both")
    ap.add_argument("--no-memory", action="store_true")
    ap.add_argument("--stats", nargs="+")
    ap.add_argument("--bootstrap", type=int, default=0,
                    help="also report what TEST.BOOTSTRAP = B adds to one test(): the replicate tables and their scoring")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps({"c_fc_kernels": c_fc_stats(a.stats)}))
        return

    import torch
    from fairfedmed_amd import config as C, ops, synth
    from fairfedmed_amd.engine import FairLoRAEngine

    mcfg = C.vit_b16(rank=8)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    bs = a.batch_size
    batches = []
    for i in range(a.batches):
        b = synth.make_batch(mcfg, bs, seed=100 + i, signal=0.2)
        batches.append((b["img"].cuda(), b["attrs"].t()[0].contiguous().cuda(), b["label"].cuda(), b["attrs"].t().contiguous().cuda()))
    eng = FairLoRAEngine(mcfg, sd, dtype=torch.bfloat16, max_images=bs)

    def finish(probs):
        prob = torch.cat(probs).float().contiguous()
        y = torch.cat([b[2] for b in batches]).contiguous()
        at = torch.cat([b[3] for b in batches], dim=1)
        return torch.stack([ops.eval_counts(prob, y, at[k].contiguous(), 8) for k in range(at.shape[0])])

    def leg_forward():
        return finish([torch.softmax(eng.forward(img, attr), -1) for img, attr, _, _ in batches])

    def leg_infer():
        with eng.inference():
            return finish([torch.softmax(eng.infer(img, attr), -1) for img, attr, _, _ in batches])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    legs = {"forward": leg_forward, "infer": leg_infer}
    names = ["forward", "infer"] if a.leg == "both" else [a.leg]
    ref = {n: legs[n]() for n in names}                           # warm-up: kernel attributes, allocator, fold caches
    torch.cuda.synchronize()
    if a.leg == "both":
        assert torch.equal(ref["forward"], ref["infer"]), "the two passes disagree"
    ms = {n: [] for n in names}
    for _ in range(a.pairs):
        for n in names:
            t, out = timed(legs[n])
            assert torch.equal(out, ref[n])
            ms[n].append(t)
    images = bs * a.batches
    res = {"workload": f"test()-shaped pass: ViT-B/16 FairLoRA r=8 G=3 bf16, {a.batches} batches of {bs} synthetic images, "
                       "softmax per batch + device metrics", "images": images, "pairs": a.pairs}
    for n in names:
        best = min(ms[n])
        res[f"{n}_ms"] = [round(t, 3) for t in ms[n]]
        res[f"{n}_images_per_sec"] = round(images / best * 1e3, 1)
    if a.leg == "both":
        res["speedup"] = round(min(ms["forward"]) / min(ms["infer"]), 4)
    if a.bootstrap > 0:
        # what TEST.BOOTSTRAP adds to one test(): the replicate tables of every attribute column with their one D2H copy
        # (GPU events), and the host's scoring of them (wall time)
        import time
        from fairfedmed_amd import metrics as M
        with eng.inference():
            prob = torch.cat([torch.softmax(eng.infer(img, attr), -1) for img, attr, _, _ in batches]).float().contiguous()
        y = torch.cat([b[2] for b in batches]).contiguous()
        at = torch.cat([b[3] for b in batches], dim=1)
        tables = ref[names[-1]].cpu().numpy()

        def boot():
            return torch.stack([ops.eval_boot_counts(prob, y, at[k].contiguous(), 8, a.bootstrap, 0, tag=1)
                                for k in range(at.shape[0])]).cpu().numpy()

        boot()
        runs = [timed(boot) for _ in range(a.pairs)]
        t0 = time.perf_counter()
        ci = M.bootstrap_intervals(tables, runs[-1][1])
        res["bootstrap"] = {"replicates": a.bootstrap, "samples": images, "attribute_columns": int(at.shape[0]),
                            "tables_ms": [round(t, 3) for t, _ in runs],
                            "intervals_host_ms": round((time.perf_counter() - t0) * 1e3, 3), "degenerate": ci["degenerate"]}
    if not a.no_memory and a.leg == "both":
        res["workspace_bytes"] = eng.infer_ws.nbytes()
        import gc
        del eng, ref, legs
        gc.collect()                                                # (an engine holds reference cycles: collect before counting)
        torch.cuda.empty_cache()
        mem = {}
        for key, kw in (("max_images=100", dict(max_images=100)), ("max_images=32,max_infer_images=100", dict(max_images=32, max_infer_images=100))):
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            e = FairLoRAEngine(mcfg, sd, dtype=torch.bfloat16, **kw)
            torch.cuda.synchronize()
            mem[key] = torch.cuda.memory_allocated() - before
            del e
            gc.collect()
            torch.cuda.empty_cache()
        res["engine_bytes_allocated"] = mem
    print(json.dumps(res))


if __name__ == "__main__":
    main()
