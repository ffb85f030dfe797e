"""What the panel-GEMM selector may answer, without a GPU: conditions on ffm_gemm_tile_shape / tiles_m / tiles_n /
lgrad_rows over a grid of shapes, ranks, storage types and epilogue words, in every setting of FFM_PANEL / FFM_PANEL_MASK.

The switches are read once per process, so every setting runs this file as a child process (`python <file> --child`),
which walks the grid, asserts the conditions case by case and prints the configurations it met; the parent then asserts
that the grid reached every configuration its setting enables, so that the conditions cannot hold by selecting nothing.
The conditions say which (tile configuration, epilogue) pairs are instantiated: a selector that answers outside them
sends ffm_gemm_nt to a kernel that does not exist.
"""
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# setting -> (environment, configurations the grid must reach; None: it must reach none at all)
SETTINGS = {
    "default": ({}, {2, 3, 7, 8, 10}),
    "mask0": ({"FFM_PANEL_MASK": "0"}, {0, 1, 2, 3, 4}),
    "mask7552": ({"FFM_PANEL_MASK": "7552"}, {2, 3, 7, 8, 10, 11, 12}),      # default + the K split (the GPU suite's value)
    # every mask bit set: the conditions hold there too; which rows win the cost model with all of them enabled is not
    # part of the contract, so nothing is required of the reach (the empty set)
    "mask8191": ({"FFM_PANEL_MASK": "8191"}, set()),
    "off": ({"FFM_PANEL": "off"}, None),
}

# (rows, columns, waves per CU) of every built configuration; 5, 6 and 9 are not built
SHAPES = {0: (208, 384, 4), 1: (256, 256, 4), 2: (160, 128, 4), 3: (176, 128, 4), 4: (128, 256, 8), 7: (208, 384, 8),
          8: (160, 128, 4), 10: (240, 256, 8), 11: (160, 128, 8), 12: (160, 128, 8)}
MS = [1, 64, 65, 197, 788, 1576, 2561, 2758, 5516, 6304, 8865, 12608, 12609, 19700]
NKS = [(768, 768), (2304, 768), (768, 2304), (3072, 768), (768, 3072), (512, 512), (1536, 512), (512, 1536), (2048, 512),
       (512, 2048), (1024, 1024), (3072, 1024), (4096, 1024), (1024, 4096), (384, 1536), (128, 512), (256, 1024), (768, 640),
       (192, 192), (576, 192), (768, 1536), (1536, 1536)]
RANKS = [0, 4, 6, 8, 14, 16, 17]


def words(L):
    """(the epilogue words of the panel launch tables and of ffm_gemm_nt's cases, those with one epilogue bit flipped)"""
    B, LO, KR, R, G, DG, RK = L.EPI_BIAS, L.EPI_LORA, L.EPI_LORA_KR, L.EPI_RESIDUAL, L.EPI_GELU, L.EPI_DGELU, L.EPI_RANKOP
    RS, LI, LG, BN, LS, LA, GO = L.EPI_ROWSTATS, L.EPI_LNIN, L.EPI_LGRAD, L.EPI_BNBWD, L.EPI_LNB_STAT, L.EPI_LNB_APPLY, L.EPI_GELU_ONLY
    base = [0, B, B | R, B | R | RS, B | LI, LA,
            RK | B | LO | G, RK | B | LO | G | LI, RK | B | LO | G | GO, RK | B | LO | G | GO | LI, RK | B | LO | R, RK | B | LO | R | RS,
            RK | LO | KR | DG, RK | LO | KR, RK | LO | KR | LA, RK | LO | KR | DG | LG, RK | LO | KR | DG | LG | LS,
            RK | LO, RK | B | LO, RK | LO | KR | R, RK | LO | KR | BN, RK | LO | KR | R | BN,
            B | G, B | G | GO, DG, B | LO, B | LO | G, B | LO | G | GO, B | LO | R, LO | KR, LO | KR | DG, BN]
    base = sorted(set(base))
    flipped = sorted({w ^ (1 << i) for w in base for i in range(14)} - set(base))
    return base, flipped


def child():
    sys.path.insert(0, ROOT)
    import torch
    from fairfedmed_amd import _lib as L
    from fairfedmed_amd import ops
    bf16, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    base, flipped = words(L)
    dxproj = L.EPI_LORA | L.EPI_LORA_KR | L.EPI_DGELU | L.EPI_RANKOP

    def ask(M, N, K, w, r, dt, pk):
        return (ops.gemm_tile_shape(M, N, K, w, r, dt, pk), ops.gemm_tiles_m(M, N, K, w, r, dt, pk), ops.gemm_tiles_n(M, N, K, w, r, dt, pk))

    reached, cases = set(), 0
    # the full grid for bfloat16 on a packed weight with the words as written, every 19th case with a flipped bit
    grid = itertools.chain(itertools.product(MS, NKS, RANKS, base),
                           itertools.islice(itertools.product(MS, NKS, RANKS, flipped), 0, None, 19))
    for M, (N, K), r, w in grid:
        cases += 1
        ans = ask(M, N, K, w, r, bf16, True)
        (cfg, rows, cols, waves), tm, tn = ans
        where = f"M {M} N {N} K {K} flags {w} rank {r}: {ans}"
        if cfg >= 0 or cases % 3 == 0:      # (every selected case, a third of the refused ones)
            assert ask(M, N, K, w | L.EPI_GELU_ONLY, r, bf16, True) == ans, "FFM_EPI_GELU_ONLY moved the answer, " + where
            assert ask(M, N, K, w, r, f16, True) == ans, "float16 differs from bfloat16, " + where
        if cases % 7 == 0:      # nothing but a packed 16-bit weight reaches the panel kernel
            assert ask(M, N, K, w, r, f32, True)[0][0] == -1 and ask(M, N, K, w, r, bf16, False)[0][0] == -1, where
            assert ask(M, N, K, w, r, f32, False)[0][0] == -1 and ask(M, N, K, w, r, f16, False)[0][0] == -1, where
        if w == dxproj:
            lg = ops.gemm_lgrad_rows(M, N, K, r, bf16, True)
            served = ops.gemm_tile_shape(M, N, K, w | L.EPI_LGRAD, r, bf16, True)[0]
            assert served in (-1, 7), where
            assert (lg == -(-M // 208)) if served == 7 else (lg < 0), f"lgrad_rows {lg}, " + where
            assert lg == ops.gemm_lgrad_rows(M, N, K, r, f16, True), where
        if cfg < 0:
            continue
        reached.add(cfg)
        rk = bool(w & L.EPI_RANKOP)
        assert cfg in SHAPES and (rows, cols, waves) == SHAPES[cfg], where
        assert N % cols == 0 and tn == N // cols and tm == -(-M // rows) * (N // cols), where
        assert (1 <= r <= 16 and cfg in (0, 3, 7, 8, 11)) if rk else cfg in (1, 2, 4, 10, 12), where
        if w & L.EPI_LGRAD:
            assert (rows, cols, waves) == (208, 384, 8) and r % 4 == 0, where
        if w & L.EPI_LNB_STAT:
            assert w & L.EPI_LGRAD, where
        if w & L.EPI_LNB_APPLY:
            assert (cfg == 8 and r <= 14) if rk else cfg == 2, where
        if w & L.EPI_ROWSTATS:
            assert cfg not in (0, 7), where
        assert not w & L.EPI_BNBWD, where
    print(json.dumps({"reached": sorted(reached), "cases": cases}))


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_panel_selection_conditions(setting):
    extra, expect = SETTINGS[setting]
    env = {k: v for k, v in os.environ.items() if k not in ("FFM_PANEL", "FFM_PANEL_MASK")}
    env.update(extra, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=60)      # (a child takes about 5 s)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(setting, out)
    reached = set(out["reached"])
    assert out["cases"] > 60000 and reached <= set(SHAPES)
    assert not reached if expect is None else reached >= expect


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    child()
