"""The forward-only evaluation path, host side (no GPU): FFM_EPI_GELU_ONLY in the header and in _lib.py, its argument
validation in ffm_gemm_nt, and kernel selection - the bit must never move a product to another tile, or the evaluation
pass would fold LayerNorms differently from forward() and stop being bit-identical to it."""
import ctypes
import os
import re

import pytest
import torch

from fairfedmed_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffm_hip.h")


def _define(name: str) -> int:
    m = re.search(r"^#define\s+%s\s+(-?\d+)" % name, open(HEADER).read(), flags=re.M)
    assert m, name
    return int(m.group(1))


def test_header_and_lib_agree_on_gelu_only_and_abi_14():
    assert _define("FFM_EPI_GELU_ONLY") == 8192 == _lib.EPI_GELU_ONLY
    assert _define("FFM_ABI_VERSION") == 14 == _lib.ABI_VERSION
    assert _lib.load().ffm_abi_version() == 14
    # the next free bit: no other epilogue flag of the header shares it
    flags = {n: int(v) for n, v in re.findall(r"^#define\s+(FFM_EPI_\w+)\s+(\d+)", open(HEADER).read(), flags=re.M)}
    assert [n for n, v in flags.items() if v & 8192] == ["FFM_EPI_GELU_ONLY"]


def _args(flags: int, gelu_deriv: int) -> "_lib.GemmArgs":
    """A well-formed 128 x 128 x 128 bf16 product on made-up (aligned, never dereferenced) addresses: the validation under
    test answers before anything is launched."""
    a = _lib.GemmArgs()
    a.a, a.b, a.c, a.bias, a.c2 = 0x10000, 0x20000, 0x30000, 0x40000, None
    a.M = a.N = a.K = a.lda = a.ldb = a.ldc = 128
    a.flags, a.gelu_deriv = flags, gelu_deriv
    return a


@pytest.mark.parametrize("dtype", [_lib.BF16, _lib.F16, _lib.F32], ids=["bf16", "f16", "f32"])
def test_gemm_nt_rejects_malformed_gelu_only(dtype):
    lib = _lib.load()
    E = _lib
    # (-1: FFM_EINVAL) without FFM_EPI_GELU the bit means nothing
    assert lib.ffm_gemm_nt(ctypes.byref(_args(E.EPI_BIAS | E.EPI_GELU_ONLY, 0)), dtype, None) == -1
    # the derivative form stores two tensors: it has no activation-only variant
    assert lib.ffm_gemm_nt(ctypes.byref(_args(E.EPI_BIAS | E.EPI_GELU | E.EPI_GELU_ONLY, 1)), dtype, None) == -1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
def test_gelu_only_never_moves_a_product_to_another_tile(dtype, packed):
    """The shapes of test_bench_shapes_select_the_documented_tiles (6 304 rows = 32 images, 19 700 = 100 images): every
    query whose flags hold EPI_GELU answers the same with and without EPI_GELU_ONLY."""
    from fairfedmed_amd import ops
    W, E = 768, _lib
    rk = E.EPI_LORA | E.EPI_RANKOP
    gelu_flags = [E.EPI_BIAS | E.EPI_GELU | E.EPI_LNIN | rk, E.EPI_BIAS | E.EPI_GELU | rk,
                  E.EPI_BIAS | E.EPI_GELU | E.EPI_LORA, E.EPI_BIAS | E.EPI_GELU]
    seen_panel = False
    for M in (32 * 197, 100 * 197):
        for fl in gelu_flags:
            for r in ((8, 16) if fl & E.EPI_LORA else (0,)):
                q = (M, 4 * W, W)
                base = ops.gemm_tile_shape(*q, fl, r, dtype, packed)
                assert ops.gemm_tile_shape(*q, fl | E.EPI_GELU_ONLY, r, dtype, packed) == base, (M, fl, r)
                seen_panel |= base[0] >= 0
                for fn in (ops.gemm_tiles_m, ops.gemm_tiles_n):
                    assert fn(*q, fl | E.EPI_GELU_ONLY, r, dtype, packed) == fn(*q, fl, r, dtype, packed), (fn.__name__, M, fl, r)
    # (not vacuous: the packed 16-bit FairLoRA products are on the panel kernel, everything else on the 128 x 128 one)
    assert seen_panel == (packed and dtype != torch.float32)
