"""The route of a transformer tower (fairfedmed_amd.engine.tower_route) and the engine's switches, without a GPU.

tower_route is a pure function of the tower's geometry, the row count and the switches, built on the library's host-side
queries alone; the tables below pin which fused kernels serve which batch size.  The ViT-B/16 table was taken from the five
per-fold methods that the route replaced, asked on an MI355X: the regime boundaries are exact, so a change to a tile table
or to a kernel's pre-conditions that moves one shows up here and not only in the step time.
"""
import dataclasses
import os

import pytest
import torch

from fairfedmed_amd.engine import Route, Switches, tower_route

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
H16 = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
ANY = pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
SW = Switches()

# ViT-B/16 (width 768, 12 heads, 197 tokens, not causal, packed weights), rank 8, both 16-bit storage types:
# images -> (ln1, ln2, lgrad, ln2_bwd, ln1_bwd, red_at); rows = images x 197.  Every row is the first or the last of a regime.
B16_TABLE = {
    13: (0, 0, 0, 0, 0, 0),
    14: (0, 0, 14, 0, 0, 0),
    27: (0, 0, 26, 0, 0, 0),
    28: (6, 6, 27, 8, 24, 0),
    32: (6, 6, 31, 8, 24, 0),
    34: (6, 6, 33, 8, 24, 0),
    35: (6, 3, 34, 0, 0, 0),
    36: (6, 3, 35, 0, 0, 0),
    37: (0, 3, 36, 0, 0, 0),
    64: (0, 3, 61, 0, 0, 0),
    65: (0, 3, 62, 0, 0, 2),
    100: (0, 3, 95, 0, 0, 2),
    110: (0, 3, 105, 0, 0, 2),
    111: (0, 0, 106, 0, 0, 2),
}


def panel_override() -> bool:
    """A tile selection from the environment (the mask_tolerant child runs) moves the boundaries: nothing to pin then."""
    return "FFM_PANEL" in os.environ or "FFM_PANEL_MASK" in os.environ


def b16(images: int, dtype=BF16, rank: int = 8, sw: Switches = SW, packed: bool = True) -> tuple:
    return dataclasses.astuple(tower_route(768, 12, 197, False, rank, dtype, packed, images * 197, sw))


def tiny(images: int, dtype) -> tuple:
    return dataclasses.astuple(tower_route(128, 2, 17, False, 4, dtype, dtype != F32, images * 17, SW))


@H16
def test_vit_b16_route_table(dtype):
    if panel_override():
        return
    got = {images: b16(images, dtype) for images in B16_TABLE}
    print("\n".join(f"{k:4d} {v}" for k, v in got.items()))
    assert got == B16_TABLE


@H16
def test_vit_b16_ranks_at_bs32(dtype):
    if panel_override():
        return
    r8 = B16_TABLE[32]
    assert b16(32, dtype, rank=16) == r8[:3] + (0,) + r8[4:], "rows 14 / 15 of the rank operand are taken: no ln_2 backward fold"
    assert b16(32, dtype, rank=4) == r8
    assert b16(32, dtype, rank=6) == (6, 6, 0, 0, 24, 0), "rank % 4: no FFM_EPI_LGRAD and with it no ln_2 backward fold"


def test_nothing_folds_without_a_fused_16_bit_rank():
    """float32 storage, rank 0 (the text tower), rank > 16 and vit_tiny's narrow tower: the all-zero route (their rowp /
    rowp2 / lnb_part buffers do not exist), the start of the reductions apart."""
    if panel_override():
        return
    for images in (1, 13, 32, 64, 65, 111):
        assert b16(images, F32, packed=False) == (0, 0, 0, 0, 0, 2 if images >= 65 else 0)
    for dtype in (BF16, F16):
        assert b16(32, dtype, rank=32)[:5] == (0,) * 5
    assert dataclasses.astuple(tower_route(512, 8, 10, True, 0, F32, False, 40, SW)) == (0,) * 6
    assert dataclasses.astuple(tower_route(512, 8, 77, True, 0, F32, False, 400 * 77, SW)) == (0,) * 6, \
        "no reductions to place in a tower without adapters"
    assert Route() == Route(0, 0, 0, 0, 0, 0)


@ANY
def test_vit_tiny_routes_are_all_zero(dtype):
    if panel_override():
        return
    assert all(tiny(images, dtype) == (0,) * 6 for images in range(1, 101))


def test_route_switches():
    if panel_override():
        return
    on = B16_TABLE[32]
    rep = lambda **k: dataclasses.replace(SW, **k)
    assert b16(32, sw=rep(lgrad=False)) == (6, 6, 0, 0, 24, 0), "FFM_LGRAD=0 takes ln_2's backward fold with it"
    assert b16(32, sw=rep(lnb_fold=False)) == on[:3] + (0, 0, 0)
    assert b16(32, sw=rep(lnb_fold1=False)) == on[:4] + (0, 0)
    for at in (0, 1, 2):
        assert b16(32, sw=rep(red_at=at)) == on[:5] + (at,)
        assert b16(100, sw=rep(red_at=at)) == B16_TABLE[100][:5] + (at,)
    assert b16(32, packed=False)[2:4] == (0, 0), "FFM_EPI_LGRAD lives in the panel kernel: packed weights only"


def test_route_is_frozen():
    with pytest.raises(dataclasses.FrozenInstanceError):
        Route().ln1 = 1
    with pytest.raises(dataclasses.FrozenInstanceError):
        SW.lgrad = False


# --------------------------------------------------------------------------------------------------- switches --
def test_switches_defaults():
    assert Switches.from_env({}) == Switches() == Switches(
        red_at=None, lgrad=True, pack_out=True, lnb_fold=True, lnb_fold1=True, bn_bwd_fused=True, f16_grad_scale=4096.0,
        f16_growth_interval=2000.0)


@pytest.mark.parametrize("env,field,value", [
    ({"FFM_RED_AT": "0"}, "red_at", 0), ({"FFM_RED_AT": "2"}, "red_at", 2),
    ({"FFM_LGRAD": "0"}, "lgrad", False), ({"FFM_LGRAD": "1"}, "lgrad", True),
    ({"FFM_PACK_OUT": "0"}, "pack_out", False),
    ({"FFM_LNB_FOLD": "0"}, "lnb_fold", False),
    ({"FFM_LNB_FOLD1": "0"}, "lnb_fold1", False),
    ({"FFM_BN_BWD_FUSED": "0"}, "bn_bwd_fused", False), ({"FFM_BN_BWD_FUSED": "1"}, "bn_bwd_fused", True),
    ({"FFM_F16_GRAD_SCALE": "1024"}, "f16_grad_scale", 1024.0),
    ({"FFM_F16_GROWTH_INTERVAL": "50"}, "f16_growth_interval", 50.0),
])
def test_switches_overrides(env, field, value):
    sw = Switches.from_env(env)
    assert getattr(sw, field) == value and type(getattr(sw, field)) is type(value)
    assert dataclasses.replace(sw, **{field: getattr(Switches(), field)}) == Switches(), "one variable moves one field"


def test_switches_read_the_process_environment(monkeypatch):
    monkeypatch.setenv("FFM_LNB_FOLD1", "0")
    monkeypatch.delenv("FFM_LNB_FOLD", raising=False)
    sw = Switches.from_env()
    assert sw.lnb_fold and not sw.lnb_fold1
