"""Which attention kernels serve a length, on the device: the four entry points of csrc/attention.hip agree with each other at
the smallest shapes that cross a routing boundary - 96 / 97 tokens (the floor of ffm_attention_bwd_lnstat) and 256 / 257 (the
hand-over to the streaming kernels of attention_long.hip).

What the kernels compute is held to float64 in test_kernels_gpu.py and test_attention_long_gpu.py; here only the status of
each call and that a served call wrote all of its output.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, HEADS, E = 1, 2, 128
FFM_OK, FFM_EUNSUP = 0, -2


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("L", [96, 97, 256, 257])
def test_the_four_attention_entry_points_agree_on_the_route(dt, L):
    from fairfedmed_amd import _lib
    lib, code, s = _lib.load(), _lib.dtype_code(dt), _lib.stream_ptr()
    g = torch.Generator(device="cuda").manual_seed(L)
    qkv = torch.randn(B * L, 3 * E, device="cuda", generator=g).to(dt)
    dout = torch.randn(B * L, E, device="cuda", generator=g).to(dt)
    nan = lambda *shape, dtype=torch.float32: torch.full(shape, float("nan"), device="cuda", dtype=dtype)
    out, lse, delta = nan(B * L, E, dtype=dt), nan(B, HEADS, L), nan(B, HEADS, L)
    p = _lib.ptr
    assert lib.ffm_attention_fwd(p(qkv), p(out), p(lse), B, L, HEADS, 0, code, s) == FFM_OK
    dqkv = nan(B * L, 3 * E, dtype=dt)
    assert lib.ffm_attention_bwd(p(qkv), p(out), p(dout), p(lse), p(delta), p(dqkv), B, L, HEADS, 0, code, s) == FFM_OK
    torch.cuda.synchronize()
    for name, t in (("out", out), ("lse", lse), ("dqkv", dqkv)):
        assert torch.isfinite(t.float()).all(), f"{name} at L = {L}"

    served = lib.ffm_attention_bwd_lnstat_ok(L, 0, code)
    assert served == (1 if 97 <= L <= 256 else 0)
    wg, d = torch.randn(3 * E, device="cuda", generator=g), torch.randn(3 * E, device="cuda", generator=g)
    part, dqkv2 = nan(2 * HEADS, B * L, 2), nan(B * L, 3 * E, dtype=dt)
    rc = lib.ffm_attention_bwd_lnstat(p(qkv), p(out), p(dout), p(lse), p(delta), p(dqkv2), p(wg), p(d), p(part), B, L, HEADS, 0, code, s)
    torch.cuda.synchronize()
    assert rc == (FFM_OK if served else FFM_EUNSUP)
    if served:
        assert torch.equal(dqkv2, dqkv) and torch.isfinite(part).all()
    else:                                                            # refused: nothing was launched
        assert torch.isnan(dqkv2.float()).all() and torch.isnan(part).all()
