"""The shapes where a tail tile goes wrong, every output between guard bands (tests/guarded.py).

Each case compares values with float64 exactly as the existing test of the same kernel does (the *_case bodies of
test_kernels_gpu.py / test_conv_gpu.py, or the same formulas at the same tolerances), runs the guard check - no store outside
an output, no element of an output left unwritten - and asserts through the library's host queries which kernel served it, so
that a change in kernel selection cannot quietly turn a case into a duplicate of another.  Scratch whose size a query promises
(ds_part, rowstats, colstats, lgrad partials, sk_part, lora_grad / bn partials) is allocated at exactly that size.
"""
import os

import pytest
import torch

from fairfedmed_amd import _lib as L
from tests import test_conv_gpu as TC
from tests import test_kernels_gpu as TK
from tests.guarded import guard_fixture
from tests.test_kernels_gpu import H16, check, mix, rnd, tol

pytestmark = pytest.mark.gpu

DT = TK.DT
IDS = TK.IDS


@pytest.fixture(scope="module")
def ops():
    from fairfedmed_amd import ops
    return ops


@pytest.fixture
def guard():
    """Every kernel output of this file: poisoned body between two guard bands; unchecked at teardown = failure."""
    yield from guard_fixture()


def qgelu(x):
    return x * torch.sigmoid(1.702 * x)


def qgelu_grad(x):
    s = torch.sigmoid(1.702 * x)
    return s * (1 + 1.702 * x * (1 - s))


# ------------------------------------------------------------ 128 x 128 GEMM (csrc/gemm.hip) ---
SKINNY_FLAGS = (0, L.EPI_BIAS, L.EPI_BIAS | L.EPI_RESIDUAL, L.EPI_BIAS | L.EPI_GELU, L.EPI_DGELU)
EPILOGUES = ["plain", "bias_lora_res", "gelu_out", "gelu_only", "dgelu_aux", "rankop", "colstats", "bnbwd"]


def assert_gemm_route(ops, M, N, K, flags, rank, dt, colstats=False):
    """The skinny kernel up to 64 rows where it has the epilogue (csrc/gemm_skinny.hip: N % 16 == 0, K % 128 == 0, no column
    sums), else the 128 x 128 kernel: never a panel tile without a packed weight."""
    skinny = M <= 64 and N % 16 == 0 and K % 128 == 0 and flags in SKINNY_FLAGS and not colstats
    assert ops.gemm_skinny(M, N, K, flags, dt) == (M <= 64 and N % 16 == 0 and K % 128 == 0 and flags in SKINNY_FLAGS)
    assert ops.gemm_tile_shape(M, N, K, flags, rank, dt, False) == (-1, 128, 128, 8)
    return "skinny" if skinny else "128x128"


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M", [1, 127, 129, 333])
@pytest.mark.parametrize("epi", EPILOGUES)
def test_gemm128_tails(ops, guard, dt, M, epi):
    K, r, G, rps = 128, 8, 3, 50
    for N in (128, 136, 264):
        what = f"{epi} M={M} N={N}"
        a, b = rnd(M, K, dt=dt, seed=3), rnd(N, K, dt=dt, scale=K ** -0.5 * 2, seed=4)
        ab = a.double() @ b.double().t()
        out = guard.out(M, N, dtype=dt, name="out " + what)
        bias = rnd(N, seed=5)
        if epi == "plain":
            route = assert_gemm_route(ops, M, N, K, 0, 0, dt)
            ops.gemm_nt(a, b, out)
            check(out, ab, tol(dt), what)
        elif epi == "bias_lora_res":
            route = assert_gemm_route(ops, M, N, K, L.EPI_BIAS | L.EPI_LORA | L.EPI_RESIDUAL, r, dt)
            ts, lw, res = rnd(M, r, seed=6), rnd(r, N, seed=7), rnd(M, N, dt=dt, seed=8)
            ops.gemm_nt(a, b, out, bias=bias, ts=ts, lw=lw, res=res)
            check(out, ab + bias.double() + ts.double() @ lw.double() + res.double(), tol(dt), what)
        elif epi == "gelu_out":
            route = assert_gemm_route(ops, M, N, K, L.EPI_BIAS | L.EPI_GELU, 0, dt)
            act = guard.out(M, N, dtype=dt, name="gelu_out " + what)
            ops.gemm_nt(a, b, out, bias=bias, gelu_out=act)
            check(out, ab + bias.double(), tol(dt), what + ": pre")
            check(act, qgelu(out.double()), tol(dt), what + ": quick_gelu(pre)")
        elif epi == "gelu_only":
            route = assert_gemm_route(ops, M, N, K, L.EPI_BIAS | L.EPI_GELU | L.EPI_GELU_ONLY, 0, dt)
            assert route == "128x128"
            ops.gemm_nt(a, b, out, bias=bias, gelu_only=True)
            pre, act = guard.out(M, N, dtype=dt, name="pre " + what), guard.out(M, N, dtype=dt, name="act " + what)
            ops.gemm_nt(a, b, pre, bias=bias, gelu_out=act)
            check(out, qgelu(pre.double()), tol(dt), what)
            if route == assert_gemm_route(ops, M, N, K, L.EPI_BIAS | L.EPI_GELU, 0, dt):
                assert torch.equal(out, act), what + ": the activation of the two-output call, bit for bit"
        elif epi == "dgelu_aux":
            route = assert_gemm_route(ops, M, N, K, L.EPI_DGELU, 0, dt)
            aux = rnd(M, N, dt=dt, seed=12)
            ops.gemm_nt(a, b, out, dgelu_aux=aux)
            check(out, ab * qgelu_grad(aux.double()), tol(dt), what)
        elif epi == "rankop":
            route = assert_gemm_route(ops, M, N, K, L.EPI_BIAS | L.EPI_LORA | L.EPI_RANKOP, r, dt)
            P, S, lw, t_fwd = rnd(K, r, scale=0.1, seed=53), rnd(G, r, seed=54), rnd(r, N, seed=55), rnd(M, r, seed=56)
            attr = torch.randint(0, G, ((M + rps - 1) // rps,), device="cuda", dtype=torch.int32)
            rk = torch.zeros(16, K, device="cuda", dtype=dt)
            ops.PackPlan([(P, False, rk)], dt, "cuda").run()
            tiles_m = ops.gemm_tiles_m(M, N, K, L.EPI_BIAS | L.EPI_LORA | L.EPI_RANKOP, r, dt, False)
            assert tiles_m == (M + 127) // 128
            t, ts = guard.out(M, r, name="t " + what), guard.out(M, r, name="ts " + what)
            dsp = guard.out(tiles_m, G, r, name="ds_part " + what)              # exactly the queried size
            ro = ops.RankOp(rk, S, attr, rps, 0.25, 0.7, t_out=t, ts_out=ts, t_fwd=t_fwd, ds_part=dsp)
            ops.gemm_nt(a, b, out, bias=bias, lw=lw, rankop=ro)
            ref_t = a.double() @ P.to(dt).double()
            pi_rows = mix(attr, G)[torch.arange(M, device="cuda") // rps]
            ref_ts = 0.25 * ref_t * (pi_rows @ S.double())
            check(t, ref_t, 2e-5, what + ": t")
            check(ts, ref_ts, 2e-5, what + ": ts")
            check(out, ab + bias.double() + ref_ts @ lw.double(), tol(dt), what + ": fused out")
            check(dsp.double().sum(0), pi_rows.t() @ (0.25 * t_fwd.double() * ref_t), 5e-5, what + ": dS")
        elif epi == "colstats":
            route = assert_gemm_route(ops, M, N, K, 0, 0, dt, colstats=True)
            assert route == "128x128"                                           # (column sums: that kernel's epilogue, at any M)
            tm = (M + 127) // 128
            st = guard.out(tm, 2, N, name="colstats " + what)                   # exactly 2 N ceil(M / 128)
            ops.gemm_nt(a, b, out, colstats=st)
            check(out, ab, tol(dt), what)
            o = out.double()
            for i in range(tm):
                blk = o[i * 128:(i + 1) * 128]
                assert TC.rel(st[i, 0], blk.sum(0)) < 1e-5 and TC.rel(st[i, 1], (blk * blk).sum(0)) < 1e-5, (what, i)
        else:                                                                    # bnbwd, with the masked gradient as a second output
            flags = L.EPI_LORA | L.EPI_LORA_KR | L.EPI_RESIDUAL | L.EPI_BNBWD | L.EPI_RANKOP
            route = assert_gemm_route(ops, M, N, K, flags, r, dt, colstats=True)
            assert route == "128x128"
            x = rnd(M, N, dt=dt, seed=3) * 1.5 + 0.2                            # the BatchNorm's input
            mask = rnd(M, N, dt=dt, seed=13)                                    # its ReLU output (only the sign matters)
            mean, rstd = x.float().mean(0), 1.0 / torch.sqrt(x.float().var(0, unbiased=False) + 1e-5)
            P, S, lw, res = rnd(K, r, scale=0.1, seed=6), rnd(G, r, seed=7), rnd(N, r, seed=8), rnd(M, N, dt=dt, seed=9)
            attr = torch.randint(0, G, ((M + rps - 1) // rps,), device="cuda", dtype=torch.int32)
            rk = torch.zeros(16, K, device="cuda", dtype=dt)
            ops.PackPlan([(P, False, rk)], dt, "cuda").run()
            tm = (M + 127) // 128
            st = guard.out(tm, 2, N, name="bn sums " + what)                    # exactly 2 N ceil(M / 128)
            gout = guard.out(M, N, dtype=dt, name="gout " + what)
            us = guard.out(M, r, name="ts " + what)
            ro = ops.RankOp(rk, S, attr, rps, 0.25, 0.7, ts_out=us)
            ops.gemm_nt(a, b, out, lw=lw, lw_is_kr=True, rankop=ro, res=res, colstats=st, bnbwd=(x, mask, mean, rstd, gout))
            pi_rows = mix(attr, G)[torch.arange(M, device="cuda") // rps]
            ref_ts = 0.25 * (a.double() @ P.to(dt).double()) * (pi_rows @ S.double())
            check(us, ref_ts, 2e-5, what + ": ts")
            check(out, ab + ref_ts @ lw.double().t() + res.double(), tol(dt), what + ": out")
            assert torch.equal(gout, out * (mask > 0)), what + ": the masked gradient"
            g64 = out.double() * (mask.double() > 0)
            xh = (x.double() - mean.double()) * rstd.double()
            for i in range(tm):
                sl = slice(i * 128, (i + 1) * 128)
                assert TC.rel(st[i, 0], g64[sl].sum(0)) < 2e-5 and TC.rel(st[i, 1], (g64[sl] * xh[sl]).sum(0)) < 2e-5, (what, i)
        assert route == ("skinny" if (M == 1 and N == 128 and epi in ("plain", "gelu_out", "dgelu_aux")) else "128x128"), what
        guard.check()


@H16
def test_gemm128_refuses_the_panel_only_epilogues(ops, guard, h16):
    """Row sums of the stored rows (FFM_EPI_ROWSTATS) and the folded LayerNorm (FFM_EPI_LNIN) are epilogues of the panel kernel
    only: at the shapes of this section no kernel serves them - the query says so, the call is refused and writes nothing.  Their
    guarded cases are the panel ones below."""
    M, N, K = 129, 136, 128
    a, b = rnd(M, K, dt=h16, seed=3), rnd(N, K, dt=h16, seed=4)
    for packed in (False, True):
        assert ops.gemm_tiles_n(M, N, K, L.EPI_BIAS | L.EPI_RESIDUAL | L.EPI_ROWSTATS, 0, h16, packed) < 0
        assert ops.gemm_tiles_n(M, N, K, L.EPI_BIAS | L.EPI_LNIN, 0, h16, packed) < 0
    out, part = guard.scratch(M, N, dtype=h16), guard.scratch(2 * M)
    with pytest.raises((RuntimeError, AssertionError)):
        ops.gemm_nt(a, b, out, bias=rnd(N, seed=5), res=rnd(M, N, dt=h16, seed=6), rowstats=part)
    guard.check()
    assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(part).all())


# ------------------------------------------------------------ skinny GEMM (csrc/gemm_skinny.hip) ---
SK_KINDS = ["bf16", "f16", "x3", "x3w16"]


@pytest.mark.parametrize("kind", SK_KINDS)
@pytest.mark.parametrize("M", [1, 33, 48, 64])
@pytest.mark.parametrize("N,K", [(48, 640), (512, 2048)], ids=["3-column-tiles", "split-over-K-shape"])
def test_skinny_tails(ops, guard, kind, M, N, K):
    """References and bounds of test_skinny_gemm_text_tower_shapes / _half / _f32 / _split_over_k (float64 on the operands as
    stored).  N = 512, K = 2048 is split over K across the grid below 64 rows for the X3 kinds: sk_part is allocated at
    exactly ffm_gemm_splitk_floats and guarded."""
    x3 = kind.startswith("x3")
    dt = torch.float32 if x3 else torch.bfloat16 if kind == "bf16" else torch.float16
    g = torch.Generator(device="cuda").manual_seed(M * 1000 + N + K)
    a = torch.randn(M, K, device="cuda", generator=g).to(dt)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.float16 if kind == "x3w16" else dt)
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M, N, device="cuda", generator=g).to(dt)
    aux = torch.randn(M, N, device="cuda", generator=g).to(dt)
    bound = 2e-5 if x3 else 1e-2 if kind == "bf16" else tol(dt)
    need = ops.gemm_splitk_floats(M, N, K, kind == "x3w16") if x3 else 0
    assert need in (0, (K // 128) * M * N)
    if (N, K) == (512, 2048):
        assert (need > 0) == (x3 and M < 64)                           # (the text tower's narrow products; 64 rows fill the grid)
    ab = a.double() @ w.double().t()
    for mode, flags in zip(("plain", "bias", "bias_res", "bias_gelu", "dgelu"), SKINNY_FLAGS):
        what = f"skinny {kind} {mode} M={M} N={N} K={K}"
        assert ops.gemm_skinny(M, N, K, flags, dt, x3=x3, w16=kind == "x3w16"), what + ": not the skinny kernel"
        out = guard.out(M, N, dtype=dt, name="out " + what)
        act = guard.out(M, N, dtype=dt, name="gelu_out " + what) if mode == "bias_gelu" else None
        kw = {"plain": {}, "bias": dict(bias=bias), "bias_res": dict(bias=bias, res=res), "bias_gelu": dict(bias=bias, gelu_out=act),
              "dgelu": dict(dgelu_aux=aux)}[mode]
        if x3:
            kw["x3"] = True
        if need:
            kw["sk_part"] = guard.scratch(need, name="sk_part " + what)          # exactly the queried size
        ops.gemm_nt(a, w, out, **kw)
        ref = ab + (bias.double() if "bias" in mode else 0) + (res.double() if mode == "bias_res" else 0)
        if mode == "dgelu":
            ref = ab * qgelu_grad(aux.double())
        check(out, ref, max(bound, 1e-5) if (x3 and mode == "dgelu") else bound, what)
        if act is not None:
            check(act, qgelu(ref), max(bound, 1e-5) if x3 else bound, what + ": quick_gelu")
        guard.check()


# ------------------------------------------------------------ panel GEMM (csrc/gemm_panel*.h) ---
def panel_rows(ops, N, K, flags, rank, dt, which):
    """M for `which` in {"below", "above", "full"}: k bm - 1 / k bm + 1 with bm the row-tile height the selector uses there
    and k the smallest tile count at which the panel kernel is selected for both, or the bench batch's 6304 rows."""
    if which == "full":
        if ops.gemm_tile_shape(6304, N, K, flags, rank, dt, True)[0] < 0:
            assert "FFM_PANEL_MASK" in os.environ, "the default tile set serves this product on the panel kernel"
            pytest.skip("no panel tile serves this product under this tile mask")
        return 6304
    for lo in range(127, 6304):
        cfg, bm, bn, _ = ops.gemm_tile_shape(lo, N, K, flags, rank, dt, True)
        if cfg < 0 or (lo + 1) % bm:
            continue
        hi = lo + 2
        cfg2, bm2, bn2, _ = ops.gemm_tile_shape(hi, N, K, flags, rank, dt, True)
        if cfg2 >= 0 and (bm2, bn2) == (bm, bn):
            # one more row tile above the edge: the dS partial rows say so
            assert ops.gemm_tiles_m(lo, N, K, flags, rank, dt, True) + N // bn == ops.gemm_tiles_m(hi, N, K, flags, rank, dt, True)
            return lo if which == "below" else hi
    assert "FFM_PANEL_MASK" in os.environ, "the default tile set serves this product on the panel kernel"
    pytest.skip("no panel tile serves this product under this tile mask")


WHICH = ["below", "above", "full"]
FAIRLORA_FLAGS = {"fc_fwd": 1 | 2 | 16, "proj_fwd": 1 | 2 | 8, "proj_dx": 2 | 4 | 32, "fc_dx": 2 | 4, "proj_dx_deriv": 2 | 4 | 32}


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("N,K,mode", [(2048, 1536, "b"), (768, 768, "br"), (768, 2304, ""), (1024, 512, "b")])
@H16
def test_panel_plain_tails(ops, guard, which, N, K, mode, h16):
    flags = (1 if "b" in mode else 0) | (8 if "r" in mode else 0)
    TK.panel_plain_case(ops, guard, panel_rows(ops, N, K, flags, 0, h16, which), N, K, mode, h16)


GEOMS = ["smallest", "engine"]


def fairlora_shape(ops, case, geom, flags, r, dt):
    """(N, K) of a FairLoRA product: the ViT-B/16 block's, or the smallest the selector accepts for the tile configuration the word
    runs on there - K = 512, and N = 1536 = 4 x 384 for the 208 x 384 words (narrower multiples of 384 never reach the 256 tiles
    the selector asks for within 6304 rows), N = 768 for the 160 x 128 words (N = 640 and below are refused)."""
    wide = case in ("fc_fwd", "proj_dx", "proj_dx_deriv", "lgrad")
    engine = (3072, 768) if wide else (768, 3072)
    if geom == "engine":
        return engine
    small = (1536, 512) if wide else (768, 512)
    cfg_e, cfg_s = (ops.gemm_tile_shape(6304, *nk, flags, r, dt, True)[0] for nk in (engine, small))
    if "FFM_PANEL_MASK" not in os.environ:
        assert cfg_s == cfg_e >= 0, "the smallest shape runs on the configuration the word uses in the engine"
        for nk in ((small[0] - 384, 512) if wide else (640, 512), (small[0], 256)):
            assert ops.gemm_tile_shape(6304, *nk, flags, r, dt, True)[0] < 0, f"{nk} is served: no longer the smallest"
    return small


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("case", list(FAIRLORA_FLAGS))
@H16
def test_panel_fairlora_tails(ops, guard, which, geom, case, h16):
    """out, gelu_out / dgelu_aux, t, ts and the dS partials (at exactly ffm_gemm_tiles_m rows) around the last row tile."""
    r, G, rps = 8, 3, 197
    N, K = fairlora_shape(ops, case, geom, FAIRLORA_FLAGS[case] | 64, r, h16)
    M = panel_rows(ops, N, K, FAIRLORA_FLAGS[case] | 64, r, h16, which)
    attr = torch.randint(0, G, ((M + rps - 1) // rps,), device="cuda", dtype=torch.int32)
    TK.panel_fairlora_case(ops, guard, case, M, r, G, attr, rps, h16, shape=(N, K))


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("geom", GEOMS)
@H16
def test_panel_lgrad_tails(ops, guard, which, geom, h16):
    """The FFM_EPI_LGRAD partial products at exactly ffm_gemm_lgrad_rows N r floats each."""
    r, G, rps = 8, 3, 197
    N, K = fairlora_shape(ops, "lgrad", geom, 2 | 4 | 32 | 64 | 512, r, h16)
    if ops.gemm_lgrad_rows(6304, N, K, r, h16, True) <= 0:
        assert "FFM_PANEL_MASK" in os.environ, "the default tile set serves FFM_EPI_LGRAD at the bench shape"
        pytest.skip("no FFM_EPI_LGRAD tile under this tile mask")
    M = panel_rows(ops, N, K, 2 | 4 | 32 | 64 | 512, r, h16, which)
    assert ops.gemm_lgrad_rows(M, N, K, r, h16, True) > 0 or "FFM_PANEL_MASK" in os.environ       # (the helper would skip)
    attr = torch.randint(0, G, ((M + rps - 1) // rps,), device="cuda", dtype=torch.int32)
    TK.panel_lgrad_case(ops, guard, M, r, G, attr, rps, h16, shape=(N, K))


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("which", WHICH)
@H16
def test_panel_layernorm_fold_tails(ops, guard, which, h16):
    """The FFM_EPI_LNB_STAT part at exactly 2 M tiles_n floats, and its consumer FFM_EPI_LNB_APPLY."""
    r, G, rps = 8, 3, 197
    N, K = 3072, 768
    if ops.gemm_tiles_n(6304, N, K, 2 | 4 | 32 | 64 | 512 | 2048, r, h16, True) <= 0 or ops.gemm_tiles_n(6304, K, N, 2 | 4 | 64 | 4096, r, h16, True) <= 0:
        assert "FFM_PANEL_MASK" in os.environ, "the default tile set serves the FFM_EPI_LNB_STAT / FFM_EPI_LNB_APPLY pair at the bench shape"
        pytest.skip("no FFM_EPI_LNB_STAT / FFM_EPI_LNB_APPLY kernel pair under this tile mask")
    # the edge of the consumer's row tiles (N = 768 needs the most rows to reach the panel kernel), and the producer's where the
    # pair is served there too
    rows = [panel_rows(ops, K, N, 2 | 4 | 64 | 4096, r, h16, which)]
    m1 = panel_rows(ops, N, K, 2 | 4 | 32 | 64 | 512 | 2048, r, h16, which)
    if m1 != rows[0] and ops.gemm_tiles_n(m1, K, N, 2 | 4 | 64 | 4096, r, h16, True) > 0 and ops.gemm_lgrad_rows(m1, N, K, r, h16, True) > 0:
        rows.append(m1)
    for M in rows:
        served = (ops.gemm_tiles_n(M, N, K, 2 | 4 | 32 | 64 | 512 | 2048, r, h16, True) > 0 and ops.gemm_lgrad_rows(M, N, K, r, h16, True) > 0
                  and ops.gemm_tiles_n(M, K, N, 2 | 4 | 64 | 4096, r, h16, True) > 0)
        assert served or "FFM_PANEL_MASK" in os.environ, f"M = {M}: the helper would skip under the default tile set"
        attr = torch.randint(0, G, ((M + rps - 1) // rps,), device="cuda", dtype=torch.int32)
        TK.panel_layernorm_backward_fold_case(ops, guard, M, r, G, attr, rps, h16)


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("which", WHICH)
@H16
def test_panel_rowstats_and_layernorm_in_tails(ops, guard, which, h16):
    """FFM_EPI_ROWSTATS at exactly 2 M tiles_n floats; FFM_EPI_LNIN with mean / rstd of exactly M floats."""
    TK.rowstats_case(guard, h16, panel_rows(ops, 768, 768, L.EPI_BIAS | L.EPI_RESIDUAL | L.EPI_ROWSTATS, 0, h16, which))
    TK.layernorm_folded_in_case(guard, 1, h16, panel_rows(ops, 2304, 768, L.EPI_BIAS | L.EPI_LNIN, 0, h16, which))


def panel_lnin_rank_case(ops, guard, kind, M, dt):
    """The FairLoRA products with the LayerNorm in front folded in (FFM_EPI_BIAS | FFM_EPI_LORA [| FFM_EPI_GELU] | FFM_EPI_LNIN with
    FFM_EPI_RANKOP): raw rows x gamma-scaled weight and gamma-scaled rank operand, corrected in the epilogue.  `kind`: "qkv"
    (N = 2304) or "fc" (N = 3072, with the QuickGELU second output).  float64: LayerNorm(x) W^T + b + ts lw with
    t = LayerNorm(x) A on the rank operand as PackPlan rounded it.  Bounds: out as test_gemm_layernorm_folded_in (1.5e-2, 16-bit
    weights and output); mean / rstd as there (1e-4); t and ts are linear in rstd, so its 1e-4 plus the 2e-5 every t / ts check of
    the unfolded products uses."""
    K, r, G, rps = 768, 8, 3, 197
    N = 2304 if kind == "qkv" else 3072
    flags = L.EPI_BIAS | L.EPI_LORA | L.EPI_LNIN | L.EPI_RANKOP | (L.EPI_GELU if kind == "fc" else 0)
    assert ops.gemm_tile_shape(M, N, K, flags, r, dt, True)[0] >= 0, "shape does not select the panel kernel"
    x = rnd(M, K, dt=dt, seed=501) * 1.5 + 0.3
    w = rnd(N, K, scale=K ** -0.5, seed=502)
    gamma, beta, bias = 1 + 0.2 * rnd(K, seed=503), 0.3 * rnd(K, seed=504), rnd(N, seed=505)
    A, S, lw = rnd(K, r, scale=0.1, seed=506), rnd(G, r, seed=507), rnd(r, N, seed=508)
    attr = torch.randint(0, G, ((M + rps - 1) // rps,), device="cuda", dtype=torch.int32)
    wg = (w * gamma).to(dt)
    c = wg.float().sum(1).contiguous()
    d = (w @ beta + bias).contiguous()
    xf = x.float()
    part = torch.stack([xf.sum(1), (xf * xf).sum(1)], 1).unsqueeze(0).contiguous()         # [1, M, 2]: the producer's row sums
    rk, lnrk = torch.zeros(16, K, device="cuda", dtype=dt), torch.zeros(2, 16, device="cuda")
    ops.PackPlan([(A, False, rk, None, (gamma, beta, lnrk))], dt, "cuda").run()
    out = guard.out(M, N, dtype=dt, name="out")
    act = guard.out(M, N, dtype=dt, name="gelu_out") if kind == "fc" else None
    t, ts = guard.out(M, r, name="t"), guard.out(M, r, name="ts")
    mean, rstd = guard.out(M, name="mean"), guard.out(M, name="rstd")                      # exactly M floats each
    ro = ops.RankOp(rk, S, attr, rps, 0.25, 0.7, t_out=t, ts_out=ts)
    ops.gemm_nt(x, wg, out, bias=d, lw=lw, rankop=ro, b_packed=ops.pack_b(wg), gelu_out=act,
                ln_in=ops.LnIn(part, 1, c, mean, rstd, rk=lnrk))
    xd = x.double()
    mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    rs = 1 / torch.sqrt(var + 1e-5)
    h = (xd - mu) * rs * gamma.double() + beta.double()
    rkd = rk[:r].double()                                                                  # gamma (.) A^T as the kernel holds it
    ref_t = rs * (xd @ rkd.t() - mu * rkd.sum(1)) + beta.double() @ A.double()
    pi_rows = mix(attr, G)[torch.arange(M, device="cuda") // rps]
    ref_ts = 0.25 * ref_t * (pi_rows @ S.double())
    ref = h @ w.double().t() + bias.double() + ref_ts.to(dt).double() @ lw.to(dt).double()
    assert float((mean.double() - mu[:, 0]).abs().max()) < 1e-4
    assert float((rstd.double() / rs[:, 0] - 1).abs().max()) < 1e-4
    check(t, ref_t, 1.2e-4, "t through the folded LayerNorm")
    check(ts, ref_ts, 1.2e-4, "ts through the folded LayerNorm")
    check(out, ref, 1.5e-2, "folded LayerNorm -> FairLoRA linear")
    if act is not None:
        check(act, qgelu(out.double()), tol(dt), "quick_gelu(pre)")
    guard.check()


def panel_plain_lnb_apply_case(ops, guard, M, dt, gscale=1.0):
    """FFM_EPI_LNB_APPLY without rank terms (the dX product of the in-projection applying ln_1's backward): out =
    rstd (gamma g_h - c1 / K - xhat c2 / K) + res with g_h = a b^T, c1 / c2 the sums over the np partial rows of `part`
    (include/ffm_hip.h) - float64 on the same operands at the bound of the folded-backward tests, tol(dt).
    gscale multiplies the gradient operands: g, res and the row sums of `part` (tests/test_grad_range_gpu.py)."""
    E, np_ = 768, 4
    assert ops.gemm_tile_shape(M, E, 3 * E, L.EPI_LNB_APPLY, 0, dt, True)[0] >= 0, "shape does not select the panel kernel"
    g, Wt = rnd(M, 3 * E, dt=dt, scale=gscale, seed=601), rnd(E, 3 * E, dt=dt, scale=(3 * E) ** -0.5, seed=602)
    x = rnd(M, E, dt=dt, seed=603) * 1.5 + 0.3
    gamma, res = 1 + 0.1 * rnd(E, seed=604), rnd(M, E, dt=dt, scale=gscale, seed=605)
    xd = x.double()
    mu, rs = xd.mean(1), 1 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)
    part = rnd(np_, M, 2, scale=gscale, seed=606)
    out = guard.out(M, E, dtype=dt, name="out")
    ops.gemm_nt(g, Wt, out, b_packed=ops.pack_b(Wt),
                lnb_apply=ops.LnBwdApply(part, np_, x, gamma, mu.float().contiguous(), rs.float().contiguous(), None, res))
    gh = g.double() @ Wt.double().t()
    c = part.double().sum(0)
    xhat = (xd - mu[:, None]) * rs[:, None]
    ref = rs[:, None] * (gamma.double() * gh - c[:, :1] / E - xhat * c[:, 1:] / E) + res.double()
    check(out, ref, tol(dt), "plain FFM_EPI_LNB_APPLY")
    guard.check()


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("kind", ["qkv", "fc"])
@H16
def test_panel_fairlora_layernorm_in_tails(ops, guard, which, kind, h16):
    """BIAS | LORA | LNIN and BIAS | LORA | GELU | LNIN: out, gelu_out, t, ts, and mean / rstd at exactly M floats."""
    flags = L.EPI_BIAS | L.EPI_LORA | L.EPI_LNIN | L.EPI_RANKOP | (L.EPI_GELU if kind == "fc" else 0)
    panel_lnin_rank_case(ops, guard, kind, panel_rows(ops, 2304 if kind == "qkv" else 3072, 768, flags, 8, h16, which), h16)


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("which", WHICH)
@H16
def test_panel_fairlora_rowstats_tails(ops, guard, which, h16):
    """BIAS | LORA | RESIDUAL | ROWSTATS (c_proj / out_proj forward leaving the next LayerNorm's row sums): the row sums of the
    stored rows at exactly 2 M tiles_n floats beside everything the c_proj forward case holds."""
    r, G, rps, N, K = 8, 3, 197, 768, 3072
    M = panel_rows(ops, N, K, 1 | 2 | 8 | 64 | 128, r, h16, which)
    attr = torch.randint(0, G, ((M + rps - 1) // rps,), device="cuda", dtype=torch.int32)
    TK.panel_fairlora_case(ops, guard, "proj_fwd", M, r, G, attr, rps, h16, rowstats=True)


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("which", WHICH)
@H16
def test_panel_plain_lnb_apply_tails(ops, guard, which, h16):
    panel_plain_lnb_apply_case(ops, guard, panel_rows(ops, 768, 2304, L.EPI_LNB_APPLY, 0, h16, which), h16)


# ------------------------------------------------------------ attention ---
ATTN_LENGTHS = [1, 17, 64, 65, 96, 97, 197, 256, 257, 300]


def expected_attention_route(L_, causal, dt):
    if L_ > 256:
        return "attention_long"
    return "attention3" if (not causal and dt != torch.float32 and L_ >= 65) else "attention"


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("L_", ATTN_LENGTHS)
def test_attention_route_boundaries(ops, guard, dt, causal, L_):
    """One length on each side of every route boundary (64 | 65: attention3 takes over in 16-bit storage; 96 | 97: the floor of
    the LayerNorm row sums; 256 | 257: the streaming kernels), with and without the mask: out, lse, dqkv poisoned and guarded,
    delta (scratch by the header) guarded; bounds of test_attention_fwd_bwd."""
    B, heads = 2, 2
    assert ops.attention_route(L_, causal, dt) == expected_attention_route(L_, causal, dt)
    assert ops.attention_bwd_lnstat_ok(L_, causal, dt) == (expected_attention_route(L_, causal, dt) == "attention3" and L_ >= 97)
    TK.attention_case(ops, guard, dt, B, L_, heads, causal, whole_gradient=L_ == 1)


@H16
@pytest.mark.parametrize("L_", [97, 197, 256])
def test_attention_layernorm_row_sums_part(ops, guard, h16, L_):
    """ln_stat's part at exactly 2 heads x B L x 2 floats, where ffm_attention_bwd_lnstat serves the length."""
    assert ops.attention_route(L_, False, h16) == "attention3" and ops.attention_bwd_lnstat_ok(L_, False, h16)
    TK.attention_lnstat_case(ops, guard, h16, 2, L_, 2)


# ------------------------------------------------------------ row-wise kernels (csrc/rowwise.hip) ---
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("rows", [1, 5, 37])
@pytest.mark.parametrize("width", [128, 2048])
def test_layernorm_few_rows(ops, guard, dt, rows, width):
    TK.layernorm_case(ops, guard, dt, rows, width)                    # mean / rstd: exactly `rows` floats


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("B", [1, 3])
def test_patchify_embed_and_backward(ops, guard, dt, B):
    TK.patchify_and_embed_case(ops, guard, dt, B, rowsums=True)
    TK.embed_lnpre_bwd_case(ops, guard, dt, B, 16, 128)


# ------------------------------------------------------------ LoRA (csrc/lora.hip) ---
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,K,r,G,rps,rk", [(70, 128, 4, 2, 17, False), (1030, 512, 5, 3, 197, True)])
def test_lora_down_tails(ops, guard, dt, M, K, r, G, rps, rk):
    """The VALU kernel (70 rows) and, in 16-bit storage with [r, K] rows from 1024 rows on, the matrix-core kernel with a ragged
    last 16-row block; ds_part at exactly ffm_lora_down_blocks rows."""
    mfma = dt != torch.float32 and rk and M >= 1024
    assert (ops.lora_down_blocks(M, K, r, dt) == (M + 15) // 16) == mfma
    TK.lora_down_case(ops, guard, dt, M, K, r, G, rps, rk, True)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,K,r", [(64, 128, 4), (130, 264, 32)])
def test_lora_grad_and_reductions(ops, guard, dt, M, K, r):
    """One row group of LG_ROWS = 128 rows, and two with a ragged second: `part` at exactly ffm_lora_grad_splits; the reduction
    plain, transposed, accumulating and through ReducePlan."""
    assert ops.lora_grad_splits(M) == (M + 127) // 128
    TK.lora_grad_case(ops, guard, dt, M, K, r)


@H16
@pytest.mark.parametrize("M", [130, 1000])
def test_lora_grad_through_layernorm_tails(guard, h16, M):
    TK.lora_grad_partial_ln_case(guard, h16, M)


# ------------------------------------------------------------ conv (csrc/conv.hip) ---
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("H,W", [(7, 7), (8, 12)])
@pytest.mark.parametrize("stride", [1, 2])
def test_im2col_col2im_small_maps(ops, guard, dt, H, W, stride):
    TC.im2col_case(ops, guard, dt, 2, H, W, 32, 64, stride)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("B,H,W,C,Co", [(1, 7, 7, 128, 64), (2, 8, 12, 32, 32)])
def test_implicit_conv_small_maps(ops, guard, dt, B, H, W, C, Co):
    # which launch geometry serves the map (ffm_conv3x3_colstat_rows describes it): one launch without scratch - a partial row
    # per 128-row tile - and, with the scratch the case passes, that or the split over K (a partial row per 8 rows)
    kq = 64 if dt != torch.float32 else 32
    Kp, M = (9 * C + kq - 1) // kq * kq, B * H * W
    q = lambda nsc: L.load().ffm_conv3x3_colstat_rows(B, H, W, C, Co, Kp, nsc, L.dtype_code(dt))
    assert q(0) == (M + 127) // 128
    split = (H, W, C) == (7, 7, 128)                                    # one tile and K = 1152: split over K; 8 x 12 x 32: not
    assert q(8 * M * max(C, Co)) == ((M + 7) // 8 if split else (M + 127) // 128)
    TC.implicit_conv_case(ops, guard, dt, B, H, W, C, Co)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("rows", [147, 7169])
@pytest.mark.parametrize("C", [24, 200])
def test_batchnorm_ragged(ops, guard, dt, rows, C):
    """A strip narrower than 64 channels / a ragged last strip, one row past a block of rows; `part` at exactly ffm_bn_blocks."""
    assert 1 <= ops.bn_blocks(147) < ops.bn_blocks(7169)                # (more than one block of rows at the larger map)
    TC.batchnorm_case(ops, guard, dt, rows, C, True, True)


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_pool_add_relu_and_tokens_of_a_7x7_map(ops, guard, dt):
    TC.pool_add_relu_tokens_case(ops, guard, dt, 49)


# ------------------------------------------------------------ text ends (csrc/text.hip) ---
@pytest.mark.parametrize("use_ot", [False, True], ids=["mean-over-prompts", "per-prompt"])
@pytest.mark.parametrize("N,n_cls,n_ctx,TL,w,D", [(2, 2, 4, 10, 512, 512), (3, 2, 2, 7, 128, 192)])
def test_text_tower_ends(ops, guard, use_ot, N, n_cls, n_ctx, TL, w, D):
    TK.text_tower_ends_case(ops, guard, use_ot, N, n_cls, n_ctx, TL, w, D)


# ------------------------------------------------------------ logits head (csrc/head.hip) ---
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("B,L_,D,n_cls,S", [(1, 2, 1024, 8, 1), (3, 50, 1024, 3, 1), (4, 17, 192, 5, 2), (8, 197, 768, 2, 1)])
def test_head_shapes_the_kernel_promises(ops, guard, dt, B, L_, D, n_cls, S):
    """D up to 1024 (RN50), up to 8 classes, one patch token, token counts that do not fill the 16 waves x 4 blocks."""
    assert D <= 1024 and D % 4 == 0 and n_cls <= 8 and B % S == 0
    TK.head_and_loss_case(ops, guard, dt, B, L_, D, S, n_cls=n_cls)


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_head_all_zero_token_row(ops, guard, dt):
    """F.normalize's 1e-12 clamp, forward and backward: one patch token of one image is all zero."""
    TK.head_and_loss_case(ops, guard, dt, 4, 17, 192, 2, n_cls=5, zero_row=1 * 17 + 3)
