"""Operands behind a row stride wider than their rows: every kernel family that takes lda / ldb / ldc / ldx.

The RN50 attention pool writes its q, k and v projections into the column thirds of one [rows, 3E] buffer (ldc = 3E) and its
backward reads the thirds of dqkv as A (lda = 3E) and as the x of the rank-r reductions; no other test passes a stride that
differs from the row width.  Every case here runs ONE call twice on the same data:

  * once with the strided operands as windows (tests/guarded.py): outputs as `guard.window` - a poisoned [rows, ld] body whose
    part outside the window is frozen -, inputs as `guard.window_in` - the source surrounded by NaN;
  * once with contiguous copies into `guard.out`,

and asserts (a) torch.equal(window result, contiguous result) for every output - the stride changes addresses only: the host
code picks the kernel from M, N, K and the flags, and the order of every reduction is fixed -, (b) the contiguous result
against float64 at the tolerance of the existing test of that kernel, (c) guard.check(): gaps bit for bit intact, windows fully
written, bands intact.  A NaN that a load outside an input window brought in fails (a).

Two layouts: "thirds" (ld = 3 width, col0 = 0 / width / 2 width: the engine's; every third in a fresh buffer, so that a spill
into a neighbouring third is not overwritten by the launch that owns it) and "tight" (ld = width + 8, col0 = 8: the smallest
gap a 16-byte row stride allows in every dtype - one vector store or load one lane too wide lands in it).

Every case names, from the library's host queries, the kernel that served it.
"""
import os
import subprocess
import sys

import pytest
import torch

from fairfedmed_amd import _lib as L
from tests import test_conv_gpu as TC
from tests import test_guard_bands_gpu as TG
from tests.guarded import guard_fixture
from tests.test_guard_bands_gpu import SKINNY_FLAGS, assert_gemm_route, qgelu, qgelu_grad
from tests.test_kernels_gpu import DT, H16, IDS, check, mix, rnd, tol

pytestmark = pytest.mark.gpu

LAYOUTS = {"first-third": lambda w: (3 * w, 0), "middle-third": lambda w: (3 * w, w), "last-third": lambda w: (3 * w, 2 * w),
           "tight": lambda w: (w + 8, 8)}


@pytest.fixture(scope="module")
def ops():
    from fairfedmed_amd import ops
    return ops


@pytest.fixture
def guard():
    """Every kernel output of this file: poisoned body (or window) between two guard bands; unchecked at teardown = failure."""
    yield from guard_fixture()


class Place:
    """Where one run's operands live.  `win`: the roles behind a stride in this run ("a", "b", "c" - c: the output and every
    [M, N] side tensor, which share ldc; "x": the activation of a LoRA call), in `layout`; every other operand is contiguous."""

    def __init__(self, guard, layout=None, win=""):
        self.g, self.layout, self.win = guard, layout, win
        self.tag = f"{'+'.join(win)} in {layout}" if win else "contiguous"

    def out(self, role, rows, cols, dt, name):
        if role in self.win:
            ld, col0 = LAYOUTS[self.layout](cols)
            return self.g.window(rows, ld, col0, cols, dtype=dt, name=f"{name} [{self.tag}]")
        return self.g.out(rows, cols, dtype=dt, name=f"{name} [{self.tag}]")

    def inp(self, role, src):
        if role in self.win:
            ld, col0 = LAYOUTS[self.layout](src.shape[1])
            v = self.g.window_in(src.shape[0], ld, col0, src)
            assert v.stride() == (ld, 1) and v.data_ptr() % 16 == 0
            return v
        return src


def same(win, ref, what):
    """(a): every output of the windowed run, bit for bit what the contiguous run left."""
    assert win.keys() == ref.keys()
    for k in ref:
        assert win[k].shape == ref[k].shape and torch.equal(win[k], ref[k]), \
            f"{what}: '{k}' differs from the contiguous run in {int((win[k] != ref[k]).sum())} element(s) " \
            f"({int(torch.isnan(win[k].float()).sum())} NaN in the windowed result)"


# ------------------------------------------------------------ 128 x 128 GEMM (csrc/gemm.hip) ---
def gemm128_data(ops, epi, dt, M, N, K):
    """The operands of one epilogue of test_guard_bands_gpu.EPILOGUES, contiguous, and the flags / rank of the call."""
    r, G, rps = 8, 3, 50
    d = dict(a=rnd(M, K, dt=dt, seed=3), b=rnd(N, K, dt=dt, scale=K ** -0.5 * 2, seed=4), bias=rnd(N, seed=5), r=r, G=G, rps=rps)
    flags = {"plain": 0, "bias_lora_res": L.EPI_BIAS | L.EPI_LORA | L.EPI_RESIDUAL, "gelu_out": L.EPI_BIAS | L.EPI_GELU,
             "gelu_only": L.EPI_BIAS | L.EPI_GELU | L.EPI_GELU_ONLY, "dgelu_aux": L.EPI_DGELU,
             "rankop": L.EPI_BIAS | L.EPI_LORA | L.EPI_RANKOP, "colstats": 0,
             "bnbwd": L.EPI_LORA | L.EPI_LORA_KR | L.EPI_RESIDUAL | L.EPI_BNBWD | L.EPI_RANKOP}[epi]
    d["flags"], d["rank"] = flags, r if flags & L.EPI_LORA else 0
    if epi == "bias_lora_res":
        d.update(ts=rnd(M, r, seed=6), lw=rnd(r, N, seed=7), res=rnd(M, N, dt=dt, seed=8))
    elif epi == "dgelu_aux":
        d["aux"] = rnd(M, N, dt=dt, seed=12)
    elif epi in ("rankop", "bnbwd"):
        d["attr"] = torch.randint(0, G, ((M + rps - 1) // rps,), device="cuda", dtype=torch.int32)
        d["rk"] = torch.zeros(16, K, device="cuda", dtype=dt)
        if epi == "rankop":
            d.update(P=rnd(K, r, scale=0.1, seed=53), S=rnd(G, r, seed=54), lw=rnd(r, N, seed=55), t_fwd=rnd(M, r, seed=56))
        else:
            x = rnd(M, N, dt=dt, seed=3) * 1.5 + 0.2                            # the BatchNorm's input
            d.update(x=x, mask=rnd(M, N, dt=dt, seed=13), mean=x.float().mean(0),
                     rstd=1.0 / torch.sqrt(x.float().var(0, unbiased=False) + 1e-5),
                     P=rnd(K, r, scale=0.1, seed=6), S=rnd(G, r, seed=7), lw=rnd(N, r, seed=8), res=rnd(M, N, dt=dt, seed=9))
        ops.PackPlan([(d["P"], False, d["rk"])], dt, "cuda").run()
    return d


def gemm128_run(ops, pl, epi, dt, d):
    """One ffm_gemm_nt call with its operands where `pl` puts them; every output of the call by name."""
    M, K = d["a"].shape
    N, r, G, g = d["b"].shape[0], d["r"], d["G"], pl.g
    a, b = pl.inp("a", d["a"]), pl.inp("b", d["b"])
    out = pl.out("c", M, N, dt, "out")
    side = lambda name: pl.inp("c", d[name])
    tm = (M + 127) // 128
    o = dict(out=out)
    if epi == "plain":
        ops.gemm_nt(a, b, out)
    elif epi == "bias_lora_res":
        ops.gemm_nt(a, b, out, bias=d["bias"], ts=d["ts"], lw=d["lw"], res=side("res"))
    elif epi == "gelu_out":
        o["gelu_out"] = pl.out("c", M, N, dt, "gelu_out")
        ops.gemm_nt(a, b, out, bias=d["bias"], gelu_out=o["gelu_out"])
    elif epi == "gelu_only":
        ops.gemm_nt(a, b, out, bias=d["bias"], gelu_only=True)
    elif epi == "dgelu_aux":
        ops.gemm_nt(a, b, out, dgelu_aux=side("aux"))
    elif epi == "rankop":
        o.update(t=g.out(M, r, name=f"t [{pl.tag}]"), ts=g.out(M, r, name=f"ts [{pl.tag}]"),
                 ds_part=g.out(tm, G, r, name=f"ds_part [{pl.tag}]"))
        ro = ops.RankOp(d["rk"], d["S"], d["attr"], d["rps"], 0.25, 0.7, t_out=o["t"], ts_out=o["ts"], t_fwd=d["t_fwd"], ds_part=o["ds_part"])
        ops.gemm_nt(a, b, out, bias=d["bias"], lw=d["lw"], rankop=ro)
    elif epi == "colstats":
        o["colstats"] = g.out(tm, 2, N, name=f"colstats [{pl.tag}]")
        ops.gemm_nt(a, b, out, colstats=o["colstats"])
    else:
        o.update(colstats=g.out(tm, 2, N, name=f"bn sums [{pl.tag}]"), gout=pl.out("c", M, N, dt, "gout"),
                 ts=g.out(M, r, name=f"ts [{pl.tag}]"))
        ro = ops.RankOp(d["rk"], d["S"], d["attr"], d["rps"], 0.25, 0.7, ts_out=o["ts"])
        ops.gemm_nt(a, b, out, lw=d["lw"], lw_is_kr=True, rankop=ro, res=side("res"), colstats=o["colstats"],
                    bnbwd=(side("x"), side("mask"), d["mean"], d["rstd"], o["gout"]))
    return o


def gemm128_check(epi, dt, d, o, what):
    """(b): the contiguous run against float64 - the formulas and bounds of test_gemm128_tails."""
    M, N, r, G, rps = d["a"].shape[0], d["b"].shape[0], d["r"], d["G"], d["rps"]
    a, bias, out = d["a"], d["bias"], o["out"]
    ab = a.double() @ d["b"].double().t()
    tm = (M + 127) // 128
    if epi == "plain":
        check(out, ab, tol(dt), what)
    elif epi == "bias_lora_res":
        check(out, ab + bias.double() + d["ts"].double() @ d["lw"].double() + d["res"].double(), tol(dt), what)
    elif epi == "gelu_out":
        check(out, ab + bias.double(), tol(dt), what + ": pre")
        check(o["gelu_out"], qgelu(out.double()), tol(dt), what + ": quick_gelu(pre)")
    elif epi == "gelu_only":
        check(out, qgelu(ab + bias.double()), tol(dt), what)       # (test_gemm128_tails holds it bit for bit against the two-output call)
    elif epi == "dgelu_aux":
        check(out, ab * qgelu_grad(d["aux"].double()), tol(dt), what)
    elif epi == "rankop":
        ref_t = a.double() @ d["P"].to(dt).double()
        pi_rows = mix(d["attr"], G)[torch.arange(M, device="cuda") // rps]
        ref_ts = 0.25 * ref_t * (pi_rows @ d["S"].double())
        check(o["t"], ref_t, 2e-5, what + ": t")
        check(o["ts"], ref_ts, 2e-5, what + ": ts")
        check(out, ab + bias.double() + ref_ts @ d["lw"].double(), tol(dt), what + ": fused out")
        check(o["ds_part"].double().sum(0), pi_rows.t() @ (0.25 * d["t_fwd"].double() * ref_t), 5e-5, what + ": dS")
    elif epi == "colstats":
        check(out, ab, tol(dt), what)
        od, st = out.double(), o["colstats"]
        for i in range(tm):
            blk = od[i * 128:(i + 1) * 128]
            assert TC.rel(st[i, 0], blk.sum(0)) < 1e-5 and TC.rel(st[i, 1], (blk * blk).sum(0)) < 1e-5, (what, i)
    else:
        pi_rows = mix(d["attr"], G)[torch.arange(M, device="cuda") // rps]
        ref_ts = 0.25 * (a.double() @ d["P"].to(dt).double()) * (pi_rows @ d["S"].double())
        check(o["ts"], ref_ts, 2e-5, what + ": ts")
        check(out, ab + ref_ts @ d["lw"].double().t() + d["res"].double(), tol(dt), what + ": out")
        assert torch.equal(o["gout"], out * (d["mask"] > 0)), what + ": the masked gradient"
        g64 = out.double() * (d["mask"].double() > 0)
        xh = (d["x"].double() - d["mean"].double()) * d["rstd"].double()
        st = o["colstats"]
        for i in range(tm):
            sl = slice(i * 128, (i + 1) * 128)
            assert TC.rel(st[i, 0], g64[sl].sum(0)) < 2e-5 and TC.rel(st[i, 1], (g64[sl] * xh[sl]).sum(0)) < 2e-5, (what, i)


def gemm128_case(ops, guard, epi, dt, M, N, K, wins=("c", "a", "b", "abc"), layouts=tuple(LAYOUTS)):
    d = gemm128_data(ops, epi, dt, M, N, K)
    route = assert_gemm_route(ops, M, N, K, d["flags"], d["rank"], dt, colstats=epi in ("colstats", "bnbwd"))
    assert route == "128x128", "more than 64 rows: csrc/gemm.hip's 128 x 128 kernel, never the skinny one"
    what = f"{epi} M={M} N={N} K={K}"
    ref = gemm128_run(ops, Place(guard), epi, dt, d)
    gemm128_check(epi, dt, d, ref, what)
    for win in wins:
        for layout in layouts:
            pl = Place(guard, layout, win)
            same(gemm128_run(ops, pl, epi, dt, d), ref, f"{what}, {pl.tag}")
    guard.check()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("epi", TG.EPILOGUES)
def test_gemm128_two_buffer_loop(ops, guard, dt, epi):
    """gemm_nt_kernel<..., NST = 2> (csrc/gemm.hip), the host queries say: no panel tile, not the skinny kernel; K 2 / 128 = 3 < 6
    keeps the 16-bit types off the four-stage ring.  M = 200: a ragged second row tile; N = 264: two full column tiles and one of
    8 columns.  `out` (with every [M, N] side tensor: res, gelu_out, dgelu_aux, bnbwd's x / mask / gout), A, B, and all three at
    once behind a stride."""
    M, N, K = 200, 264, 192
    assert K * 2 // 128 < 6
    gemm128_case(ops, guard, epi, dt, M, N, K)


def ring_qualifies(M, N, K, dt):
    """The selection rule of ffm_gemm_nt (csrc/gemm.hip, `deep`): 16-bit storage, at most 256 tiles of 128 x 128, at least six
    128-byte K steps - and the switch FFM_GEMM_DEEP, which the caller reads."""
    return dt != torch.float32 and ((M + 127) // 128) * ((N + 127) // 128) <= 256 and K * 2 // 128 >= 6


@H16
@pytest.mark.parametrize("epi", ["plain", "bias_lora_res"])
def test_gemm128_four_stage_ring(ops, guard, h16, epi):
    """gemm_nt_kernel<..., NST = 4>: 6 tiles, K 2 / 128 = 8 steps.  With FFM_GEMM_DEEP=0 in the environment (the child process of
    the test below) the same shapes and data run the two-buffer loop."""
    M, N, K = 200, 264, 512
    assert ring_qualifies(M, N, K, h16) and not ring_qualifies(M, N, 192, h16)
    assert ops.switch("FFM_GEMM_DEEP") == (0 if os.environ.get("FFM_GEMM_DEEP") == "0" else 1)
    gemm128_case(ops, guard, epi, h16, M, N, K)


def test_gemm128_ring_shapes_on_the_two_buffer_loop(ops):
    """FFM_GEMM_DEEP=0 (read once per process): the ring cases again in a child process, on the two-buffer loop."""
    assert ops.switch("FFM_GEMM_DEEP") == 1 or os.environ.get("FFM_GEMM_DEEP") == "0"
    env = dict(os.environ, FFM_GEMM_DEEP="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", os.path.join(root, "tests", "test_strided_gpu.py"), "-k",
                        "four_stage_ring"], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "4 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("epi", ["plain", "bias_lora_res", "gelu_out"])
def test_gemm128_narrow_output(ops, guard, dt, epi):
    """M = 300, N = 64, K = 128 with ldc = 192 (and the tight 72).  ffm_gemm_tile_shape reports (-1, 128, 128, 8): ffm_gemm_nt
    runs this on the 128 x 128 kernel with half of its one column tile masked off - the 128 x N narrow kernel of csrc/gemm.hip
    serves the convolutions only (ffm_conv3x3_nhwc, whose ABI has no stride)."""
    M, N, K = 300, 64, 128
    assert ops.gemm_tile_shape(M, N, K, 0, 0, dt, False) == (-1, 128, 128, 8)
    assert LAYOUTS["middle-third"](N) == (192, 64)
    gemm128_case(ops, guard, epi, dt, M, N, K, wins=("c", "abc"))


# ------------------------------------------------------------ the attention pool as engine_rn.py calls it ---
@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_attention_pool_forward_thirds(ops, guard, dt):
    """q, k, v = tok W^T + b + ts B into the thirds of one [150, 768] layout (RNEngine._vision_forward): FFM_EPI_BIAS | LORA with
    the rank operand (G = 1, attr None, rank 8) - the 128 x 128 kernel on its two-buffer loop (K 2 / 128 = 4 steps: below the
    ring's six; the ring with this epilogue on strided outputs: test_gemm128_four_stage_ring).  Each third in its own fresh
    buffer: a spill into a neighbour stays visible."""
    E, rows, r = 256, 150, 8
    flags = L.EPI_BIAS | L.EPI_LORA | L.EPI_RANKOP
    assert assert_gemm_route(ops, rows, E, E, flags, r, dt) == "128x128"
    assert not ring_qualifies(rows, E, E, dt)
    tok = rnd(rows, E, dt=dt, seed=201)
    ab, t_ref = {}, {}
    for i, n in enumerate("qkv"):
        W, bias = rnd(E, E, dt=dt, scale=E ** -0.5, seed=202 + i), rnd(E, seed=205 + i)
        A, S, B = rnd(E, r, scale=0.1, seed=208 + i), rnd(1, r, seed=211 + i), rnd(r, E, seed=214 + i)
        rk = torch.zeros(16, E, device="cuda", dtype=dt)
        ops.PackPlan([(A, False, rk)], dt, "cuda").run()
        got = []
        for pl in (Place(guard), Place(guard, ("first-third", "middle-third", "last-third")[i], "c"), Place(guard, "tight", "c")):
            o = dict(out=pl.out("c", rows, E, dt, f"{n}"), t=guard.out(rows, r, name=f"t {n} [{pl.tag}]"),
                     ts=guard.out(rows, r, name=f"ts {n} [{pl.tag}]"))
            ops.gemm_nt(tok, W, o["out"], bias=bias, lw=B, rankop=ops.RankOp(rk, S, None, 50, 0.25, 0.7, t_out=o["t"], ts_out=o["ts"]))
            got.append(o)
        ref_t = tok.double() @ A.to(dt).double()
        ref_ts = 0.25 * ref_t * S.double()                             # (G = 1: the mix is 1)
        check(got[0]["t"], ref_t, 2e-5, n + ": t")
        check(got[0]["ts"], ref_ts, 2e-5, n + ": ts")
        check(got[0]["out"], tok.double() @ W.double().t() + bias.double() + ref_ts @ B.double(), tol(dt), n + ": out")
        same(got[1], got[0], f"{n}: its third of [150, 768]")
        same(got[2], got[0], f"{n}: tight")
        if i == 1:
            assert LAYOUTS["middle-third"](E) == (768, 256) and got[1]["out"].stride() == (768, 1)
    guard.check()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("r", [8, 32])
def test_attention_pool_backward_thirds(ops, guard, dt, r):
    """dtok = sum over q, k, v of dqkv[:, third] W + us A^T (RNEngine._vision_backward): A is a third of a NaN-gapped [150, 768]
    buffer, the output contiguous, `res` the previous output.  Rank 8: FFM_EPI_LORA | LORA_KR | RESIDUAL with the rank operand
    (us out of the GEMM), the 128 x 128 kernel on its two-buffer loop.  Rank 32: ffm_lora_down on the strided slice (the VALU
    kernel, two passes over the rank), then the `ts=` form on the generic-flag 128 x 128 kernel (rank > 16)."""
    E, rows = 256, 150
    flags = L.EPI_LORA | L.EPI_LORA_KR | L.EPI_RESIDUAL | (L.EPI_RANKOP if r <= 16 else 0)
    assert assert_gemm_route(ops, rows, E, E, flags, r, dt) == "128x128"
    assert rows < 1024, "ffm_lora_down's matrix-core kernel starts at 1024 rows (down_mfma_ok, csrc/lora.hip)"
    dqkv = rnd(rows, 3 * E, dt=dt, seed=221)
    runs = {}
    for mode in ("contiguous", "thirds", "tight"):
        acc, outs = None, {}
        for i, n in enumerate("qkv"):
            g_src = dqkv[:, i * E:(i + 1) * E].contiguous()
            if mode == "thirds":                                       # one third live per buffer: the other two stay NaN
                buf = torch.full_like(dqkv, float("nan"))
                buf[:, i * E:(i + 1) * E] = g_src
                g = buf[:, i * E:(i + 1) * E]
                assert g.stride() == (3 * E, 1)
            else:
                g = Place(guard, "tight", "a" if mode == "tight" else "").inp("a", g_src)
            Wt = rnd(E, E, dt=dt, scale=E ** -0.5, seed=222 + i)
            A, S, B = rnd(E, r, scale=0.1, seed=225 + i), rnd(1, r, seed=228 + i), rnd(r, E, scale=0.1, seed=231 + i)
            dst = guard.out(rows, E, dtype=dt, name=f"dtok after {n} [{mode}]")
            us = guard.out(rows, r, name=f"us {n} [{mode}]")
            kw = dict(res=acc) if acc is not None else {}
            if r <= 16:
                rk = torch.zeros(16, E, device="cuda", dtype=dt)
                ops.PackPlan([(B, True, rk)], dt, "cuda").run()
                ops.gemm_nt(g, Wt, dst, lw=A, lw_is_kr=True, rankop=ops.RankOp(rk, S, None, 50, 0.25, 0.7, ts_out=us), **kw)
            else:
                u = guard.out(rows, r, name=f"u {n} [{mode}]")
                ops.lora_down(g, B, True, S, None, r, 1, 50, 0.25, 0.7, u, us)
                ops.gemm_nt(g, Wt, dst, ts=us, lw=A, lw_is_kr=True, **kw)
                outs["u" + n] = u
            outs["us" + n], outs["dtok" + n] = us, dst
            if mode == "contiguous":
                ref_us = 0.25 * (g_src.double() @ B.to(dt).double().t()) * S.double()
                ref = g_src.double() @ Wt.double().t() + ref_us @ A.double().t() + (acc.double() if acc is not None else 0)
                check(us, ref_us, 2e-5, f"{n}: us")
                check(dst, ref, tol(dt), f"{n}: dtok")
            acc = dst
        runs[mode] = outs
    same(runs["thirds"], runs["contiguous"], "A = dqkv[:, third]")
    same(runs["tight"], runs["contiguous"], "A tight")
    guard.check()


# ------------------------------------------------------------ skinny GEMM (csrc/gemm_skinny.hip) ---
@pytest.mark.parametrize("kind,M,N,K", [("bf16", 33, 48, 640), ("f16", 33, 48, 640), ("f32", 40, 512, 512), ("x3", 40, 512, 512),
                                        ("x3w16", 40, 512, 512), ("x3", 40, 512, 2048), ("x3w16", 40, 512, 2048)])
def test_skinny_strided(ops, guard, kind, M, N, K):
    """gemm_skinny_kernel on 4 waves (K = 640: not a multiple of 256) in 16-bit storage; at (40, 512, 512) the exact float32
    kernel on 8 waves and, for the split-operand kinds, gemm_skinny_nt_kernel (several column tiles per block); at
    (40, 512, 2048) with sk_part of exactly ffm_gemm_splitk_floats the products split over K and skinny_splitk_finish_kernel,
    whose epilogue indexes out / res / aux / gelu_out with ldc.  A, the weight and every [M, N] tensor behind a stride at once;
    references and bounds of test_skinny_tails / test_skinny_gemm_f32."""
    x3 = kind.startswith("x3")
    dt = torch.bfloat16 if kind == "bf16" else torch.float16 if kind == "f16" else torch.float32
    g = torch.Generator(device="cuda").manual_seed(M * 1000 + N + K)
    a = torch.randn(M, K, device="cuda", generator=g).to(dt)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.float16 if kind == "x3w16" else dt)
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M, N, device="cuda", generator=g).to(dt)
    aux = torch.randn(M, N, device="cuda", generator=g).to(dt)
    bound = 2e-5 if x3 else 2e-6 if kind == "f32" else 1e-2 if kind == "bf16" else tol(dt)
    # (without sk_part a split-operand product runs as one launch - ffm_skinny_launch -: the K = 512 cases)
    need = ops.gemm_splitk_floats(M, N, K, kind == "x3w16") if (x3 and K == 2048) else 0
    assert need == ((K // 128) * M * N if (x3 and K == 2048) else 0), "K = 2048: split over K into 16 slices"
    ab = a.double() @ w.double().t()

    def run(pl, mode, what):
        o = dict(out=pl.out("c", M, N, dt, "out " + what))
        if mode == "bias_gelu":
            o["gelu_out"] = pl.out("c", M, N, dt, "gelu_out " + what)
        kw = {"plain": {}, "bias": dict(bias=bias), "bias_res": dict(bias=bias, res=pl.inp("c", res)),
              "bias_gelu": dict(bias=bias, gelu_out=o.get("gelu_out")), "dgelu": dict(dgelu_aux=pl.inp("c", aux))}[mode]
        if x3:
            kw["x3"] = True
        if need:
            kw["sk_part"] = guard.scratch(need, name=f"sk_part {what} [{pl.tag}]")      # exactly the queried size
        ops.gemm_nt(pl.inp("a", a), pl.inp("b", w), o["out"], **kw)
        return o

    for mode, flags in zip(("plain", "bias", "bias_res", "bias_gelu", "dgelu"), SKINNY_FLAGS):
        what = f"skinny {kind} {mode} M={M} N={N} K={K}"
        assert ops.gemm_skinny(M, N, K, flags, dt, x3=x3, w16=kind == "x3w16"), what + ": not the skinny kernel"
        o = run(Place(guard), mode, what)
        ref = ab + (bias.double() if "bias" in mode else 0) + (res.double() if mode == "bias_res" else 0)
        if mode == "dgelu":
            ref = ab * qgelu_grad(aux.double())
        loose = max(bound, 1e-5) if dt == torch.float32 else bound
        check(o["out"], ref, loose if mode == "dgelu" else bound, what)
        if mode == "bias_gelu":
            check(o["gelu_out"], qgelu(ref), loose, what + ": quick_gelu")
        for layout in LAYOUTS:
            pl = Place(guard, layout, "abc")
            same(run(pl, mode, what), o, f"{what}, {pl.tag}")
    guard.check()


# ------------------------------------------------------------ panel GEMM (csrc/gemm_panel*.h) and ffm_pack_b ---
@pytest.mark.mask_tolerant
@H16
def test_panel_plain_strided(ops, guard, h16):
    """M = 6304, N = K = 768, bias + residual on a packed weight: the panel kernel (the tile ffm_gemm_tile_shape names; skipped
    where a tile mask leaves none, as panel_rows does).  `out` and `res`: the middle third of [6304, 2304] buffers; A: tight."""
    N = K = 768
    flags = L.EPI_BIAS | L.EPI_RESIDUAL
    M = TG.panel_rows(ops, N, K, flags, 0, h16, "full")
    assert ops.gemm_tile_shape(M, N, K, flags, 0, h16, True)[0] >= 0
    assert ops.gemm_tiles_m(M, N, K, flags, 0, h16, True) != ops.gemm_tiles_m(M, N, K, flags, 0, h16, False), "not the panel kernel"
    a, b = rnd(M, K, dt=h16, seed=60), rnd(N, K, dt=h16, scale=K ** -0.5, seed=61)
    bias, res = rnd(N, seed=62), rnd(M, N, dt=h16, seed=63)
    bp = ops.pack_b(b)
    out = guard.out(M, N, dtype=h16, name="out [contiguous]")
    ops.gemm_nt(a, b, out, b_packed=bp, bias=bias, res=res)
    check(out, a.double() @ b.double().t() + bias.double() + res.double(), tol(h16), "panel br")
    c, at = Place(guard, "middle-third", "c"), Place(guard, "tight", "a")
    outw = c.out("c", M, N, h16, "out")
    assert outw.stride() == (2304, 1)
    ops.gemm_nt(at.inp("a", a), b, outw, b_packed=bp, bias=bias, res=c.inp("c", res))
    same(dict(out=outw), dict(out=out), "panel br: out / res in the middle third, A tight")
    guard.check()


@pytest.mark.mask_tolerant
@H16
def test_panel_fairlora_strided(ops, guard, h16):
    """The c_proj-forward word (FFM_EPI_BIAS | LORA | RESIDUAL with the rank operand) on the same layout: the FairLoRA panel
    tile of gemm_panel_rk*.hip; t and ts have no stride.  References of panel_fairlora_case."""
    N = K = 768
    r, G, rps = 8, 3, 197
    flags = TG.FAIRLORA_FLAGS["proj_fwd"] | 64
    M = TG.panel_rows(ops, N, K, flags, r, h16, "full")
    assert ops.gemm_tile_shape(M, N, K, flags, r, h16, True)[0] >= 0
    a, b = rnd(M, K, dt=h16, seed=70), rnd(N, K, dt=h16, scale=K ** -0.5, seed=71)
    P, S, lw = rnd(K, r, scale=0.1, seed=73), rnd(G, r, seed=74), rnd(r, N, seed=75)
    bias, res = rnd(N, seed=72), rnd(M, N, dt=h16, seed=77)
    attr = torch.randint(0, G, ((M + rps - 1) // rps,), device="cuda", dtype=torch.int32)
    rk = torch.zeros(16, K, device="cuda", dtype=h16)
    ops.PackPlan([(P, False, rk)], h16, "cuda").run()
    bp = ops.pack_b(b)
    c, at = Place(guard, "middle-third", "c"), Place(guard, "tight", "a")
    got = []
    for pc, pa in ((Place(guard), Place(guard)), (c, at)):
        o = dict(out=pc.out("c", M, N, h16, "out"), t=guard.out(M, r, name=f"t [{pc.tag}]"), ts=guard.out(M, r, name=f"ts [{pc.tag}]"))
        ro = ops.RankOp(rk, S, attr, rps, 0.25, 0.7, t_out=o["t"], ts_out=o["ts"])
        ops.gemm_nt(pa.inp("a", a), b, o["out"], lw=lw, rankop=ro, b_packed=bp, bias=bias, res=pc.inp("c", res))
        got.append(o)
    ref_t = a.double() @ P.to(h16).double()
    ref_ts = 0.25 * ref_t * (mix(attr, G)[torch.arange(M, device="cuda") // rps] @ S.double())
    ref = a.double() @ b.double().t() + ref_ts.to(h16).double() @ lw.to(h16).double() + bias.double() + res.double()
    check(got[0]["t"], ref_t, 2e-5, "t")
    check(got[0]["ts"], ref_ts, 2e-5, "ts")
    check(got[0]["out"], ref, tol(h16), "fused out")
    same(got[1], got[0], "panel proj_fwd: out / res in the middle third, A tight")
    guard.check()


@H16
def test_pack_b_strided_source(ops, guard, h16):
    """pack_b_kernel (csrc/gemm_panel.hip) on a source with ld = K + 8 (and the thirds): the packed weight of the contiguous copy,
    bit for bit - and that one is a permutation of the source."""
    N, K = 128, 256
    w = rnd(N, K, dt=h16, seed=81)
    ref = ops.pack_b(w, guard.out(N * K, dtype=h16, name="packed [contiguous]"))
    assert torch.equal(ref.float().sort().values, w.float().flatten().sort().values)
    lane = ref.view(N // 16, K // 32, 64, 8)[3, 5, 37]                  # lane l: row l & 15, k-group l >> 4 (include/ffm_hip.h)
    assert torch.equal(lane, w[3 * 16 + (37 & 15), 5 * 32 + (37 >> 4) * 8:][:8])
    for layout in LAYOUTS:
        pl = Place(guard, layout, "b")
        got = ops.pack_b(pl.inp("b", w), guard.out(N * K, dtype=h16, name=f"packed [{pl.tag}]"))
        assert torch.equal(got, ref), pl.tag
    guard.check()


# ------------------------------------------------------------ LoRA (csrc/lora.hip) ---
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,K,r,G,rps,rk", [(333, 768, 16, 3, 50, True), (70, 128, 4, 2, 17, False), (333, 768, 32, 3, 50, True),
                                            (1030, 512, 5, 3, 197, True)])
def test_lora_down_strided(ops, guard, dt, M, K, r, G, rps, rk):
    """lora_down_kernel (the VALU kernel: fewer than 1024 rows keep 16-bit storage off the matrix-core one); r = 32: two passes
    over the rank, the second re-reading x.  1030 rows of [r, K] operand rows in 16-bit storage: lora_down_mfma_kernel, which
    writes a dS partial row per 16 rows (test_lora_down_tails asserts the same from ffm_lora_down_blocks).  x behind a stride;
    t, ts and the dS partials bit for bit; reference of lora_down_case."""
    mfma = dt != torch.float32 and rk and r <= 16 and M >= 1024         # down_mfma_ok (csrc/lora.hip)
    assert mfma == (M == 1030 and dt != torch.float32)
    if M >= 1024:
        assert (ops.lora_down_blocks(M, K, r, dt) == (M + 15) // 16) == mfma
    x = rnd(M, K, dt=dt, seed=25)
    P = rnd(r, K, scale=0.1, seed=26) if rk else rnd(K, r, scale=0.1, seed=26)
    S, t_fwd = rnd(G, r, seed=27), rnd(M, r, seed=28)
    attr = torch.randint(0, G, ((M + rps - 1) // rps,), device="cuda", dtype=torch.int32)
    nb = ops.lora_down_blocks(M, K, r, dt)

    def run(pl):
        o = dict(t=guard.out(M, r, name=f"t [{pl.tag}]"), ts=guard.out(M, r, name=f"ts [{pl.tag}]"),
                 ds_part=guard.out(nb, G, r, name=f"ds_part [{pl.tag}]"))
        ops.lora_down(pl.inp("x", x), P, rk, S, attr, r, G, rps, 0.25, 0.7, o["t"], o["ts"], t_fwd, o["ds_part"])
        return o

    ref = run(Place(guard))
    Pq = P.to(dt).double()
    ref_t = x.double() @ (Pq.t() if rk else Pq)
    pi_rows = mix(attr, G)[torch.arange(M, device="cuda") // rps]
    check(ref["t"], ref_t, 2e-5, "t")
    check(ref["ts"], 0.25 * ref_t * (pi_rows @ S.double()), 2e-5, "ts")
    check(ref["ds_part"].double().sum(0), pi_rows.t() @ (0.25 * t_fwd.double() * ref_t), 5e-5, "dS")
    for layout in LAYOUTS:
        pl = Place(guard, layout, "x")
        same(run(pl), ref, pl.tag)
    guard.check()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,K,r", [(130, 256, 8), (130, 264, 32), (64, 128, 4)])
def test_lora_grad_partial_strided(ops, guard, dt, M, K, r):
    """(130, 256, 8): lora_grad_mfma_kernel in 16-bit storage (K a multiple of 128), lora_grad_kernel in float32; (130, 264, 32):
    lora_grad_kernel in every dtype, two passes over the rank; (64, 128, 4): one row group.  x behind a stride: the partials
    bit for bit; their sum as lora_grad_case checks it."""
    x, v = rnd(M, K, dt=dt, seed=29), rnd(M, r, seed=30)
    ns = ops.lora_grad_splits(M)
    assert ns == (M + 127) // 128

    def run(pl):
        part = guard.out(ns, K, r, name=f"part [{pl.tag}]")
        ops.lora_grad_partial(pl.inp("x", x), v, r, part)
        return dict(part=part)

    ref = run(Place(guard))
    want = x.double().t() @ v.double()
    out, out_t = guard.out(K, r, name="dA-style"), guard.out(r, K, name="dB-style")
    ops.reduce_partials(ref["part"], ns, K * r, out)
    ops.reduce_partials(ref["part"], ns, K * r, out_t, transpose_K=K, transpose_r=r)
    check(out, want, 3e-5, "dA-style [K,r]")
    check(out_t, want.t(), 3e-5, "dB-style [r,K]")
    for layout in LAYOUTS:
        pl = Place(guard, layout, "x")
        same(run(pl), ref, pl.tag)
    guard.check()


@H16
def test_lora_grad_partial_ln_strided(ops, guard, h16):
    """lora_grad_mfma_kernel with the folded LayerNorm (ffm_lora_grad_partial_ln), M = 130, K = 256, r = 8, x - the RAW rows -
    behind a stride; reference and bound of lora_grad_partial_ln_case."""
    M, K, r = 130, 256, 8
    g = torch.Generator(device="cuda").manual_seed(9)
    x = (0.7 + 1.5 * torch.randn(M, K, device="cuda", generator=g)).to(h16)
    v = torch.randn(M, r, device="cuda", generator=g)
    gamma = 1 + 0.2 * torch.randn(K, device="cuda", generator=g)
    beta = 0.3 * torch.randn(K, device="cuda", generator=g)
    xd = x.double()
    mu, rstd = xd.mean(1), 1 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)
    mu32, rstd32 = mu.float(), rstd.float()
    ns = ops.lora_grad_splits(M)

    def run(pl):
        part = guard.out(ns, K, r, name=f"part [{pl.tag}]")
        ops.lora_grad_partial_ln(pl.inp("x", x), v, mu32, rstd32, gamma, beta, r, part)
        return dict(part=part)

    ref = run(Place(guard))
    y = (xd - mu[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    want = y.t() @ v.double()
    assert not torch.isnan(ref["part"]).any()
    assert float((ref["part"].double().sum(0) - want).abs().max() / want.abs().max()) < 2e-4      # v enters as a bf16 hi + lo pair
    for layout in LAYOUTS:
        pl = Place(guard, layout, "x")
        same(run(pl), ref, pl.tag)
    guard.check()


# ------------------------------------------------------------ refusals: host code, ahead of any launch ---
def bad_views(buf, rows, width, dt):
    """The refused forms of a [rows, width] operand, each a view of `buf` [rows, width + 8] that stays inside it:
    a stride below the width, a stride that is no multiple of 16 bytes, a base that is not 16-byte aligned."""
    odd = 4 if dt != torch.float32 else 2                              # half of 16 bytes, in elements
    flat = buf.reshape(-1)
    return {"ld < width": torch.as_strided(flat, (rows, width), (width - 8, 1)),
            "stride not a multiple of 16 bytes": torch.as_strided(flat, (rows, width), (width + odd, 1)),
            "base not 16-byte aligned": buf[:, odd:odd + width]}


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_gemm_refuses_bad_strides(ops, guard, dt):
    """ffm_gemm_nt validates lda / ldb / ldc and the three bases (csrc/gemm.hip, ahead of every launch): FFM_EINVAL, nothing
    written.  A side tensor whose stride differs from `out`'s is refused by ops.gemm_nt itself (they share ldc in the ABI)."""
    M, N, K = 200, 264, 192
    a, b = rnd(M, K + 8, dt=dt, seed=3), rnd(N, K + 8, dt=dt, seed=4)
    good_a, good_b = a[:, 8:], b[:, 8:]
    out = guard.scratch(M, N + 8, dtype=dt, name="out")
    good_out = out[:, 8:]
    for role, views in (("a", bad_views(a, M, K, dt)), ("b", bad_views(b, N, K, dt)), ("c", bad_views(out, M, N, dt))):
        for why, v in views.items():
            args = dict(a=good_a, b=good_b, c=good_out)
            args[role] = v
            with pytest.raises(RuntimeError, match="invalid argument"):
                ops.gemm_nt(args["a"], args["b"], args["c"])
    res = rnd(M, N, dt=dt, seed=8)                                     # stride N against out's N + 8
    for kw in (dict(res=res), dict(gelu_out=res, bias=rnd(N, seed=5)), dict(dgelu_aux=res)):
        with pytest.raises(AssertionError):
            ops.gemm_nt(good_a, good_b, good_out, **kw)
    guard.check()
    assert bool(torch.isnan(out.float()).all())


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_lora_calls_refuse_bad_strides(ops, guard, dt):
    """ffm_lora_down, ffm_lora_grad_partial and ffm_lora_grad_partial_ln (16-bit storage) validate ldx and the base of x ahead
    of every launch (csrc/lora.hip): ldx < K - rows that overlap -, a stride that is no multiple of 16 bytes and a misaligned
    base are FFM_EINVAL, nothing written.  Every view stays inside an [M, K + 8] buffer the test owns."""
    M, K, r, G = 70, 128, 8, 2
    xb = rnd(M, K + 8, dt=dt, seed=25)
    P, S, v = rnd(K, r, scale=0.1, seed=26), rnd(G, r, seed=27), rnd(M, r, seed=30)
    t, ts = guard.scratch(M, r, name="t"), guard.scratch(M, r, name="ts")
    part = guard.scratch(ops.lora_grad_splits(M), K, r, name="part")
    stats, vec = torch.ones(M, device="cuda"), torch.ones(K, device="cuda")
    for why, x in bad_views(xb, M, K, dt).items():
        with pytest.raises(RuntimeError, match="ffm_lora_down failed .*invalid argument"):
            ops.lora_down(x, P, False, S, None, r, G, 17, 0.25, 0.7, t, ts)
        with pytest.raises(RuntimeError, match="ffm_lora_grad_partial failed .*invalid argument"):
            ops.lora_grad_partial(x, v, r, part)
        if dt != torch.float32:
            with pytest.raises(RuntimeError, match="ffm_lora_grad_partial_ln failed .*invalid argument"):
                ops.lora_grad_partial_ln(x, v, stats, stats, vec, vec, r, part)
    guard.check()
    assert all(bool(torch.isnan(o).all()) for o in (t, ts, part))


@H16
def test_pack_b_refuses_bad_strides(ops, guard, h16):
    """ffm_pack_b (csrc/gemm_panel.hip): ld < K, ld % 8, a misaligned source - FFM_EINVAL ahead of the launch."""
    N, K = 128, 256
    wb = rnd(N, K + 8, dt=h16, seed=81)
    dst = guard.scratch(N * K, dtype=h16, name="packed")
    for why, w in bad_views(wb, N, K, h16).items():
        with pytest.raises(RuntimeError, match="ffm_pack_b failed .*invalid argument"):
            ops.pack_b(w, dst)
    guard.check()
    assert bool(torch.isnan(dst.float()).all())
