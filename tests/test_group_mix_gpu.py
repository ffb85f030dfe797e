"""The FairLoRA group mix pi_b for attribute values outside [0, G), in all four kernels that implement it.

The rule (include/ffm_hip.h): a value outside [0, G) - the loaders' -1, any other negative value, an index
at or above G - is "unknown"; that sample takes the uniform 1/G mix, with the arithmetic of attr == NULL, in the forward's
ts and in the dS partials alike.  The reference raises in F.one_hot on such a value, so the oracle's rule
(oracle.fairlora_oracle.group_mix, tests/test_group_mix_cpu.py; `mix` of tests/test_kernels_gpu.py is the same rule in
float64 on the GPU) is the project's own definition.

The four implementations: the VALU lora_down kernel (group_mix_w), the matrix-core lora_down kernel, the FFM_EPI_RANKOP
epilogue of the 128 x 128 GEMM and the rank stage of the panel GEMM.

Every launch takes ONE fixed attribute pattern repeated over the samples - for G = 3: [0, -1, 2, G, 1, -2, 0, G + 1, 1] - at
37 rows per sample, so that every 128- to 208-row tile holds at least three sample boundaries, samples straddle tile edges
and the last sample is ragged.  The unknown values stay within {-2, -1, G, G + 1}.

Assertions per launch (float64 references from the kernel's own rounded inputs, outputs pre-filled with NaN):
  (a) t at 2e-5 of its scale, the fused output at tol(dt), and ts at 2e-5 PER SAMPLE (max error over the sample's rows
      over the max of the reference over the same rows: a wrong sample cannot hide under the global scale);
  (b) dS per group ROW: |sum of partials - ref|[g] over max_j (pi^T |scaling t_fwd t|)[g, j], the cancellation-free scale of
      the sum being formed, at the project's 5e-5;
  (c) bit-level: an all-unknown attribute vector (all -1, all G) gives torch.equal results to attr=None.
"""
import pytest
import torch

from tests.guarded import guard_fixture
from tests.test_kernels_gpu import (DT, H16, IDS, check, mix, panel_fairlora_case, panel_layernorm_backward_fold_case,
                                    panel_lgrad_case, rnd, tol)

pytestmark = pytest.mark.gpu

RPS = 37                      # rows per sample
SCALING, LAM = 0.25, 0.7
DS_BOUND = 5e-5


@pytest.fixture(scope="module")
def ops():
    from fairfedmed_amd import ops
    return ops


@pytest.fixture
def guard():
    """Every kernel output of this file: poisoned body between two guard bands (tests/guarded.py); unchecked at teardown = failure."""
    yield from guard_fixture()


def attr_pattern(G, M, rps=RPS, kind="mixed"):
    """[ceil(M / rps)] int32: the fixed pattern, repeated.  `valid`: the same with every unknown value replaced by a group."""
    n = (M + rps - 1) // rps
    base = {"mixed": [0, -1, G - 1, G, 1, -2, 0, G + 1, 1], "valid": [0, 1, G - 1, 0, 1, G - 1, 0, 1, 1]}[kind]
    return torch.tensor((base * (n // 9 + 1))[:n], device="cuda", dtype=torch.int32)


def attr_const(v, M, rps=RPS):
    return torch.full(((M + rps - 1) // rps,), v, device="cuda", dtype=torch.int32)


def pi_of_rows(attr, G, M, rps=RPS):
    pi = mix(attr, G, LAM)
    return pi[torch.arange(M, device="cuda") // rps] if attr is not None else pi.expand(M, G)


def check_ts_per_sample(ts, ref_ts, attr, rps, bound, what):
    M, r = ref_ts.shape
    n = (M + rps - 1) // rps
    pad = (0, 0, 0, n * rps - M)
    err = torch.nan_to_num((ts.double() - ref_ts).abs(), nan=float("inf"))
    e = torch.nn.functional.pad(err, pad).view(n, rps * r).amax(1)
    s = torch.nn.functional.pad(ref_ts.abs(), pad).view(n, rps * r).amax(1).clamp_min(1e-30)
    q = e / s
    b = int(q.argmax())
    print(f"{what}: worst per-sample ts error {float(q[b]):.3e}")
    assert float(q[b]) <= bound, (f"{what}: ts of sample {b} (rows {b * rps}..{min(M, (b + 1) * rps) - 1}, attribute "
                                  f"{'none' if attr is None else int(attr[b])}): max err / sample scale = {float(q[b]):.3e} > {bound:.1e}")


def check_ds_per_group(dsp, ref_t, t_fwd, pi_rows, scaling, bound, what):
    w = scaling * t_fwd.double() * ref_t
    ref = pi_rows.t() @ w                                             # [G, r]
    scale = (pi_rows.t() @ w.abs()).amax(1).clamp_min(1e-30)          # [G]: no cancellation in it
    q = torch.nan_to_num((dsp.double().sum(0) - ref).abs(), nan=float("inf")).amax(1) / scale
    g = int(q.argmax())
    print(f"{what}: worst per-group dS error {float(q[g]):.3e}")
    assert float(q[g]) <= bound, f"{what}: dS row of group {g}: |sum of partials - ref| / sum of magnitudes = {float(q[g]):.3e} > {bound:.1e}"


def strict_checks(what):
    """`before_checks` of the panel helpers of tests/test_kernels_gpu.py: assertions (a) and (b) on one launch."""
    def f(res):
        if res.t is not None:
            check(res.t, res.ref_t, 2e-5, what + ": t")
        check_ts_per_sample(res.ts, res.ref_ts, res.attr, res.rps, 2e-5, what)
        if res.out is not None:
            check(res.out, res.ref_out, tol(res.dt), what + ": fused out")
        if res.dsp is not None:
            check_ds_per_group(res.dsp, res.ref_t, res.t_fwd, res.pi_rows, res.scaling, DS_BOUND, what)
    return f


def same_bits(got, ref, what):
    for name in ref:
        if ref[name] is not None:
            assert torch.equal(got[name], ref[name]), f"{what}: {name} differs from the attr=None launch"


# ------------------------------------------------------- lora_down (both kernels) ---
def down_launch(ops, guard, x, P, rk, S, attr, r, G, with_ds, t_fwd, rps=RPS):
    M, K = x.shape
    t, ts = guard.out(M, r), guard.out(M, r)
    dsp = guard.out(ops.lora_down_blocks(M, K, r, x.dtype), G, r) if with_ds else None
    ops.lora_down(x, P, rk, S, attr, r, G, rps, SCALING, LAM, t, ts, t_fwd if with_ds else None, dsp)
    return {"t": t, "ts": ts, "dsp": dsp}


def down_checks(got, ref_t, S, attr, G, t_fwd, what, rps=RPS):
    M = ref_t.shape[0]
    pi_rows = pi_of_rows(attr, G, M, rps)
    check(got["t"], ref_t, 2e-5, what + ": t")
    check_ts_per_sample(got["ts"], SCALING * ref_t * (pi_rows @ S.double()), attr, rps, 2e-5, what)
    if got["dsp"] is not None:
        check_ds_per_group(got["dsp"], ref_t, t_fwd, pi_rows, SCALING, DS_BOUND, what)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("rk", [False, True], ids=["P_Kr", "P_rK"])
@pytest.mark.parametrize("K", [128, 768, 3072])            # 1, 2 and 4 K slices per block (down_kq), in f32 and 16-bit alike
def test_valu_lora_down(ops, guard, dt, rk, K):
    """lora_down_kernel (group_mix_w): 300 rows stay below the matrix-core kernel's 1024; r = 32 takes the second rank
    pass (j0 = 16)."""
    M = 300
    x = rnd(M, K, dt=dt, seed=25)
    for r in (4, 12, 32):
        P = rnd(r, K, scale=0.1, seed=26) if rk else rnd(K, r, scale=0.1, seed=26)
        Pq = P.to(dt).double()                                # the kernel keeps P in the activation dtype in LDS
        ref_t = x.double() @ (Pq.t() if rk else Pq)
        t_fwd = rnd(M, r, seed=28)
        for G in (2, 3, 8):
            S = rnd(G, r, seed=27)
            what = f"VALU lora_down r={r} G={G}"
            attr = attr_pattern(G, M)
            got = down_launch(ops, guard, x, P, rk, S, attr, r, G, True, t_fwd)
            down_checks(got, ref_t, S, attr, G, t_fwd, what)
            fwd = down_launch(ops, guard, x, P, rk, S, attr, r, G, False, t_fwd)        # the forward call: no t_fwd / ds_part
            assert torch.equal(fwd["t"], got["t"]) and torch.equal(fwd["ts"], got["ts"]), what + ": forward call differs"
            none = down_launch(ops, guard, x, P, rk, S, None, r, G, True, t_fwd)
            down_checks(none, ref_t, S, None, G, t_fwd, what + " attr=None")
            for v in (-1, G):
                same_bits(down_launch(ops, guard, x, P, rk, S, attr_const(v, M), r, G, True, t_fwd), none, f"{what} all {v}")
    guard.check()


@pytest.mark.parametrize("r", [5, 16])
@pytest.mark.parametrize("G", [3, 8])                      # G * r = 128 > 64: the second store loop of the dS partial
@H16
def test_mfma_lora_down(ops, guard, r, G, h16):
    """lora_down_mfma_kernel: 16-bit storage, [r, K] rows, >= 1024 rows (1030: a ragged last 16-row block)."""
    dt, M, K = h16, 1030, 512
    # by construction not the VALU kernel: one dS partial row per 16 rows is the matrix-core kernel's block count
    assert ops.lora_down_blocks(M, K, r, dt) == (M + 15) // 16
    assert ops.lora_down_blocks(1000, K, r, dt) != (1000 + 15) // 16
    x = rnd(M, K, dt=dt, seed=25)
    P, S, t_fwd = rnd(r, K, scale=0.1, seed=26), rnd(G, r, seed=27), rnd(M, r, seed=28)
    ref_t = x.double() @ P.to(dt).double().t()
    what = f"MFMA lora_down r={r} G={G}"
    attr = attr_pattern(G, M)
    got = down_launch(ops, guard, x, P, True, S, attr, r, G, True, t_fwd)
    down_checks(got, ref_t, S, attr, G, t_fwd, what)
    fwd = down_launch(ops, guard, x, P, True, S, attr, r, G, False, t_fwd)
    assert torch.equal(fwd["t"], got["t"]) and torch.equal(fwd["ts"], got["ts"]), what + ": forward call differs"
    none = down_launch(ops, guard, x, P, True, S, None, r, G, True, t_fwd)
    down_checks(none, ref_t, S, None, G, t_fwd, what + " attr=None")
    for v in (-1, G):
        same_bits(down_launch(ops, guard, x, P, True, S, attr_const(v, M), r, G, True, t_fwd), none, f"{what} all {v}")
    # the VALU kernel on the first 1000 rows (27 whole samples and a part of the 28th: the same attribute prefix) agrees
    valu = down_launch(ops, guard, x[:1000], P, True, S, attr[:(1000 + RPS - 1) // RPS].contiguous(), r, G, False, None)
    check(got["t"][:1000], valu["t"].double(), 2e-5, what + ": t against the VALU kernel")
    check_ts_per_sample(got["ts"][:1000], valu["ts"].double(), attr, RPS, 2e-5, what + " against the VALU kernel")
    guard.check()


# ------------------------------------------------- 128 x 128 GEMM, FFM_EPI_RANKOP ---
def rankop_launch(ops, guard, a, b, bias, rk_op, S, lw, kr, attr, r, G, t_fwd, rps=RPS):
    M, N = a.shape[0], b.shape[0]
    out = guard.out(M, N, dtype=a.dtype)
    t, ts = guard.out(M, r), guard.out(M, r)
    dsp = guard.out(ops.gemm_tiles_m(M), G, r)
    ro = ops.RankOp(rk_op, S, attr, rps, SCALING, LAM, t_out=t, ts_out=ts, t_fwd=t_fwd, ds_part=dsp)
    ops.gemm_nt(a, b, out, bias=bias, lw=lw, lw_is_kr=kr, rankop=ro)
    return {"t": t, "ts": ts, "out": out, "dsp": dsp}


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("kr", [False, True], ids=["lw_rN", "lw_Nr"])
@pytest.mark.parametrize("r", [8, 12, 16])                 # a power of two and any other rank take different dS code
def test_gemm128_rank_epilogue(ops, guard, dt, kr, r):
    M, N, K = 300, 256, 256
    a, b = rnd(M, K, dt=dt, seed=50), rnd(N, K, dt=dt, scale=K ** -0.5, seed=51)
    bias, P = rnd(N, seed=52), rnd(K, r, scale=0.1, seed=53)
    lw = rnd(N, r, seed=55) if kr else rnd(r, N, seed=55)
    t_fwd = rnd(M, r, seed=56)
    rk_op = torch.zeros(16, K, device="cuda", dtype=dt)
    ops.PackPlan([(P, False, rk_op)], dt, "cuda").run()
    ref_t = a.double() @ P.to(dt).double()
    ref_ab = a.double() @ b.double().t() + bias.double()
    lwm = lw.double().t() if kr else lw.double()
    for G in (2, 3, 8):
        S = rnd(G, r, seed=54)
        what = f"128x128 rank epilogue r={r} G={G}"

        def checks(got, attr, what):
            pi_rows = pi_of_rows(attr, G, M)
            ref_ts = SCALING * ref_t * (pi_rows @ S.double())
            check(got["t"], ref_t, 2e-5, what + ": t")
            check_ts_per_sample(got["ts"], ref_ts, attr, RPS, 2e-5, what)
            check(got["out"], ref_ab + ref_ts @ lwm, tol(dt), what + ": fused out")
            check_ds_per_group(got["dsp"], ref_t, t_fwd, pi_rows, SCALING, DS_BOUND, what)

        attr = attr_pattern(G, M)
        checks(rankop_launch(ops, guard, a, b, bias, rk_op, S, lw, kr, attr, r, G, t_fwd), attr, what)
        none = rankop_launch(ops, guard, a, b, bias, rk_op, S, lw, kr, None, r, G, t_fwd)
        checks(none, None, what + " attr=None")
        for v in (-1, G):
            same_bits(rankop_launch(ops, guard, a, b, bias, rk_op, S, lw, kr, attr_const(v, M), r, G, t_fwd), none, f"{what} all {v}")
    guard.check()


# ------------------------------------------------------- panel GEMM, rank stage ---
# N = 3072, K = 768: the dispatcher hands a shape to the panel kernel once the 128 x 128 kernel would need more than 256
# tiles (M > 1280 there): 1500 rows take the 160 x 128 tile.  N = 768, K = 3072: 5377 is the smallest M for which
# gemm_tiles_m(packed) != gemm_tiles_m(unpacked); the helpers assert that idiom, so a shape that silently falls back to the
# 128 x 128 kernel fails.  The FFM_EPI_LGRAD epilogue exists on the 208 x 384 tile only, which the dispatcher picks from
# 2689 rows on.
M_WIDE, M_NARROW, M_LGRAD = 1500, 5377, 2689
PANEL_RG = [(4, 3), (4, 8), (8, 3), (8, 8), (16, 3), (16, 8)]


def panel_m(case):
    return M_WIDE if case in ("fc_fwd", "proj_dx", "proj_dx_deriv") else M_NARROW


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("case", ["fc_fwd", "proj_fwd", "proj_dx", "fc_dx", "proj_dx_deriv"])
@pytest.mark.parametrize("r,G", PANEL_RG)
@H16
def test_panel_rank_stage(ops, guard, case, r, G, h16):
    M = panel_m(case)
    what = f"panel {case} r={r} G={G}"
    res = panel_fairlora_case(ops, guard, case, M, r, G, attr_pattern(G, M), RPS, h16, before_checks=strict_checks(what))
    none = panel_fairlora_case(ops, guard, case, M, r, G, None, RPS, h16, before_checks=strict_checks(what + " attr=None"))
    ref = {k: getattr(none, k) for k in ("t", "ts", "out", "act", "dsp")}
    for v in (-1, G):
        got = panel_fairlora_case(ops, guard, case, M, r, G, attr_const(v, M), RPS, h16)
        same_bits({k: getattr(got, k) for k in ref}, ref, f"{what} all {v}")
    guard.check()


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("r,G", PANEL_RG)
@H16
def test_panel_rank_stage_lgrad(ops, guard, r, G, h16):
    M = M_LGRAD
    import os
    if "FFM_PANEL_MASK" not in os.environ:       # (under a tile mask without the 208 x 384 LGRAD tile the helper skips, as its own test does)
        assert ops.gemm_lgrad_rows(M, 3072, 768, r, h16, True) > 0, "the default tile set serves FFM_EPI_LGRAD at this shape"
    panel_lgrad_case(ops, guard, M, r, G, attr_pattern(G, M), RPS, h16, before_checks=strict_checks(f"panel LGRAD r={r} G={G}"))


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("r,G", [(4, 3), (4, 8), (8, 3), (8, 8), (12, 3), (12, 8)])     # (rows 14 / 15 of the rank operand are taken: r <= 14)
@H16
def test_panel_rank_stage_layernorm_fold(ops, guard, r, G, h16):
    """LNB_STAT (dX of c_proj, N = 3072) and LNB_APPLY (dX of c_fc, N = 768: the larger M of the two shapes)."""
    M = M_NARROW
    panel_layernorm_backward_fold_case(ops, guard, M, r, G, attr_pattern(G, M), RPS, h16,
                                       before_checks=strict_checks(f"panel LayerNorm fold r={r} G={G}"))
    guard.check()
