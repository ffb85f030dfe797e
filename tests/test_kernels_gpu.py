"""Per-kernel parity of the HIP library (through the C ABI) against plain
PyTorch fp32/fp64 references of the same op, on the GPU.

Tolerances: fp32 kernels run exact-f32 MFMA / VALU with a different reduction
order than PyTorch -> rtol 2e-5 of the output scale; bf16 kernels are compared
with a reference computed from the SAME bf16-rounded inputs in fp32, so only
accumulation order and the final rounding differ -> 1e-2 of the output scale.
"""
import math

import pytest
import torch

from tests.guarded import guard_fixture

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
# the two 16-bit storage types run the same sources (csrc/common.h, FFM_TWIN_F16): every 16-bit-only test takes both
H16 = pytest.mark.parametrize("h16", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])


def tol(dt):
    # max error / tensor scale: bf16 rounds to 2^-9, IEEE half to 2^-12 (held 6x tighter: a half path that quietly ran
    # in bfloat16 fails it)
    return 2e-5 if dt == torch.float32 else 1.2e-2 if dt == torch.bfloat16 else 2e-3


def rel_err(got, ref):
    got, ref = got.double(), ref.double()
    scale = ref.abs().max().clamp_min(1e-30)
    return float((got - ref).abs().max() / scale)


def check(got, ref, t, what):
    e = rel_err(got, ref)
    assert math.isfinite(e) and e <= t, f"{what}: max err / scale = {e:.3e} > {t:.1e}"


@pytest.fixture(scope="module")
def ops():
    from fairfedmed_amd import ops
    return ops


@pytest.fixture
def guard():
    """Every kernel output of this file: poisoned body between two guard bands (tests/guarded.py); unchecked at teardown = failure."""
    yield from guard_fixture()


def rnd(*shape, dt=torch.float32, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dt)


# ------------------------------------------------------------------ GEMM ---
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (200, 264, 192), (6304, 768, 768), (1000, 512, 3072)])
def test_gemm_plain(ops, guard, dt, M, N, K):
    a, b = rnd(M, K, dt=dt, seed=1), rnd(N, K, dt=dt, scale=K ** -0.5, seed=2)
    out = guard.out(M, N, dtype=dt)
    ops.gemm_nt(a, b, out)
    check(out, a.double() @ b.double().t(), tol(dt), "gemm")
    guard.check()


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_gemm_asymmetric_identity(ops, guard, dt):
    # A = I, asymmetric B: catches a transposed C write or a wrong k mapping exactly
    n = 128
    a = torch.eye(n, device="cuda", dtype=dt)
    b = (torch.arange(n * n, device="cuda", dtype=torch.float32).reshape(n, n) % 251 - 125).to(dt)
    out = guard.out(n, n, dtype=dt)
    ops.gemm_nt(a, b, out)
    assert torch.equal(out.float(), b.float().t())
    guard.check()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("r,kr", [(4, False), (8, False), (8, True), (16, False), (32, True)])
def test_gemm_fused_epilogue(ops, guard, dt, r, kr):
    M, N, K = 333, 384, 256
    a, b = rnd(M, K, dt=dt, seed=3), rnd(N, K, dt=dt, scale=K ** -0.5, seed=4)
    bias = rnd(N, seed=5)
    ts = rnd(M, r, seed=6)
    lw = rnd(N, r, seed=7) if kr else rnd(r, N, seed=7)
    res = rnd(M, N, dt=dt, seed=8)
    lwm = lw.t() if kr else lw
    ref = a.double() @ b.double().t() + bias.double() + ts.double() @ lwm.double() + res.double()
    out = guard.out(M, N, dtype=dt)
    ops.gemm_nt(a, b, out, bias=bias, ts=ts, lw=lw, lw_is_kr=kr, res=res)
    check(out, ref, tol(dt), "gemm+bias+lora+res")
    guard.check()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("r,G,kr,use_attr", [(8, 3, False, True), (16, 3, True, True), (4, 2, False, False), (12, 3, True, True)])
def test_gemm_rankop_fused_lora(ops, guard, dt, r, G, kr, use_attr):
    """FFM_EPI_RANKOP: t = a . P (inside the GEMM), ts = scaling t s_b, out = a b^T + bias + ts lw, dS partials."""
    M, N, K, rps = 700, 384, 256, 197
    a, b = rnd(M, K, dt=dt, seed=50), rnd(N, K, dt=dt, scale=K ** -0.5, seed=51)
    bias = rnd(N, seed=52)
    P = rnd(K, r, scale=0.1, seed=53)                                  # e.g. lora_A [K, r]
    S = rnd(G, r, seed=54)
    lw = rnd(N, r, seed=55) if kr else rnd(r, N, seed=55)
    nsamp = (M + rps - 1) // rps
    attr = torch.randint(0, G, (nsamp,), device="cuda", dtype=torch.int32) if use_attr else None
    t_fwd = rnd(M, r, seed=56)
    rk = torch.zeros(16, K, device="cuda", dtype=dt)
    ops.PackPlan([(P, False, rk)], dt, "cuda").run()
    assert torch.equal(rk[:r].float(), P.t().to(dt).float()) and float(rk[r:].abs().sum()) == 0.0
    out = guard.out(M, N, dtype=dt)
    t, ts = guard.out(M, r), guard.out(M, r)
    dsp = guard.out(ops.gemm_tiles_m(M), G, r)
    ro = ops.RankOp(rk, S, attr, rps, 0.25, 0.7, t_out=t, ts_out=ts, t_fwd=t_fwd, ds_part=dsp)
    ops.gemm_nt(a, b, out, bias=bias, lw=lw, lw_is_kr=kr, rankop=ro)
    ref_t = a.double() @ P.to(dt).double()
    pi = mix(attr, G)
    rows = torch.arange(M, device="cuda") // rps
    pi_rows = pi[rows] if attr is not None else pi.expand(M, G)
    ref_ts = 0.25 * ref_t * (pi_rows @ S.double())
    lwm = lw.double().t() if kr else lw.double()
    check(t, ref_t, 2e-5, "t")
    check(ts, ref_ts, 2e-5, "ts")
    check(out, a.double() @ b.double().t() + bias.double() + ref_ts @ lwm, tol(dt), "fused out")
    check(dsp.double().sum(0), pi_rows.t() @ (0.25 * t_fwd.double() * ref_t), 5e-5, "dS")
    guard.check()



# ------------------------------------------------- panel GEMM (packed B) ---
@pytest.mark.mask_tolerant
@pytest.mark.parametrize("M,N,K,mode", [(6304, 2048, 1536, "b"), (6304, 768, 768, "br"), (6304, 768, 2304, ""),
                                         (6000, 768, 3072, "br"), (4100, 1024, 512, "b")])
@H16
def test_gemm_panel_plain(ops, guard, M, N, K, mode, h16):
    panel_plain_case(ops, guard, M, N, K, mode, h16)


def panel_plain_case(ops, guard, M, N, K, mode, h16):
    """Frozen weights packed in MFMA-fragment order -> panel kernel (csrc/gemm_panel_impl.h); same contract as
    ffm_gemm_nt on the row-major operand."""
    dt = h16
    flags = (1 if "b" in mode else 0) | (8 if "r" in mode else 0)
    assert ops.gemm_tiles_m(M, N, K, flags, 0, dt, True) != ops.gemm_tiles_m(M, N, K, flags, 0, dt, False), \
        "shape does not select the panel kernel"
    a, b = rnd(M, K, dt=dt, seed=60), rnd(N, K, dt=dt, scale=K ** -0.5, seed=61)
    kw = {}
    ref = a.double() @ b.double().t()
    if "b" in mode:
        kw["bias"] = rnd(N, seed=62)
        ref = ref + kw["bias"].double()
    if "r" in mode:
        kw["res"] = rnd(M, N, dt=dt, seed=63)
        ref = ref + kw["res"].double()
    out = guard.out(M, N, dtype=dt)
    ops.gemm_nt(a, b, out, b_packed=ops.pack_b(b), **kw)
    check(out, ref, tol(dt), "panel " + mode)
    out2 = guard.like(out)
    ops.gemm_nt(a, b, out2, **kw)                    # the 128x128 kernel on the same operands
    check(out, out2.double(), 1e-2, "panel vs 128x128")
    guard.check()


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("case", ["fc_fwd", "proj_fwd", "proj_dx", "fc_dx", "proj_dx_deriv"])
@pytest.mark.parametrize("M,r,G,use_attr", [(6304, 8, 3, True), (5500, 16, 2, False), (6304, 4, 3, True)])
@H16
def test_gemm_panel_fairlora(ops, guard, case, M, r, G, use_attr, h16):
    """The four FairLoRA GEMMs of a block on the panel kernel: t / ts / dS partials / fused rank-r update / GELU."""
    rps = 197
    nsamp = (M + rps - 1) // rps
    attr = torch.randint(0, G, (nsamp,), device="cuda", dtype=torch.int32) if use_attr else None
    panel_fairlora_case(ops, guard, case, M, r, G, attr, rps, h16)


def panel_fairlora_case(ops, guard, case, M, r, G, attr, rps, dt, before_checks=None, rowstats=False, shape=None, gscale=1.0):
    """Body of test_gemm_panel_fairlora for a given attribute vector ([ceil(M / rps)] int32 or None) and rows per sample.
    gscale multiplies the gradient operand of the two dX cases (a = dL/dy; tests/test_grad_range_gpu.py).
    `before_checks(res)` (tests/test_group_mix_gpu.py) sees every tensor of the launch and its float64 reference before
    this function's own assertions run."""
    width = 768
    deriv = case == "proj_dx_deriv"               # dX(c_proj) with the saved tensor = quick_gelu'(pre) (gelu_deriv)
    case = "proj_dx" if deriv else case
    N, K = (4 * width, width) if case in ("fc_fwd", "proj_dx") else (width, 4 * width)
    if shape is not None:                         # (N, K) other than the ViT-B/16 block's (tests/test_guard_bands_gpu.py)
        N, K = shape
    kr = case in ("proj_dx", "fc_dx")
    flags = {"fc_fwd": 1 | 2 | 16, "proj_fwd": 1 | 2 | 8, "proj_dx": 2 | 4 | 32, "fc_dx": 2 | 4}[case] | 64
    nrows = ops.gemm_tiles_m(M, N, K, flags, r, dt, True)
    assert nrows != ops.gemm_tiles_m(M, N, K, flags, r, dt, False), "shape does not select the panel kernel"
    a, b = rnd(M, K, dt=dt, scale=gscale if kr else 1.0, seed=70), rnd(N, K, dt=dt, scale=K ** -0.5, seed=71)
    P = rnd(K, r, scale=0.1, seed=73)
    S = rnd(G, r, seed=74)
    lw = rnd(N, r, seed=75) if kr else rnd(r, N, seed=75)
    rk = torch.zeros(16, K, device="cuda", dtype=dt)
    ops.PackPlan([(P, False, rk)], dt, "cuda").run()
    out = guard.out(M, N, dtype=dt)
    t, ts = guard.out(M, r), guard.out(M, r)
    kw, bwd = {}, kr
    t_fwd = rnd(M, r, seed=76) if bwd else None
    dsp = guard.out(nrows, G, r) if bwd else None
    ro = ops.RankOp(rk, S, attr, rps, 0.25, 0.7, t_out=t, ts_out=ts, t_fwd=t_fwd, ds_part=dsp)
    ref_t = a.double() @ P.to(dt).double()
    pi = mix(attr, G)
    rows = torch.arange(M, device="cuda") // rps
    pi_rows = pi[rows] if attr is not None else pi.expand(M, G)
    ref_ts = 0.25 * ref_t * (pi_rows @ S.double())
    # the kernel feeds ts to the matrix cores as bf16 (like the 128x128 kernel's MFMA update)
    ref = a.double() @ b.double().t() + ref_ts.to(dt).double() @ (lw.double().t() if kr else lw.double()).to(dt).double()
    if case in ("fc_fwd", "proj_fwd"):
        kw["bias"] = rnd(N, seed=72)
        ref = ref + kw["bias"].double()
    if case == "proj_fwd":
        kw["res"] = rnd(M, N, dt=dt, seed=77)
        ref = ref + kw["res"].double()
    rs_part = None
    if rowstats:                                     # FFM_EPI_ROWSTATS beside the c_proj forward: [tiles_n, M, 2], exactly
        assert case == "proj_fwd"
        tn = ops.gemm_tiles_n(M, N, K, flags | 128, r, dt, True)
        assert tn > 0, "no FFM_EPI_ROWSTATS kernel for this shape"
        rs_part = guard.out(tn, M, 2)
        kw["rowstats"] = rs_part
    act = None
    if case == "fc_fwd":
        act = guard.out(M, N, dtype=dt)
        kw["gelu_out"] = act
    if case == "proj_dx":
        kw["dgelu_aux"] = rnd(M, N, dt=dt, seed=78)
        x = kw["dgelu_aux"].double()
        sg = torch.sigmoid(1.702 * x)
        ref = ref * (x if deriv else sg * (1 + 1.702 * x * (1 - sg)))
        if deriv:
            kw["gelu_deriv"] = True
    ops.gemm_nt(a, b, out, lw=lw, lw_is_kr=kr, rankop=ro, b_packed=ops.pack_b(b), **kw)
    from types import SimpleNamespace
    res = SimpleNamespace(t=t, ts=ts, out=out, act=act, dsp=dsp, ref_t=ref_t, ref_ts=ref_ts, ref_out=ref, pi_rows=pi_rows,
                          t_fwd=t_fwd, attr=attr, rps=rps, scaling=0.25, dt=dt)
    if before_checks is not None:
        before_checks(res)
    check(t, ref_t, 2e-5, "t")
    check(ts, ref_ts, 2e-5, "ts")
    check(out, ref, tol(dt), "fused out")
    if act is not None:
        pre = out.double()
        check(act, pre * torch.sigmoid(1.702 * pre), tol(dt), "quick_gelu(pre)")
    if rs_part is not None:                          # sums of the STORED rows, as test_gemm_rowstats_partials holds them
        o, got = out.double(), rs_part.double().sum(0)
        check(got[:, 0], o.sum(1), 1e-5, "row sums")
        check(got[:, 1], (o * o).sum(1), 1e-5, "row sums of squares")
    if bwd:
        check(dsp.double().sum(0), pi_rows.t() @ (0.25 * t_fwd.double() * ref_t), 5e-5, "dS")
    guard.check()
    return res


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("M,r,G,use_attr", [(6304, 8, 3, True), (6250, 16, 2, False), (6304, 4, 3, True), (3000, 8, 3, True)])
@H16
def test_gemm_panel_lgrad_partials(ops, guard, M, r, G, use_attr, h16):
    """FFM_EPI_LGRAD: the dX product of c_proj also leaves the per-row-tile partial products of the two large rank-r
    gradient reductions of the block - dB(c_fc) = dpre^T ts1 from the rows it stores and dA(c_proj) = act^T us from
    quick_gelu(pre) and its own ts.  Held to float64 on the 16-bit tensors the kernel itself produced, and to the
    reduction kernel it replaces (ffm_lora_grad_partial); everything else the launch writes must not move."""
    rps = 197
    nsamp = (M + rps - 1) // rps
    attr = torch.randint(0, G, (nsamp,), device="cuda", dtype=torch.int32) if use_attr else None
    panel_lgrad_case(ops, guard, M, r, G, attr, rps, h16)


def panel_lgrad_case(ops, guard, M, r, G, attr, rps, dt, before_checks=None, shape=None, gscale=1.0):
    """Body of test_gemm_panel_lgrad_partials for a given attribute vector and rows per sample (`before_checks`: as in
    panel_fairlora_case, on the launch WITH the partial products).  gscale multiplies the gradient operand a = dL/dy."""
    width = 768
    N, K = shape if shape is not None else (4 * width, width)
    nlg = ops.gemm_lgrad_rows(M, N, K, r, dt, True)
    if nlg <= 0:
        pytest.skip("no FFM_EPI_LGRAD kernel for this shape (the engine then launches the reductions)")
    flags = 2 | 4 | 32 | 64
    nrows = ops.gemm_tiles_m(M, N, K, flags, r, dt, True)
    a, b = rnd(M, K, dt=dt, scale=gscale, seed=70), rnd(N, K, dt=dt, scale=K ** -0.5, seed=71)
    P, S, lw = rnd(K, r, scale=0.1, seed=73), rnd(G, r, seed=74), rnd(N, r, seed=75)
    rk = torch.zeros(16, K, device="cuda", dtype=dt)
    ops.PackPlan([(P, False, rk)], dt, "cuda").run()
    pre = rnd(M, N, dt=dt, seed=78)
    ts1 = rnd(M, r, seed=79)
    t_fwd = rnd(M, r, seed=76)
    bp = ops.pack_b(b)

    def run(lgrad):
        out = guard.out(M, N, dtype=dt)
        t, ts = guard.out(M, r), guard.out(M, r)
        dsp = guard.out(nrows, G, r)
        ro = ops.RankOp(rk, S, attr, rps, 0.25, 0.7, t_out=t, ts_out=ts, t_fwd=t_fwd, ds_part=dsp, lgrad=lgrad)
        ops.gemm_nt(a, b, out, lw=lw, lw_is_kr=True, rankop=ro, b_packed=bp, dgelu_aux=pre)
        return out, t, ts, dsp

    pc = guard.out(nlg, N, r)
    pa = guard.out(nlg, N, r)
    out, t, ts, dsp = run((ts1, pc, pa))
    out0, t0, ts0, dsp0 = run(None)
    if before_checks is not None:
        from types import SimpleNamespace
        ref_t = a.double() @ P.to(dt).double()
        rows = torch.arange(M, device="cuda") // rps
        pi = mix(attr, G)
        pi_rows = pi[rows] if attr is not None else pi.expand(M, G)
        before_checks(SimpleNamespace(t=t, ts=ts, out=None, act=None, dsp=dsp, ref_t=ref_t, ref_ts=0.25 * ref_t * (pi_rows @ S.double()),
                                      ref_out=None, pi_rows=pi_rows, t_fwd=t_fwd, attr=attr, rps=rps, scaling=0.25, dt=dt))
    assert torch.equal(out, out0) and torch.equal(t, t0) and torch.equal(ts, ts0) and torch.equal(dsp, dsp0)
    assert not torch.isnan(pc).any() and not torch.isnan(pa).any()
    x = pre.float()
    act = (x * torch.sigmoid(1.702 * x)).to(dt)                       # the forward's stored activation, to 16-bit rounding
    ref_c = out.double().t() @ ts1.double()
    ref_a = act.double().t() @ ts.double()
    check(pc.double().sum(0), ref_c, 2e-4, "dB(c_fc) partials")
    # (quick_gelu by v_exp / v_rcp: a 16-bit rounding flips here and there against torch's sigmoid)
    check(pa.double().sum(0), ref_a, 2e-3, "dA(c_proj) partials")
    ns = ops.lora_grad_splits(M)
    part = guard.out(ns * N * r)
    ops.lora_grad_partial(out, ts1, r, part)
    check(pc.double().sum(0), part.view(ns, N, r).double().sum(0), 2e-5, "against ffm_lora_grad_partial")
    guard.check()


@pytest.mark.mask_tolerant
@H16
def test_gemm_panel_lgrad_race_screen_bitwise_repeatable(ops, guard, h16):
    """The FFM_EPI_LGRAD epilogue lays two 16-bit images over the part of the wave's output stage it has already read and
    orders its LDS traffic by program order inside the wave (asm ds_write / ds_read_b64_tr_b16 between compiler-visible
    loads), its V tables by the block's barriers, its MFMA results by hand-placed wait states: a hazard there shows as a value
    that depends on timing.  Screen: the bench shape 24 times back to back, a cache-flushing write in front of every third
    launch, every output (the stored rows, t / ts, dS partials, both partial products) bit-identical to the first run's."""
    dt = h16
    M, r, G, width, rps = 6304, 8, 3, 768, 197
    N, K = 4 * width, width
    nlg = ops.gemm_lgrad_rows(M, N, K, r, dt, True)
    if nlg <= 0:
        pytest.skip("no LGRAD tile under this FFM_PANEL_MASK (the engine falls back to the two reduction launches)")
    nrows = ops.gemm_tiles_m(M, N, K, 2 | 4 | 32 | 64, r, dt, True)
    a, b = rnd(M, K, dt=dt, seed=170), rnd(N, K, dt=dt, scale=K ** -0.5, seed=171)
    P, S, lw = rnd(K, r, scale=0.1, seed=173), rnd(G, r, seed=174), rnd(N, r, seed=175)
    attr = torch.randint(0, G, ((M + rps - 1) // rps,), device="cuda", dtype=torch.int32)
    rk = torch.zeros(16, K, device="cuda", dtype=dt)
    ops.PackPlan([(P, False, rk)], dt, "cuda").run()
    pre, ts1, t_fwd, bp = rnd(M, N, dt=dt, seed=178), rnd(M, r, seed=179), rnd(M, r, seed=176), ops.pack_b(b)
    flush = torch.empty(320 << 20, device="cuda", dtype=torch.uint8)
    first = None
    for it in range(24):
        out = guard.out(M, N, dtype=dt)
        t, ts = guard.out(M, r), guard.out(M, r)
        dsp = guard.out(nrows, G, r)
        pc, pa = guard.out(nlg, N, r), guard.out(nlg, N, r)
        if it % 3 == 1:
            flush.fill_(it)
        ro = ops.RankOp(rk, S, attr, rps, 0.25, 0.7, t_out=t, ts_out=ts, t_fwd=t_fwd, ds_part=dsp, lgrad=(ts1, pc, pa))
        ops.gemm_nt(a, b, out, lw=lw, lw_is_kr=True, rankop=ro, b_packed=bp, dgelu_aux=pre)
        cur = (out, t, ts, dsp, pc, pa)
        if first is None:
            first = cur
            assert all(bool(torch.isfinite(x.float()).all()) for x in cur)
        else:
            for x, y, nm in zip(cur, first, ("out", "t", "ts", "dS", "part_c", "part_a")):
                assert torch.equal(x, y), f"run {it}: {nm} differs from run 0 in {int((x != y).sum())} elements"
    guard.check()


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_gemm_gelu_and_dgelu(ops, guard, dt):
    M, N, K = 260, 256, 128
    a, b = rnd(M, K, dt=dt, seed=9), rnd(N, K, dt=dt, scale=K ** -0.5 * 2, seed=10)
    bias = rnd(N, seed=11)
    pre = guard.out(M, N, dtype=dt)
    act = guard.out(M, N, dtype=dt)
    ops.gemm_nt(a, b, pre, bias=bias, gelu_out=act)
    ref_pre = a.double() @ b.double().t() + bias.double()
    check(pre, ref_pre, tol(dt), "pre")
    p = pre.double()
    check(act, p * torch.sigmoid(1.702 * p), tol(dt), "quick_gelu(pre)")
    # dgelu: out = (a b^T) * gelu'(aux)
    aux = rnd(M, N, dt=dt, seed=12)
    out = guard.out(M, N, dtype=dt)
    ops.gemm_nt(a, b, out, dgelu_aux=aux)
    x = aux.double()
    s = torch.sigmoid(1.702 * x)
    check(out, (a.double() @ b.double().t()) * (s * (1 + 1.702 * x * (1 - s))), tol(dt), "dgelu")
    guard.check()


# ------------------------------------------------------------- LayerNorm ---
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("rows,width", [(6304, 768), (308, 512), (37, 128), (5, 2048)])
def test_layernorm_fwd_bwd(ops, guard, dt, rows, width):
    layernorm_case(ops, guard, dt, rows, width)


def layernorm_case(ops, guard, dt, rows, width, gscale=1.0):
    # gscale multiplies the two gradient operands of the backward, dy and res
    x = rnd(rows, width, dt=dt, seed=13) * 2 + 0.5
    gamma, beta = 1 + 0.1 * rnd(width, seed=14), 0.1 * rnd(width, seed=15)
    y = guard.like(x)
    mean = guard.out(rows)
    rstd = guard.out(rows)
    ops.layernorm_fwd(x, y, gamma, beta, mean, rstd)
    xd = x.double().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xd, (width,), gamma.double(), beta.double(), 1e-5)
    check(y, ref.detach(), tol(dt), "ln fwd")
    check(mean, x.double().mean(1), 1e-5, "mean")
    dy = rnd(rows, width, dt=dt, scale=gscale, seed=16)
    res = rnd(rows, width, dt=dt, scale=gscale, seed=17)
    ref.backward(dy.double())
    out = guard.like(x)
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, res, out)
    check(out, xd.grad + res.double(), tol(dt), "ln bwd + res")
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, None, out)
    check(out, xd.grad, tol(dt), "ln bwd")
    guard.check()


# ---------------------------------------------------- patchify / embed ----
@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_patchify_and_embed(ops, guard, dt):
    patchify_and_embed_case(ops, guard, dt, 3)


def patchify_and_embed_case(ops, guard, dt, B, rowsums=False):
    H, ps, width = 64, 16, 128
    img = torch.rand(B, 3, H, H, device="cuda") * 255
    mean3, std3 = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
    P = (H // ps) ** 2
    cols = guard.out(B * P, 3 * ps * ps, dtype=dt)
    ops.patchify(img, cols, ps, mean3, std3)
    x = (img / 255.0 - torch.tensor(mean3, device="cuda").view(1, 3, 1, 1)) / torch.tensor(std3, device="cuda").view(1, 3, 1, 1)
    ref = torch.nn.functional.unfold(x, kernel_size=ps, stride=ps).transpose(1, 2).reshape(B * P, -1)
    check(cols, ref, 1e-6 if dt == torch.float32 else 8e-3, "patchify")
    # conv1 as a GEMM over the gathered patches == F.conv2d
    w = rnd(width, 3, ps, ps, scale=0.02, seed=18)
    out = guard.out(B * P, width, dtype=dt)
    ops.gemm_nt(cols, w.reshape(width, -1).to(dt), out)
    conv = torch.nn.functional.conv2d(x.double(), w.to(dt).double(), stride=ps).reshape(B, width, P).permute(0, 2, 1)
    check(out, conv.reshape(B * P, width), tol(dt) * 2, "patch-embed")
    # token assembly + ln_pre
    cls, pos = rnd(width, dt=dt, scale=0.1, seed=19), rnd(P + 1, width, dt=dt, scale=0.1, seed=20)
    gamma, beta = 1 + 0.1 * rnd(width, seed=21), 0.1 * rnd(width, seed=22)
    xt = guard.out(B * (P + 1), width, dtype=dt)
    rs = guard.out(B * (P + 1), 2) if rowsums else None
    ops.embed_lnpre(out, cls, pos, gamma, beta, xt, B, P + 1, rowstat=rs)
    tok = torch.cat([cls.to(dt).expand(B, 1, width), out.reshape(B, P, width)], 1) + pos
    ref = torch.nn.functional.layer_norm(tok.double(), (width,), gamma.double(), beta.double(), 1e-5)
    check(xt, ref.reshape(-1, width), tol(dt), "embed+ln_pre")
    if rowsums:                                        # {sum, sum of squares} of every output row AS STORED (include/ffm_hip.h)
        check(rs[:, 0], xt.double().sum(1), 1e-5, "row sums")
        check(rs[:, 1], (xt.double() ** 2).sum(1), 1e-5, "row sums of squares")
    guard.check()



# ------------------------------------------------- 3D OCT slice front end ---
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("N,D,H,ps,width", [(4, 4, 64, 16, 128), (3, 8, 96, 16, 256), (2, 2, 224, 16, 768),
                                            (2, 16, 32, 8, 64),      # MAXD slices per group, one strip, ragged row blocks
                                            (2, 5, 40, 8, 64),       # a slice count that is no multiple of the 4 waves
                                            (1, 8, 224, 16, 768)])   # the bench geometry: 16 x 14-row / 4 x 56-row blocks
def test_slice3d_front_end(ops, guard, dt, N, D, H, ps, width):
    slice3d_case(ops, guard, dt, N, D, H, ps, width)


def slice3d_case(ops, guard, dt, N, D, H, ps, width, gscale=1.0):
    """conv5x5 + per-image min-max + patchify, and their backward down to the conv weight/bias gradient,
    against torch autograd in fp64 (trainers/GLP_OT_SVLoRA.py:681-693).  gscale multiplies the gradient operand dcols."""
    F = torch.nn.functional
    img = torch.rand(1, N * D, H, H, device="cuda", generator=torch.Generator("cuda").manual_seed(31)) * 255
    w = rnd(3, D, 5, 5, scale=D ** -0.5, seed=32)
    b = rnd(3, scale=0.1, seed=33)
    mean3, std3 = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
    P = (H // ps) ** 2
    nblk = ops.slice_blocks(H, H)
    conv = guard.out(N, 3, H, H)
    mm_part = guard.scratch(N * nblk * 2)
    mnmx = guard.out(N, 2)
    cnt = guard.out(N, 2, dtype=torch.int32)
    cols = guard.out(N * P, 3 * ps * ps, dtype=dt)
    ops.slice_conv_fwd(img, w, b, conv, mm_part, mnmx, cnt, D)
    ops.patchify_minmax(conv, mnmx, cnt, cols, ps, mean3, std3)

    wd, bd = w.double().requires_grad_(), b.double().requires_grad_()
    x = (img.double() / 255.0).reshape(-1, D, H, H)
    c = F.conv2d(x, wd, bd, padding=2)
    mn, mx = c.amin(dim=(1, 2, 3), keepdim=True), c.amax(dim=(1, 2, 3), keepdim=True)
    y = (c - mn) / (mx - mn + 1e-5)
    z = (y - torch.tensor(mean3, device="cuda", dtype=torch.float64).view(1, 3, 1, 1)) \
        / torch.tensor(std3, device="cuda", dtype=torch.float64).view(1, 3, 1, 1)
    ref_cols = F.unfold(z, kernel_size=ps, stride=ps).transpose(1, 2).reshape(N * P, -1)
    check(conv, c.detach(), 2e-6, "slice conv")
    check(mnmx[:, 0], mn.flatten().detach(), 2e-6, "min")
    check(mnmx[:, 1], mx.flatten().detach(), 2e-6, "max")
    check(cols, ref_cols.detach(), 2e-5 if dt == torch.float32 else 8e-3, "patchify_minmax")
    # random floats: one pixel attains each extremum.  Tied extrema (black borders, blank slices, saturated regions: counts
    # in the thousands, gradients divided by them) and H != W are tests/test_slice3d_ties_gpu.py
    assert cnt.tolist() == [[1, 1]] * N

    dcols = rnd(N * P, 3 * ps * ps, dt=dt, scale=gscale, seed=34)
    ref_cols.backward(dcols.double())
    dconv = guard.scratch(*conv.shape)                                # (scratch by the header: bands only)
    ab_part = guard.scratch(N * ops.slice_bwd_ab_blocks() * 2)
    gmm = guard.scratch(N, 2)
    nw = 3 * D * 25 + 3
    nwb = ops.slice_wgrad_blocks(H, H)
    wpart = guard.out(N * nwb * nw)          # every entry must be written
    ops.slice_bwd(dcols, img, conv, mnmx, cnt, dconv, ab_part, gmm, wpart, D, ps, std3)
    got = guard.out(nw)
    ops.reduce_partials(wpart, N * nwb, nw, got)
    check(got[:nw - 3].reshape(3, D, 5, 5), wd.grad, 2e-4, "slice conv dW")
    check(got[nw - 3:], bd.grad, 2e-4, "slice conv dbias")
    guard.check()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("B,P,width", [(3, 16, 128), (2, 196, 768), (2, 9, 1024), (2, 9, 1536)])
def test_embed_lnpre_bwd(ops, guard, dt, B, P, width):
    embed_lnpre_bwd_case(ops, guard, dt, B, P, width)


def embed_lnpre_bwd_case(ops, guard, dt, B, P, width, gscale=1.0):
    patch = rnd(B * P, width, dt=dt, seed=41)
    cls, pos = rnd(width, dt=dt, scale=0.1, seed=42), rnd(P + 1, width, dt=dt, scale=0.1, seed=43)
    gamma, beta = 1 + 0.1 * rnd(width, seed=44), 0.1 * rnd(width, seed=45)
    dx = rnd(B * (P + 1), width, dt=dt, scale=gscale, seed=46)              # the gradient operand
    pd = patch.double().requires_grad_()
    tok = torch.cat([cls.double().expand(B, 1, width), pd.reshape(B, P, width)], 1) + pos.double()
    y = torch.nn.functional.layer_norm(tok, (width,), gamma.double(), beta.double(), 1e-5)
    y.backward(dx.double().reshape(B, P + 1, width))
    dpatch = guard.like(patch)
    ops.embed_lnpre_bwd(dx, patch, pos, gamma, dpatch, B, P + 1)
    check(dpatch, pd.grad, tol(dt), "embed+ln_pre backward")
    guard.check()


# ------------------------------------------------------------- attention ---
def ref_attention(qkv, B, L, heads, causal):
    E = heads * 64
    q, k, v = qkv.double().reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    if causal:
        s = s + torch.full((L, L), float("-inf"), device=qkv.device, dtype=torch.float64).triu_(1)
    p = torch.softmax(s, -1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B * L, E)
    return o, torch.logsumexp(s, -1)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("B,L,heads,causal", [(2, 17, 2, False), (3, 197, 12, False), (4, 77, 8, True), (2, 64, 1, False),
                                               (1, 256, 2, True)])
def test_attention_fwd_bwd(ops, guard, dt, B, L, heads, causal):
    attention_case(ops, guard, dt, B, L, heads, causal)


def attention_case(ops, guard, dt, B, L, heads, causal, whole_gradient=False, gscale=1.0):
    E = heads * 64
    qkv = rnd(B * L, 3 * E, dt=dt, seed=23)
    out = guard.out(B * L, E, dtype=dt)
    lse = guard.out(B, heads, L)
    ops.attention_fwd(qkv, out, lse, B, L, heads, causal)
    qd = qkv.double().requires_grad_(True)
    ref, ref_lse = ref_attention(qd, B, L, heads, causal)
    check(out, ref.detach(), tol(dt), "attn out")
    check(lse, ref_lse.detach(), 1e-5 if dt == torch.float32 else 2e-3, "lse")
    dout = rnd(B * L, E, dt=dt, scale=gscale, seed=24)                 # the gradient operand
    ref.backward(dout.double())
    dqkv = guard.out(B * L, 3 * E, dtype=dt)
    delta = guard.scratch(B, heads, L)                                # (scratch by the header: bands only)
    ops.attention_bwd(qkv, out, dout, lse, delta, dqkv, B, L, heads, causal)
    t = tol(dt) * (1 if dt == torch.float32 else 2)
    if whole_gradient:
        # one token: dq and dk are exactly zero (softmax of one score), so they have no scale of their own - held to dv's
        check(dqkv, qd.grad, t, "dqkv")
        assert float(qd.grad[:, :2 * E].abs().max()) == 0.0                  # (the reference's dq, dk: exactly zero)
        # ... the kernels form dP and delta in different summation orders, so theirs are zero to rounding: an absolute bound
        assert float(dqkv[:, :2 * E].double().abs().max()) <= t * float(qd.grad[:, 2 * E:].abs().max()), "dq / dk at one token"
        guard.check()
        return
    check(dqkv[:, :E], qd.grad[:, :E], t, "dq")
    check(dqkv[:, E:2 * E], qd.grad[:, E:2 * E], t, "dk")
    check(dqkv[:, 2 * E:], qd.grad[:, 2 * E:], t, "dv")
    guard.check()


# ------------------------------------------------------------------ LoRA ---
def mix(attr, G, lam=0.7):
    """pi_b in float64; a value outside [0, G) is "unknown" and takes the uniform row of attr=None."""
    if attr is None:
        return torch.full((1, G), 1.0 / G, device="cuda", dtype=torch.float64)
    a = attr.long()
    known = (a >= 0) & (a < G)
    oh = torch.nn.functional.one_hot(torch.where(known, a, torch.zeros_like(a)), G).double()
    pi = oh * lam + (1 - oh) * (1 - lam) / (G - 1)
    return torch.where(known[:, None], pi, torch.full_like(pi, 1.0 / G))


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,K,r,G,rps,rk,use_attr", [(1000, 768, 8, 3, 197, False, True), (333, 3072, 16, 3, 50, True, True),
                                                      (70, 128, 4, 2, 17, False, False), (300, 256, 32, 3, 100, True, True),
                                                      (300, 256, 12, 3, 100, False, True),
                                                      # bf16 + [r, K] rows + >= 1024 rows: the matrix-core kernel (the step's last
                                                      # down projection, u = dpre B_fc^T), ragged last block, 1..16 rank slots
                                                      (6304, 3072, 8, 3, 197, True, True), (2000, 768, 16, 2, 50, True, False),
                                                      (1030, 512, 5, 3, 197, True, True)])
def test_lora_down(ops, guard, dt, M, K, r, G, rps, rk, use_attr):
    lora_down_case(ops, guard, dt, M, K, r, G, rps, rk, use_attr)


def lora_down_case(ops, guard, dt, M, K, r, G, rps, rk, use_attr, gscale=1.0):
    x = rnd(M, K, dt=dt, scale=gscale, seed=25)                        # (the backward's u = g B^T: x is dL/dy, t_fwd the forward's t)
    P = rnd(r, K, scale=0.1, seed=26) if rk else rnd(K, r, scale=0.1, seed=26)
    S = rnd(G, r, seed=27)
    nsamp = (M + rps - 1) // rps
    attr = torch.randint(0, G, (nsamp,), device="cuda", dtype=torch.int32) if use_attr else None
    t = guard.out(M, r)
    ts = guard.out(M, r)
    t_fwd = rnd(M, r, seed=28)
    nb = ops.lora_down_blocks(M, K, r, dt)
    ds_part = guard.out(nb, G, r)
    ops.lora_down(x, P, rk, S, attr, r, G, rps, 0.25, 0.7, t, ts, t_fwd, ds_part)
    Pq = P.to(dt).double()                         # the kernel keeps P in the activation dtype in LDS
    Pm = Pq.t() if rk else Pq
    ref_t = x.double() @ Pm
    pi = mix(attr, G)
    sample = torch.arange(M, device="cuda") // rps
    pi_rows = pi[sample] if attr is not None else pi.expand(M, G)
    sb = pi_rows @ S.double()
    check(t, ref_t, 2e-5, "t")                      # fp32 accumulate of exact products in both dtypes
    check(ts, 0.25 * ref_t * sb, 2e-5, "ts")
    ref_ds = pi_rows.t() @ (0.25 * t_fwd.double() * ref_t)
    check(ds_part.double().sum(0), ref_ds, 5e-5, "dS")
    guard.check()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,K,r", [(1000, 768, 8), (197, 3072, 16), (64, 128, 4), (130, 264, 32)])
def test_lora_grad(ops, guard, dt, M, K, r):
    lora_grad_case(ops, guard, dt, M, K, r)


def lora_grad_case(ops, guard, dt, M, K, r, gscale=1.0, grad="v"):
    # the gradient operand: v in dA = x^T us, x in dB = g^T ts (fairfedmed_amd/lora_site.py)
    x = rnd(M, K, dt=dt, scale=gscale if grad == "x" else 1.0, seed=29)
    v = rnd(M, r, scale=gscale if grad == "v" else 1.0, seed=30)
    ns = ops.lora_grad_splits(M)
    part = guard.out(ns, K, r)
    ops.lora_grad_partial(x, v, r, part)
    ref = x.double().t() @ v.double()
    out = guard.out(K, r)
    ops.reduce_partials(part, ns, K * r, out)
    check(out, ref, 3e-5, "dA-style [K,r]")
    out_t = guard.out(r, K)
    ops.reduce_partials(part, ns, K * r, out_t, transpose_K=K, transpose_r=r)
    check(out_t, ref.t(), 3e-5, "dB-style [r,K]")
    ops.reduce_partials(part, ns, K * r, out, accumulate=True)
    check(out, 2 * ref, 3e-5, "accumulate")
    # the batched form (one launch for many tensors)
    o1, o2 = guard.out(K, r), guard.out(r, K)
    plan = ops.ReducePlan([(part, ns, K * r, o1, 0, 0), (part, ns, K * r, o2, K, r)], "cuda")
    plan.run()
    check(o1, ref, 3e-5, "multi [K,r]")
    check(o2, ref.t(), 3e-5, "multi [r,K]")
    guard.check()


# ------------------------------------------------------------------ head ---
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("B,L,D,S", [(8, 197, 512, 1), (6, 17, 128, 2)])
def test_head_and_loss(ops, guard, dt, B, L, D, S):
    head_and_loss_case(ops, guard, dt, B, L, D, S)


def head_and_loss_case(ops, guard, dt, B, L, D, S, n_cls=2, zero_row=None, gscale=1.0):
    f = rnd(B * L, D, dt=dt, seed=31)
    if zero_row is not None:
        f[zero_row] = 0                                               # the 1e-12 clamp of F.normalize, forward and backward
    tbar = rnd(n_cls, D, scale=D ** -0.5, seed=32)
    ls = torch.tensor([math.log(1 / 0.07)], device="cuda")
    fbar = guard.out(B, D)
    rnorm = guard.out(B * L)
    logits_img = guard.out(B, n_cls)
    ops.head_fwd(f, tbar, ls, fbar, rnorm, logits_img, B, L, n_cls)
    fd = f.double().requires_grad_(True)
    td = tbar.double().requires_grad_(True)
    feats = torch.nn.functional.normalize(fd.reshape(B, L, D)[:, 1:], dim=2)
    ref_img = ls.double().exp() * torch.einsum("bmd,cd->bc", feats, td) / (L - 1)
    check(logits_img, ref_img.detach(), 2e-5 if dt == torch.float32 else 1e-4, "logits_img")
    nb = B // S
    label = torch.randint(0, n_cls, (nb,), device="cuda")
    logits = guard.out(nb, n_cls)
    prob = guard.out(nb, n_cls)
    loss = guard.out(1)
    dl = guard.out(B, n_cls)
    fin = guard.out(1, dtype=torch.int32)
    ops.ce_loss(logits_img, label, logits, prob, loss, dl, fin, nb, S, n_cls)
    ref_logits = ref_img.reshape(nb, S, n_cls).mean(1)
    ref_loss = torch.nn.functional.cross_entropy(ref_logits, label)
    check(logits, ref_logits.detach(), 2e-5 if dt == torch.float32 else 1e-4, "logits")
    assert abs(float(loss) - float(ref_loss)) <= 2e-5 * abs(float(ref_loss)) + (0 if dt == torch.float32 else 1e-4)
    assert int(fin) == 1
    check(prob, torch.softmax(ref_logits, -1).detach(), 1e-4, "prob")
    (ref_loss * gscale).backward()
    if gscale != 1.0:
        dl.mul_(gscale)                                              # the engine's ffm_loss_scale on dL/dlogits
    df = guard.like(f)
    dtbar = guard.like(tbar)
    ops.head_bwd(f, tbar, ls, fbar, rnorm, dl, df, dtbar, B, L, n_cls)
    t_df = 2e-4 if dt == torch.float32 else 1.5e-2
    if zero_row is None:
        check(df, fd.grad, t_df, "df")
    else:
        # the clamped row's gradient is dL/dy / 1e-12: held on its own (it would set the scale for every other row), and where
        # it does not fit the storage type (IEEE half) it must be the infinity the rounded reference is
        rows = torch.ones(B * L, dtype=torch.bool, device="cuda")
        rows[zero_row] = False
        check(df[rows], fd.grad[rows], t_df, "df of the other rows")
        want = fd.grad[zero_row].to(dt)
        inf = torch.isinf(want)
        assert torch.equal(df[zero_row][inf], want[inf]), "df of the all-zero row where 1e12 dL/dy overflows the storage type"
        if bool((~inf).any()):
            check(df[zero_row][~inf], fd.grad[zero_row][~inf], t_df, "df of the all-zero row")
    check(dtbar, td.grad, 2e-4 if dt == torch.float32 else 1e-3, "dtbar")
    guard.check()


# ----------------------------------------------------------- optimizer ----
def test_sgd_matches_torch(ops):
    n = 741952
    p = rnd(n, seed=33)
    ref_p = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([ref_p], lr=1e-3, momentum=0.9, weight_decay=5e-4)
    buf = torch.zeros(n, device="cuda")
    for step in range(3):
        g = rnd(n, seed=34 + step)
        ref_p.grad = g.clone()
        opt.step()
        ops.sgd_momentum(p, g, buf, 1e-3, 0.9, 5e-4, step == 0)
        check(p, ref_p.detach(), 1e-6, f"sgd step {step}")


def test_fedavg_aggregator_gpu_equals_cpu():
    """fedavg.FedAvgAggregator (the ONE round boundary of the FL rank driver and of bench.py): a rank that holds two clients of
    a round - begin / add / add / finish - on the HIP kernels against the host-tensor path the gloo tests run.  The weighted sum
    (ffm_scale_by, ffm_scale_acc: product and sum rounded separately, compiled without FMA contraction) is BIT-identical; behind
    shared_half_s and the EMA the two agree to one rounding of the (1 - beta) coefficient (the host forms it in double)."""
    from fairfedmed_amd.fedavg import FedAvgAggregator
    G, r = 3, 8
    offsets = {"prompt_learner.ctx": (0, (2, 4, 16)), "a.lora_S.weight": (128, (G, r)), "a.lora_A.weight": (152, (40, r)),
               "b.lora_S.weight": (472, (G, r)), "b.lora_S_global.weight": (496, (r,))}
    n = 504
    g = torch.Generator().manual_seed(7)
    flat0 = torch.randn(n, generator=g)
    clients = [torch.randn(n, generator=g) for _ in range(4)]
    n_client, by_attr = [40, 80], [[10, 20, 10], [30, 25, 25]]
    res = {}
    for dev in ("cpu", "cuda"):
        agg = FedAvgAggregator(flat0.to(dev).clone(), offsets, G, r, shared_half_s=True)
        sums, outs = [], []
        for rnd in range(2):
            agg.begin()
            agg.add(clients[2 * rnd].to(dev), 0, [0, 1], n_client, by_attr)
            agg.add(clients[2 * rnd + 1].to(dev), 1, [0, 1], n_client, by_attr)
            sums.append(agg.buf.cpu().clone())
            outs.append(agg.finish(rnd, 2, grouped=True).cpu().clone())
        res[dev] = (sums, outs)
    for a, b in zip(res["cpu"][0], res["cuda"][0]):
        assert torch.equal(a, b), "the weighted sum of a rank's clients: bit-identical"
    for a, b in zip(res["cpu"][1], res["cuda"][1]):
        assert float((a - b).abs().max()) <= 2e-7 * float(a.abs().max())
    assert not torch.equal(res["cpu"][1][0], res["cpu"][1][1])
    # the [G, r] blocks' first half is the column mean on every device, the 1-D lora_S_global is left alone
    blk = res["cuda"][1][0][128:128 + G * r].view(G, r)
    assert torch.equal(blk[0, : r // 2], blk[1, : r // 2]) and not torch.equal(blk[0, r // 2:], blk[1, r // 2:])


def test_fedavg_helpers(ops, guard):
    G, r, n = 3, 8, 1000
    p, w = rnd(n, seed=40), torch.rand(n, device="cuda")
    out = guard.out(n)
    ops.scale_by(p, w, out)
    assert torch.allclose(out, p * w)
    # the second client of a rank: acc += p2 * w2 with the product and the sum rounded separately (bit-exact vs torch)
    p2, w2 = rnd(n, seed=44), torch.rand(n, device="cuda")
    ref_acc = out + p2 * w2
    ops.scale_acc(p2, w2, out)
    assert torch.equal(out, ref_acc)
    avg, prev = rnd(n, seed=41), rnd(n, seed=42)
    offs = torch.tensor([100, 500], device="cuda", dtype=torch.int64)
    ref = avg.clone()
    for o in (100, 500):
        blk = ref[o:o + G * r].view(G, r)
        blk[:, : r // 2] = blk[:, : r // 2].mean(0, keepdim=True)
    ref = (1 - 0.3) * ref + 0.3 * prev
    res = guard.out(n)
    ops.fedavg_finish(avg, prev, res, offs, G, r, True, 0.3)
    check(res, ref, 1e-6, "fedavg_finish")
    # in place on the previous global (what FedAvgAggregator.finish does): same values
    prev2 = prev.clone()
    ops.fedavg_finish(avg.clone(), prev2, prev2, offs, G, r, True, 0.3)
    assert torch.equal(prev2, res)
    guard.check()


def test_casts(ops):
    x = rnd(37, 53, seed=43)
    assert torch.equal(ops.cast_from_f32(x, torch.bfloat16), x.to(torch.bfloat16))
    assert torch.equal(ops.cast_to_f32(x.to(torch.bfloat16)), x.to(torch.bfloat16).float())
    assert torch.equal(ops.transpose_cast(x, torch.bfloat16), x.t().contiguous().to(torch.bfloat16))
    assert torch.equal(ops.transpose_cast(x, torch.float32), x.t().contiguous())


def test_casts_half(ops):
    """test_casts in IEEE half: the three casts of the half twin (a cast is one rounding, so the results are exact)."""
    x = rnd(37, 53, seed=43)
    assert torch.equal(ops.cast_from_f32(x, torch.float16), x.to(torch.float16))
    assert torch.equal(ops.cast_to_f32(x.to(torch.float16)), x.to(torch.float16).float())
    assert torch.equal(ops.transpose_cast(x, torch.float16), x.t().contiguous().to(torch.float16))


@pytest.mark.parametrize("M,N,K", [(40, 1536, 512), (40, 512, 2048), (40, 2048, 512), (1, 512, 128), (64, 128, 128),
                                   (33, 48, 640), (8, 512, 512)])
@pytest.mark.parametrize("mode", ["plain", "bias", "bias_res", "bias_gelu", "dgelu"])
def test_skinny_gemm_text_tower_shapes(guard, M, N, K, mode):
    """gemm_skinny.hip (M <= 64 rows, bf16): the text tower's products and epilogues against fp32 PyTorch on the same
    bf16 operands; split-K over four waves must not change the result beyond fp32 summation order."""
    from fairfedmed_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M * 1000 + N + K)
    a = (torch.randn(M, K, device="cuda", generator=g)).to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
    aux = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
    out = guard.out(M, N, dtype=torch.bfloat16)
    act = guard.out(M, N, dtype=torch.bfloat16) if mode == "bias_gelu" else None                    # (the second output exists under the GELU epilogue only)
    ref = a.float() @ w.float().t()
    rel = lambda got, want: float((got.double() - want.double()).abs().max() / want.double().abs().max())
    if mode == "plain":
        ops.gemm_nt(a, w, out)
    elif mode == "bias":
        ops.gemm_nt(a, w, out, bias=bias)
        ref = ref + bias
    elif mode == "bias_res":
        ops.gemm_nt(a, w, out, bias=bias, res=res)
        ref = ref + bias + res.float()
    elif mode == "bias_gelu":
        ops.gemm_nt(a, w, out, bias=bias, gelu_out=act)
        ref = ref + bias
        assert rel(act.float(), ref * torch.sigmoid(1.702 * ref)) < 1e-2
    else:
        ops.gemm_nt(a, w, out, dgelu_aux=aux)
        x = aux.float()
        s = torch.sigmoid(1.702 * x)
        ref = ref * (s * (1 + 1.702 * x * (1 - s)))
    assert rel(out.float(), ref) < 1e-2                              # bf16 rounding of the output only
    guard.check()


@pytest.mark.parametrize("M,N,K", [(33, 48, 640), (8, 512, 512)], ids=["4waves", "8waves"])
@pytest.mark.parametrize("mode", ["plain", "bias", "bias_res", "bias_gelu", "dgelu"])
def test_skinny_gemm_half(guard, M, N, K, mode):
    """test_skinny_gemm_text_tower_shapes in IEEE half (the half twin of gemm_skinny.hip), at its two smallest shapes that
    take the four-wave and the eight-wave split of K; fp64 reference on the same half operands, bound tol(float16)."""
    from fairfedmed_amd import ops
    dt = torch.float16
    g = torch.Generator(device="cuda").manual_seed(M * 1000 + N + K)
    a = (torch.randn(M, K, device="cuda", generator=g)).to(dt)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(dt)
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M, N, device="cuda", generator=g).to(dt)
    aux = torch.randn(M, N, device="cuda", generator=g).to(dt)
    out = guard.out(M, N, dtype=dt)
    act = guard.out(M, N, dtype=dt) if mode == "bias_gelu" else None
    ref = a.double() @ w.double().t()
    if mode == "plain":
        ops.gemm_nt(a, w, out)
    elif mode == "bias":
        ops.gemm_nt(a, w, out, bias=bias)
        ref = ref + bias
    elif mode == "bias_res":
        ops.gemm_nt(a, w, out, bias=bias, res=res)
        ref = ref + bias + res.double()
    elif mode == "bias_gelu":
        ops.gemm_nt(a, w, out, bias=bias, gelu_out=act)
        ref = ref + bias
        check(act, ref * torch.sigmoid(1.702 * ref), tol(dt), "gelu")
    else:
        ops.gemm_nt(a, w, out, dgelu_aux=aux)
        x = aux.double()
        s = torch.sigmoid(1.702 * x)
        ref = ref * (s * (1 + 1.702 * x * (1 - s)))
    check(out, ref, tol(dt), "skinny " + mode)
    guard.check()


@pytest.mark.parametrize("M,N,K", [(40, 1536, 512), (40, 512, 2048), (40, 2048, 512), (1, 512, 128), (64, 128, 128),
                                   (33, 48, 640), (8, 512, 512)])
@pytest.mark.parametrize("x3", [True, False, "w16"], ids=["x3", "exact", "x3w16"])
@pytest.mark.parametrize("mode", ["plain", "bias", "bias_res", "bias_gelu", "dgelu"])
def test_skinny_gemm_f32(guard, M, N, K, x3, mode):
    """The text tower's products in float32 (engine.py: always, also beside a bf16 vision tower): FFM_F32_X3 (operands
    split into bf16 hi + lo pairs, three MFMAs at the bf16 rate), the same on a weight stored as IEEE half
    (FFM_F32_X3_W16: the half value is split exactly, so the reference is float64 on the ROUNDED weight at the same
    tolerance) and the exact f32 MFMA, 4 or 8 waves splitting K.  Reference: float64 on the same operands."""
    from fairfedmed_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M * 1000 + N + K)
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
    if x3 == "w16":
        w, x3 = w.half(), True
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M, N, device="cuda", generator=g)
    aux = torch.randn(M, N, device="cuda", generator=g)
    out = guard.out(M, N)
    act = guard.out(M, N) if mode == "bias_gelu" else None
    ref = a.double() @ w.double().t()
    rel = lambda got, want: float((got.double() - want.double()).abs().max() / want.double().abs().max())
    # hi + lo keeps 16 significant bits of every operand (2^-16 per product, the lo*lo term is dropped); after the sum
    # over K the result is far below that
    tol = 2e-5 if x3 else 2e-6
    if mode == "plain":
        ops.gemm_nt(a, w, out, x3=x3)
    elif mode == "bias":
        ops.gemm_nt(a, w, out, bias=bias, x3=x3)
        ref = ref + bias
    elif mode == "bias_res":
        ops.gemm_nt(a, w, out, bias=bias, res=res, x3=x3)
        ref = ref + bias + res.double()
    elif mode == "bias_gelu":
        ops.gemm_nt(a, w, out, bias=bias, gelu_out=act, x3=x3)
        ref = ref + bias
        assert rel(act, ref * torch.sigmoid(1.702 * ref)) < max(tol, 1e-5)
    else:
        ops.gemm_nt(a, w, out, dgelu_aux=aux, x3=x3)
        x = aux.double()
        s = torch.sigmoid(1.702 * x)
        ref = ref * (s * (1 + 1.702 * x * (1 - s)))
        tol = max(tol, 1e-5)
    assert not torch.isnan(out).any()
    assert rel(out, ref) < tol, rel(out, ref)
    guard.check()


@pytest.mark.parametrize("M,N,K", [(40, 512, 2048), (40, 512, 1536), (40, 2048, 512), (40, 1536, 512), (33, 512, 1024), (48, 256, 2048), (1, 512, 2048)])
@pytest.mark.parametrize("w16", [False, True], ids=["x3", "x3w16"])
@pytest.mark.parametrize("mode", ["plain", "bias", "bias_res", "bias_gelu", "dgelu"])
def test_skinny_gemm_split_over_k(guard, M, N, K, w16, mode):
    """ffm_gemm_args.sk_part (ABI 12): the text tower's narrow products split over K across the grid - partial tiles per
    128-deep slice, summed in slice order by the finish launch with the one-launch kernel's epilogues.  Against float64 at the
    X3 tolerance, bit-identical from run to run (no atomics), and the scratch query says which products are split."""
    from fairfedmed_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M * 1000 + N + K)
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
    if w16:
        w = w.half()
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M, N, device="cuda", generator=g)
    aux = torch.randn(M, N, device="cuda", generator=g)
    need = ops.gemm_splitk_floats(M, N, K, w16)
    assert need == (K // 128) * M * N and ops.gemm_splitk_floats(M, 4096, 512, w16) == 0 and ops.gemm_splitk_floats(64, N, K, w16) == 0 and ops.gemm_splitk_floats(M, N, 256, w16) == 0
    part = guard.scratch(need)                                         # exactly the queried size; partial tiles: scratch
    rel = lambda got, want: float((got.double() - want.double()).abs().max() / want.double().abs().max())
    ref = a.double() @ w.double().t()
    outs = []
    for _ in range(2):
        out = guard.out(M, N)
        act = guard.out(M, N) if mode == "bias_gelu" else None
        kw = {"plain": {}, "bias": dict(bias=bias), "bias_res": dict(bias=bias, res=res), "bias_gelu": dict(bias=bias, gelu_out=act),
              "dgelu": dict(dgelu_aux=aux)}[mode]
        ops.gemm_nt(a, w, out, x3=True, sk_part=part, **kw)
        outs.append((out, act))
    assert torch.equal(outs[0][0], outs[1][0])
    out, act = outs[0]
    tol = 2e-5
    if mode in ("bias", "bias_res", "bias_gelu"):
        ref = ref + bias
    if mode == "bias_res":
        ref = ref + res.double()
    if mode == "bias_gelu":
        assert rel(act, ref * torch.sigmoid(1.702 * ref)) < tol
    if mode == "dgelu":
        x = aux.double()
        sg = torch.sigmoid(1.702 * x)
        ref = ref * (sg * (1 + 1.702 * x * (1 - sg)))
    assert not torch.isnan(out).any()
    assert rel(out, ref) < tol, rel(out, ref)
    # the one-launch kernel on the same operands: same value to the fp32 summation order
    one = guard.like(out)
    kw = {"plain": {}, "bias": dict(bias=bias), "bias_res": dict(bias=bias, res=res), "bias_gelu": dict(bias=bias, gelu_out=guard.like(out) if mode == "bias_gelu" else None),
          "dgelu": dict(dgelu_aux=aux)}[mode]
    ops.gemm_nt(a, w, one, x3=True, **kw)
    assert rel(out, one) < 5e-6
    guard.check()


@pytest.mark.parametrize("M,r,G,use_attr", [(6304, 8, 3, True), (6250, 12, 2, False), (6304, 16, 3, True), (5000, 4, 3, True), (3000, 8, 3, True)])
@H16
def test_gemm_panel_layernorm_backward_fold(ops, guard, M, r, G, use_attr, h16):
    """FFM_EPI_LNB_STAT / FFM_EPI_LNB_APPLY (ABI 12): ln_2's backward folded into the two dX products of the MLP.
    (1) the dX product of c_proj leaves sum_n dpre pre per row and column tile (packed 16-bit dot products) - float64 on the
    16-bit rows it stored - and nothing else it writes moves; (2) the dX product of c_fc, whose rank operand carries W gamma and
    d = W beta + b as rows 14 / 15 (rank <= 14: its t[14] / t[15] are the two sums against them), fed those partial rows, stores
    rstd (gamma g_h - c1/K - xhat c2/K) + res: held to float64 autograd THROUGH LayerNorm -> FairLoRA linear on the same
    operands (the algebra of include/ffm_hip.h), and to the unfolded pair (plain dX product, then ffm_layernorm_bwd)."""
    rps = 197
    nsamp = (M + rps - 1) // rps
    attr = torch.randint(0, G, (nsamp,), device="cuda", dtype=torch.int32) if use_attr else None
    panel_layernorm_backward_fold_case(ops, guard, M, r, G, attr, rps, h16)


def panel_layernorm_backward_fold_case(ops, guard, M, r, G, attr, rps, dt, before_checks=None, gscale=1.0):
    """Body of test_gemm_panel_layernorm_backward_fold for a given attribute vector and rows per sample.  `before_checks`
    (as in panel_fairlora_case) is called twice: for the LNB_STAT launch (rank operand P2 / S2) and for the LNB_APPLY
    launch (rank operand B_fc / S, whose ts is `us`; that launch stores no t)."""
    width = 768
    N, K = 4 * width, width                                            # c_fc: x [M, 768] -> pre [M, 3072]
    flags1 = 2 | 4 | 32 | 64 | 512 | 2048
    tn = ops.gemm_tiles_n(M, N, K, flags1, r, dt, True)
    nlg = ops.gemm_lgrad_rows(M, N, K, r, dt, True)
    n2 = ops.gemm_tiles_n(M, K, N, 2 | 4 | 64 | 4096, r, dt, True)
    if tn <= 0 or nlg <= 0 or n2 <= 0:
        pytest.skip("no FFM_EPI_LNB_STAT / FFM_EPI_LNB_APPLY kernel pair for this shape or tile mask (the engine then launches "
                    "ffm_layernorm_bwd: the engine's route, Route.ln2_bwd, asks the same two questions)")
    g = lambda *sh, **k: rnd(*sh, **k)
    # the LayerNorm-folded forward product: pre = LN(x) W_eff^T + b
    x = g(M, K, dt=dt, seed=301)
    gamma, beta = 1 + 0.1 * g(K, seed=302), 0.1 * g(K, seed=303)
    Wfc = g(N, K, dt=dt, scale=K ** -0.5, seed=304)                     # frozen c_fc weight [3072, 768]
    bfc = 0.1 * g(N, seed=305)
    A, Bm, S = g(K, r, scale=0.1, seed=306), g(r, N, scale=0.1, seed=307), g(G, r, seed=308)
    pi = mix(attr, G)
    rows = torch.arange(M, device="cuda") // rps
    sb = (pi[rows] if attr is not None else pi.expand(M, G)) @ S.double()                  # [M, r]
    sigma = 0.25
    xd = x.double().requires_grad_(True)
    mu = xd.mean(-1, keepdim=True)
    rstd = (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    xh = (xd - mu) * rstd
    h = xh * gamma.double() + beta.double()
    pre64 = h @ Wfc.double().t() + bfc.double() + sigma * ((h @ A.double()) * sb) @ Bm.double()
    pre = pre64.detach().to(dt)                                        # what the forward stored
    # ---- launch 1: dX of c_proj (its own operands are arbitrary here: what matters is the dpre it stores)
    gi = g(M, K, dt=dt, scale=gscale, seed=310)                        # the gradient operands: gi, and gres of launch 2
    Wpt = g(N, K, dt=dt, scale=K ** -0.5, seed=311)
    P2, S2, lw2 = g(K, r, scale=0.1, seed=312), g(G, r, seed=313), g(N, r, seed=314)
    rk2 = torch.zeros(16, K, device="cuda", dtype=dt)
    ops.PackPlan([(P2, False, rk2)], dt, "cuda").run()
    nrows = ops.gemm_tiles_m(M, N, K, 2 | 4 | 32 | 64, r, dt, True)
    ts1, t_fwd = g(M, r, seed=315), g(M, r, seed=316)
    wg = (Wfc.double() @ gamma.double()).float()
    dvec = (Wfc.double() @ beta.double() + bfc.double()).float()
    bp = ops.pack_b(Wpt)

    def run1(stat):
        out = guard.out(M, N, dtype=dt)
        t, ts = guard.out(M, r), guard.out(M, r)
        dsp = guard.out(nrows, G, r)
        pc, pa = guard.out(nlg, N, r), guard.out(nlg, N, r)
        ro = ops.RankOp(rk2, S2, attr, rps, sigma, 0.7, t_out=t, ts_out=ts, t_fwd=t_fwd, ds_part=dsp, lgrad=(ts1, pc, pa))
        ops.gemm_nt(gi, Wpt, out, lw=lw2, lw_is_kr=True, rankop=ro, b_packed=bp, dgelu_aux=pre, lnb_stat=stat)
        return out, t, ts, dsp, pc, pa

    part = guard.out(tn, M, 2)
    got = run1(ops.LnBwdStat(part))
    base = run1(None)
    for a_, b_ in zip(got, base):
        assert torch.equal(a_, b_), "FFM_EPI_LNB_STAT must not move anything else the launch writes"
    dpre = got[0]
    pi_rows = pi[rows] if attr is not None else pi.expand(M, G)
    if before_checks is not None:
        from types import SimpleNamespace
        ref_t2 = gi.double() @ P2.to(dt).double()
        before_checks(SimpleNamespace(t=got[1], ts=got[2], out=None, act=None, dsp=got[3], ref_t=ref_t2,
                                      ref_ts=sigma * ref_t2 * (pi_rows @ S2.double()), ref_out=None, pi_rows=pi_rows, t_fwd=t_fwd,
                                      attr=attr, rps=rps, scaling=sigma, dt=dt))
    assert not torch.isnan(part).any()
    P = part.double().sum(0)
    assert float(P[:, 0].abs().max()) == 0.0                            # (slot 0: reserved)
    check(P[:, 1], (dpre.double() * pre.double()).sum(-1), 2e-5, "sum dpre pre")
    # ---- launch 2: dX of c_fc with the LayerNorm backward applied
    Wfct = Wfc.t().contiguous()                                        # [768, 3072]: the dX product's B operand
    rk1 = torch.zeros(16, N, device="cuda", dtype=dt)
    # u = dpre B^T: rank operand = B_fc [N, r], with W gamma and d as its rows 14 / 15
    ops.PackPlan([(Bm.t().contiguous(), False, rk1, None, None, (wg, dvec))], dt, "cuda").run()
    assert torch.equal(rk1[14].float(), wg.to(dt).float()) and torch.equal(rk1[15].float(), dvec.to(dt).float())
    gres = g(M, K, dt=dt, scale=gscale, seed=320)
    mean32, rstd32 = mu.detach().float().reshape(-1).contiguous(), rstd.detach().float().reshape(-1).contiguous()
    ag = torch.zeros(2, 16, device="cuda")
    ag[0, :r] = (A.double().t() @ gamma.double()).float()
    ag[1, :r] = (A.double().t() @ beta.double()).float()
    nrows2 = ops.gemm_tiles_m(M, K, N, 2 | 4 | 64, r, dt, True)
    t_fwd1 = g(M, r, seed=321)
    bp2 = ops.pack_b(Wfct)

    def run2(apply):
        out = guard.out(M, K, dtype=dt)
        us = guard.out(M, r)
        dsp = guard.out(nrows2, G, r)
        ro = ops.RankOp(rk1, S, attr, rps, sigma, 0.7, ts_out=us, t_fwd=t_fwd1, ds_part=dsp)
        ops.gemm_nt(dpre, Wfct, out, lw=A, lw_is_kr=True, rankop=ro, b_packed=bp2, lnb_apply=apply)
        return out, us, dsp

    g1, us, dsp = run2(ops.LnBwdApply(part, tn, x, gamma, mean32, rstd32, ag, gres))
    gh, us0, dsp0 = run2(None)
    if before_checks is not None:
        ref_u = dpre.double() @ Bm.t().to(dt).double()                    # u = dpre B_fc^T on the operand as the kernel holds it
        before_checks(SimpleNamespace(t=None, ts=us, out=None, act=None, dsp=dsp, ref_t=ref_u, ref_ts=sigma * ref_u * sb,
                                      ref_out=None, pi_rows=pi_rows, t_fwd=t_fwd1, attr=attr, rps=rps, scaling=sigma, dt=dt))
    if ops.gemm_tile_shape(M, K, N, 2 | 4 | 64 | 4096, r, dt, True)[0] == ops.gemm_tile_shape(M, K, N, 2 | 4 | 64, r, dt, True)[0]:
        assert torch.equal(us, us0) and torch.equal(dsp, dsp0)
    else:
        # FFM_PANEL_MASK with the K split: FFM_EPI_LNB_APPLY exists on the 4-wave 160 x 128 tile only, the plain dX product takes
        # the 8-wave K-split tile - two kernels that add the K slices in different orders, so equal to fp32 rounding
        # (the bounds every t / ts / dS check of this file uses), not to the bit
        check(us, us0.double(), 2e-5, "us against the plain launch on the K-split tile")
        check(dsp.double().sum(0), dsp0.double().sum(0), 5e-5, "dS against the plain launch on the K-split tile")
    assert not torch.isnan(g1.float()).any()
    # float64 autograd through LayerNorm -> FairLoRA linear with the dpre the first launch stored
    (pre64 * dpre.double()).sum().backward()
    ref = xd.grad + gres.double()
    check(g1, ref, tol(dt), "folded LayerNorm backward vs float64 autograd")
    # the unfolded pair: plain dX product (g_h rounded to 16 bits), then ffm_layernorm_bwd with the residual
    g1u = guard.out(M, K, dtype=dt)
    ops.layernorm_bwd(gh, x, gamma, mean32, rstd32, gres, g1u)
    check(g1, g1u.double(), 2 * tol(dt), "against the unfolded pair")
    # ... and the fold is the closer of the two to float64 (g_h is never rounded to 16 bits on its way)
    err = lambda t_: float((t_.double() - ref).abs().max() / ref.abs().max())
    print("LayerNorm backward fold: max error vs float64", err(g1), " unfolded pair", err(g1u))
    guard.check()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,L,heads", [(32, 197, 12), (5, 197, 12), (3, 130, 4), (2, 256, 12)])
def test_attention_backward_layernorm_row_sums_and_plain_apply(ops, guard, dt, B, L, heads):
    attention_lnstat_case(ops, guard, dt, B, L, heads)


def attention_lnstat_case(ops, guard, dt, B, L, heads, gscale=1.0):
    """ln_1's backward folded (ABI 12): ffm_attention_bwd_lnstat leaves, per head, {sum dqkv (W gamma), sum dqkv (qkv - d)} over
    the head's q columns (dQ kernel) and its k and v columns (dK/dV kernel) - float64 on the 16-bit dqkv it stored, which must
    be bit-identical to the plain call's; the dX product of the in-projection with FFM_EPI_LNB_APPLY then stores
    rstd (gamma g_h - c1/K - xhat c2/K) + res: held to float64 autograd through LayerNorm -> in-projection."""
    E, M = heads * 64, B * L
    assert ops.attention_bwd_lnstat_ok(L, False, dt)
    x = rnd(M, E, dt=dt, seed=401)
    gamma, beta = 1 + 0.1 * rnd(E, seed=402), 0.1 * rnd(E, seed=403)
    W = rnd(3 * E, E, dt=dt, scale=E ** -0.5, seed=404)
    bias = 0.1 * rnd(3 * E, seed=405)
    xd = x.double().requires_grad_(True)
    mu = xd.mean(-1, keepdim=True)
    rstd = (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    h = (xd - mu) * rstd * gamma.double() + beta.double()
    qkv64 = h @ W.double().t() + bias.double()
    qkv = qkv64.detach().to(dt).contiguous()
    out = guard.out(M, E, dtype=dt)
    lse = guard.out(B, heads, L)
    ops.attention_fwd(qkv, out, lse, B, L, heads, False)
    dout = rnd(M, E, dt=dt, scale=gscale, seed=406)                    # the gradient operands: dout and the residual gres
    delta = guard.scratch(B, heads, L)
    dq0 = guard.out(M, 3 * E, dtype=dt)
    ops.attention_bwd(qkv, out, dout, lse, delta, dq0, B, L, heads, False)
    wg = (W.double() @ gamma.double()).float().contiguous()
    dvec = (W.double() @ beta.double() + bias.double()).float().contiguous()
    part = guard.out(2 * heads, M, 2)
    dqkv = guard.out(M, 3 * E, dtype=dt)
    ops.attention_bwd(qkv, out, dout, lse, delta, dqkv, B, L, heads, False, ln_stat=(wg, dvec, part))
    assert torch.equal(dqkv, dq0), "the row sums must not move dqkv"
    assert not torch.isnan(part).any()
    g64 = dqkv.double()
    t1, t2 = g64 * wg.double(), g64 * (qkv.double() - dvec.double())
    for hh in range(heads):
        sl = slice(hh * 64, hh * 64 + 64)
        check(part[hh, :, 0], t1[:, sl].sum(-1), 1e-5, f"q columns of head {hh}: sum dqkv (W gamma)")
        check(part[hh, :, 1], t2[:, sl].sum(-1), 1e-5, f"q columns of head {hh}: sum dqkv (qkv - d)")
        kv = lambda t_: t_[:, E + hh * 64:E + hh * 64 + 64].sum(-1) + t_[:, 2 * E + hh * 64:2 * E + hh * 64 + 64].sum(-1)
        check(part[heads + hh, :, 0], kv(t1), 1e-5, f"k, v columns of head {hh}: sum dqkv (W gamma)")
        check(part[heads + hh, :, 1], kv(t2), 1e-5, f"k, v columns of head {hh}: sum dqkv (qkv - d)")
    # the consumer: dX of the in-projection, [M, 3E] x [E, 3E]^T
    if E % 128 or ops.gemm_tiles_n(M, E, 3 * E, 4096, 0, dt, True) <= 0:
        guard.check()
        return                                                          # (no plain panel tile for this shape: the engine asks too)
    Wt = W.t().contiguous()
    gres = rnd(M, E, dt=dt, scale=gscale, seed=407)
    mean32, rstd32 = mu.detach().float().reshape(-1).contiguous(), rstd.detach().float().reshape(-1).contiguous()
    g1 = guard.out(M, E, dtype=dt)
    ops.gemm_nt(dqkv, Wt, g1, b_packed=ops.pack_b(Wt),
                lnb_apply=ops.LnBwdApply(part, 2 * heads, x, gamma, mean32, rstd32, None, gres))
    (qkv64 * dqkv.double()).sum().backward()
    ref = xd.grad + gres.double()
    check(g1, ref, tol(dt), "folded ln_1 backward vs float64 autograd")
    gh = guard.out(M, E, dtype=dt)
    ops.gemm_nt(dqkv, Wt, gh, b_packed=ops.pack_b(Wt))
    g1u = guard.out(M, E, dtype=dt)
    ops.layernorm_bwd(gh, x, gamma, mean32, rstd32, gres, g1u)
    check(g1, g1u.double(), 2 * tol(dt), "against the unfolded pair")
    guard.check()


def test_skinny_x3_tiles_per_block_switch():
    """FFM_SKINNY_NT (read once per process): the text tower's X3 product with 1 / 2 / 4 column tiles per block
    (csrc/gemm_skinny.hip, gemm_skinny_nt_kernel: the tiles of a block share the activation fragments).  The partial sums
    meet in the one-tile kernel's order, so the three settings are BIT-identical on the text tower's shapes; the float64
    test runs again under each setting in a child process."""
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import torch, sys; sys.path.insert(0, %r); from fairfedmed_amd import ops\n"
            "g = torch.Generator(device='cuda').manual_seed(11)\n"
            "res = {}\n"
            "for (M, N, K) in ((40, 1536, 512), (40, 512, 512), (40, 2048, 512), (40, 512, 2048), (33, 48, 640), (40, 96, 512)):\n"
            "    a = torch.randn(M, K, device='cuda', generator=g); w = torch.randn(N, K, device='cuda', generator=g) * K ** -0.5\n"
            "    bias = torch.randn(N, device='cuda', generator=g); r = torch.randn(M, N, device='cuda', generator=g)\n"
            "    out = torch.full((M, N), float('nan'), device='cuda'); act = torch.full((M, N), float('nan'), device='cuda')\n"
            "    ops.gemm_nt(a, w, out, bias=bias, res=r, x3=True); res[(M, N, K, 'res')] = out.cpu().clone()\n"
            "    ops.gemm_nt(a, w, out, bias=bias, gelu_out=act, x3=True); res[(M, N, K, 'gelu')] = (out.cpu().clone(), act.cpu().clone())\n"
            "    ops.gemm_nt(a, w, out, dgelu_aux=r, x3=True); res[(M, N, K, 'dgelu')] = out.cpu().clone()\n"
            "torch.cuda.synchronize(); torch.save(res, sys.argv[1])\n" % root)
    with tempfile.TemporaryDirectory() as d:
        got = {}
        for nt in ("1", "2", "4"):
            f = os.path.join(d, nt + ".pt")
            env = dict(os.environ, FFM_SKINNY_NT=nt)
            r = subprocess.run([sys.executable, "-c", code, f], env=env, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            got[nt] = torch.load(f)
            r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", os.path.join(root, "tests", "test_kernels_gpu.py"), "-k",
                                "test_skinny_gemm_f32 and x3"], env=env, cwd=root, capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for key, ref in got["1"].items():
        for nt in ("2", "4"):
            other = got[nt][key]
            if isinstance(ref, tuple):
                assert all(torch.equal(x, y) for x, y in zip(ref, other)), (key, nt)
            else:
                assert not torch.isnan(other).any() and torch.equal(ref, other), (key, nt)


def test_x3_gemm_rejects_large_products():
    """FFM_F32_X3 exists for skinny products only: anything else is refused, never computed some other way."""
    from fairfedmed_amd import ops
    a = torch.randn(256, 512, device="cuda")
    w = torch.randn(512, 512, device="cuda")
    with pytest.raises(RuntimeError):
        ops.gemm_nt(a, w, torch.empty(256, 512, device="cuda"), x3=True)


# ------------------------------------------------ LayerNorm folded into the GEMMs around it ---
@pytest.mark.mask_tolerant
@H16
def test_gemm_rowstats_partials(guard, h16):
    rowstats_case(guard, h16, 6304)


def rowstats_case(guard, h16, M):
    """FFM_EPI_ROWSTATS (out-proj forward shape): the partial {sum, sum of squares} of every STORED output row, one
    partial per column tile, add up to the row sums of the bf16 output."""
    from fairfedmed_amd import ops, _lib as L
    N, K = 768, 768
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn(M, K, device="cuda", generator=g).to(h16)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(h16)
    bias = torch.randn(N, device="cuda", generator=g)
    res = (3 + torch.randn(M, N, device="cuda", generator=g)).to(h16)
    out = guard.out(M, N, dtype=h16)
    bp = ops.pack_b(w)
    tn = ops.gemm_tiles_n(M, N, K, L.EPI_BIAS | L.EPI_RESIDUAL | L.EPI_ROWSTATS, 0, h16, True)
    assert tn > 0
    part = guard.out(tn, M, 2)
    ops.gemm_nt(a, w, out, bias=bias, res=res, b_packed=bp, rowstats=part)
    ref = a.float() @ w.float().t() + bias + res.float()
    assert float((out.float() - ref).abs().max() / ref.abs().max()) < 1e-2
    o = out.double()
    got = part.double().sum(0)
    assert not torch.isnan(part).any()
    assert float((got[:, 0] - o.sum(1)).abs().max() / o.sum(1).abs().max()) < 1e-5
    assert float((got[:, 1] - (o * o).sum(1)).abs().max() / (o * o).sum(1).abs().max()) < 1e-5
    # without the packed weight no kernel serves the flag: refused, not computed some other way
    with pytest.raises(RuntimeError):
        ops.gemm_nt(a, w, out, bias=bias, res=res, rowstats=part)
    guard.check()


@pytest.mark.mask_tolerant
@pytest.mark.parametrize("np_", [1, 6])
@H16
def test_gemm_layernorm_folded_in(guard, np_, h16):
    layernorm_folded_in_case(guard, np_, h16, 6304)


def layernorm_folded_in_case(guard, np_, h16, M):
    """FFM_EPI_LNIN (qkv forward shape): raw rows x gamma-scaled weight, corrected in the epilogue with the row statistics
    assembled from np partial sums, equals LayerNorm(x) W^T + b; mean / rstd come out for the LayerNorm backward."""
    from fairfedmed_amd import ops
    N, K = 2304, 768
    g = torch.Generator(device="cuda").manual_seed(6)
    x = (1.5 + 2.0 * torch.randn(M, K, device="cuda", generator=g)).to(h16)     # a row mean far from 0
    x[:, 5] += 40.0                                                                          # one outlier channel
    w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
    gamma = 1 + 0.2 * torch.randn(K, device="cuda", generator=g)
    beta = 0.3 * torch.randn(K, device="cuda", generator=g)
    bias = torch.randn(N, device="cuda", generator=g)
    wg = (w * gamma).to(h16)
    c = wg.float().sum(1).contiguous()
    d = (w @ beta + bias).contiguous()
    xf = x.float()
    cols = torch.tensor_split(torch.arange(K, device="cuda"), np_)
    part = torch.stack([torch.stack([xf[:, ix].sum(1), (xf[:, ix] ** 2).sum(1)], 1) for ix in cols]).contiguous()
    out = guard.out(M, N, dtype=h16)
    mean = guard.out(M)
    rstd = guard.out(M)
    ops.gemm_nt(x, wg, out, bias=d, b_packed=ops.pack_b(wg), ln_in=ops.LnIn(part, np_, c, mean, rstd))
    xd = x.double()
    mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    ref = ((xd - mu) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()) @ w.double().t() + bias.double()
    assert float((out.double() - ref).abs().max() / ref.abs().max()) < 1.5e-2           # bf16 weights and output
    assert float((mean.double() - mu[:, 0]).abs().max()) < 1e-4
    assert float((rstd.double() * torch.sqrt(var[:, 0] + 1e-5) - 1).abs().max()) < 1e-4
    # against the unfolded bf16 path (LayerNorm kernel, then the product): the folded form is no less accurate
    h = guard.like(x)
    ops.layernorm_fwd(x, h, gamma, beta, guard.out(M), guard.out(M))
    wb = w.to(h16)
    out2 = guard.like(out)
    ops.gemm_nt(h, wb, out2, bias=bias, b_packed=ops.pack_b(wb))
    e_fold = float((out.double() - ref).abs().mean())
    e_plain = float((out2.double() - ref).abs().mean())
    print(f"mean abs error: folded {e_fold:.3e}, LayerNorm kernel + GEMM {e_plain:.3e}")
    assert e_fold < 1.5 * e_plain
    guard.check()


@H16
def test_lora_grad_partial_through_a_folded_layernorm(guard, h16):
    lora_grad_partial_ln_case(guard, h16, 6304)


def lora_grad_partial_ln_case(guard, h16, M, gscale=1.0):
    """ffm_lora_grad_partial_ln: dA = LayerNorm(x)^T v from the RAW rows (the normalised copy is never written when ln_2
    rides inside the c_fc product) equals the plain reduction on a materialised LayerNorm output."""
    from fairfedmed_amd import ops
    K, r = 768, 8
    g = torch.Generator(device="cuda").manual_seed(9)
    x = (0.7 + 1.5 * torch.randn(M, K, device="cuda", generator=g)).to(h16)
    v = torch.randn(M, r, device="cuda", generator=g) * gscale           # the gradient operand (us)
    gamma = 1 + 0.2 * torch.randn(K, device="cuda", generator=g)
    beta = 0.3 * torch.randn(K, device="cuda", generator=g)
    xd = x.double()
    mu, var = xd.mean(1), xd.var(1, unbiased=False)
    rstd = 1 / torch.sqrt(var + 1e-5)
    ns = ops.lora_grad_splits(M)
    part = guard.out(ns, K, r)
    ops.lora_grad_partial_ln(x, v, mu.float(), rstd.float(), gamma, beta, r, part)
    got = part.double().sum(0)
    y = (xd - mu[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    ref = y.t() @ v.double()
    assert not torch.isnan(part).any()
    check(got, ref, 2e-4, "dA through the folded LayerNorm")           # v enters as a 16-bit hi + lo pair
    guard.check()


def test_reduce_partials_many_rows_of_a_short_tensor():
    """ffm_reduce_partials on the 3D OCT shape (19 600 partial rows of 603 outputs: the tall kernel) and on a short
    stack of a long tensor (the 4-lane kernel): both equal the float64 column sums, also transposing and accumulating."""
    from fairfedmed_amd import ops
    g = torch.Generator(device="cuda").manual_seed(3)
    for ns, n, tk, tr in ((19600, 603, 0, 0), (700, 96, 12, 8), (50, 24576, 3072, 8)):
        part = torch.randn(ns, n, device="cuda", generator=g)
        out = torch.full((n,), 2.0, device="cuda")
        ops.reduce_partials(part, ns, n, out, transpose_K=tk, transpose_r=tr, accumulate=True)
        ref = part.double().sum(0)
        if tk:
            ref = ref.view(tk, tr).t().reshape(-1)
        ref = ref + 2.0
        assert float((out.double() - ref).abs().max()) < 2e-3 * (ns ** 0.5) / 10, (ns, n)


# ------------------------------------------------------ text tower's two ends ---
@pytest.mark.parametrize("use_ot", [False, True], ids=["mean-over-prompts", "per-prompt"])
@pytest.mark.parametrize("N,n_cls,n_ctx,TL,w,D", [(2, 2, 4, 10, 512, 512), (3, 2, 2, 7, 128, 192)])
def test_text_tower_ends_vs_autograd(ops, guard, use_ot, N, n_cls, n_ctx, TL, w, D):
    text_tower_ends_case(ops, guard, use_ot, N, n_cls, n_ctx, TL, w, D)


def text_tower_ends_case(ops, guard, use_ot, N, n_cls, n_ctx, TL, w, D, gscale=1.0):
    """csrc/text.hip against the PyTorch statement of the same ops (trainers/GLP_OT_SVLoRA.py:131-152, 55-66, 713-717):
    prompt assembly + positional embedding; EOT gather -> ln_final -> projection -> normalise (-> mean over prompts);
    their backward down to the tower's output rows; d ctx summed over the classes."""
    n_text = N * n_cls
    prefix, suffix = rnd(n_text, 1, w, seed=1), rnd(n_text, 20, w, seed=2)
    ctx, pos = rnd(N, n_ctx, w, seed=3), rnd(TL + 5, w, seed=4)
    x0 = guard.out(n_text * TL, w)
    ops.text_embed(prefix, ctx, suffix, pos, x0, n_cls, TL)
    ctx_rows = ctx.unsqueeze(1).expand(N, n_cls, n_ctx, w).reshape(n_text, n_ctx, w)
    ref0 = torch.cat([prefix, ctx_rows, suffix[:, :TL - 1 - n_ctx]], dim=1) + pos[:TL]
    assert torch.equal(x0, ref0.reshape(n_text * TL, w))
    # tail forward
    x = rnd(n_text * TL, w, seed=5) * 1.5 + 0.3
    eot_pos = [TL - 1 - (i % n_cls) for i in range(n_text)]
    eot_row = torch.tensor([i * TL + e for i, e in enumerate(eot_pos)], device="cuda", dtype=torch.int32)
    lnw, lnb, proj = 1 + 0.1 * rnd(w, seed=6), 0.1 * rnd(w, seed=7), rnd(w, D, seed=8) * w ** -0.5
    tf, tn = guard.out(n_text, D), guard.out(n_text, D)
    rn, st = guard.out(n_text), guard.out(n_text, 2)
    tbar = None if use_ot else guard.out(n_cls, D)
    ops.text_tail_fwd(x, eot_row, lnw, lnb, proj, tf, tn, rn, st, tbar, N, n_cls)
    xd = x.double().requires_grad_(True)
    xe = xd[eot_row.long()]
    y = torch.nn.functional.layer_norm(xe, (w,), lnw.double(), lnb.double(), 1e-5)
    tfr = y @ proj.double()
    tnr = torch.nn.functional.normalize(tfr.view(N, n_cls, D), dim=2)
    out_ref = tnr.reshape(n_text, D) if use_ot else tnr.mean(0)
    check(tf, tfr, 2e-6, "tf")
    check(tn, tnr.reshape(n_text, D), 2e-6, "tn")
    if not use_ot:
        check(tbar, out_ref, 2e-6, "tbar")
    # tail backward
    dout = rnd(*out_ref.shape, scale=gscale, seed=9)                      # the gradient operands: dout and gin
    out_ref.backward(dout.double())
    g = guard.out(n_text * TL, w)
    dy = guard.out(n_text, w)
    ops.text_tail_bwd(x, eot_row, lnw, proj, tn, rn, st, None if use_ot else dout, dout if use_ot else None, dy, g, N, n_cls, TL)
    check(g, xd.grad, 5e-6, "d(tower output)")
    rows = torch.ones(n_text * TL, dtype=torch.bool, device="cuda")
    rows[eot_row.long()] = False
    assert float(g[rows].abs().max()) == 0.0                               # every non-EOT row is exactly zero
    # d ctx = input-gradient rows 1 .. n_ctx of every prompt, summed over the classes
    gin = rnd(n_text * TL, w, scale=gscale, seed=10)
    dctx = guard.out(N, n_ctx, w)
    ops.text_ctx_grad(gin, dctx, n_cls, TL)
    refc = gin.double().view(N, n_cls, TL, w)[:, :, 1:1 + n_ctx, :].sum(1)
    check(dctx, refc, 1e-6, "dctx")
    guard.check()


@pytest.mark.parametrize("mask,what", [(0, "the round-2 tiles only (configurations 0-4)"),
                                       ((1 << 7) | (1 << 8) | (1 << 10) | (1 << 11) | (1 << 12), "default set + the K split")])
def test_panel_tile_configurations_behind_the_mask(mask, what):
    """FFM_PANEL_MASK (read once per process) selects among the panel-kernel configurations (csrc/gemm_panel.hip): the
    default set is what every other test runs on; here the panel, row-sum and LayerNorm-folding tests run again in a child
    process on the round-2 tiles alone and with the 8-wave K split of the 160 x 128 tiles switched on, so that every
    instantiated kernel stays held to float64."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FFM_PANEL_MASK=str(mask))
    # no -x in the child: the tail then names every failure, not just the first
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-rfE", os.path.join(root, "tests", "test_kernels_gpu.py"),
                        os.path.join(root, "tests", "test_group_mix_gpu.py"), os.path.join(root, "tests", "test_guard_bands_gpu.py"), "-m",
                        "mask_tolerant"], env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "deselected" in r.stdout


def test_attention_quarter_head_blocks_switch():
    """FFM_ATTN_PARTS=4 (read once per process): the attn2_* kernels as quarter heads of 4 waves instead of half heads of
    7 (csrc/attention.hip; measured slower, kept as a switch) - the attention tests again in a child process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", os.path.join(root, "tests", "test_kernels_gpu.py"), "-k",
                        "test_attention_fwd_bwd"], env=dict(os.environ, FFM_ATTN_PARTS="4"), cwd=root, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


# --------------------------------------- attention, third generation (csrc/attention3.hip) ---
# Every 32-token tile count the fat-wave kernels take (3..8 tiles: 65..256 tokens), tile edges (L = 32 k, 32 k + 1,
# 32 k - 1), the vision tower's lengths (197; 113..224 in steps), one and several (batch, head) pairs per XCD group, in
# both 16-bit storage types, against float64.
A3_LENGTHS = [65, 96, 97, 113, 128, 129, 144, 160, 161, 176, 192, 193, 197, 200, 208, 209, 224, 225, 240, 255, 256]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("L", A3_LENGTHS)
def test_attention3_lengths(ops, guard, dt, L):
    B, heads = (3, 5) if L % 2 else (2, 12)
    E = heads * 64
    qkv = rnd(B * L, 3 * E, dt=dt, seed=230 + L)
    out = guard.out(B * L, E, dtype=dt)
    lse = guard.out(B, heads, L)
    ops.attention_fwd(qkv, out, lse, B, L, heads, False)
    qd = qkv.double().requires_grad_(True)
    ref, ref_lse = ref_attention(qd, B, L, heads, False)
    t16 = 1.2e-2 if dt == torch.bfloat16 else 2e-3
    check(out, ref.detach(), t16, "attn out")
    check(lse, ref_lse.detach(), 2e-3 if dt == torch.bfloat16 else 3e-4, "lse")
    dout = rnd(B * L, E, dt=dt, seed=240 + L)
    ref.backward(dout.double())
    dqkv = guard.out(B * L, 3 * E, dtype=dt)
    delta = guard.out(B, heads, L)
    ops.attention_bwd(qkv, out, dout, lse, delta, dqkv, B, L, heads, False)
    check(delta, (dout.double() * out.double()).reshape(B, L, heads, 64).sum(-1).permute(0, 2, 1), 1e-5, "delta")
    check(dqkv[:, :E], qd.grad[:, :E], 2 * t16, "dq")
    check(dqkv[:, E:2 * E], qd.grad[:, E:2 * E], 2 * t16, "dk")
    check(dqkv[:, 2 * E:], qd.grad[:, 2 * E:], 2 * t16, "dv")
    guard.check()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_attention3_propagates_non_finite_inputs(ops, guard, dt, bad):
    """attention3.hip is compiled with -fno-honor-nans (the row maxima), and the step's only divergence guard is the finite
    flag ce_loss raises from the logits: a NaN / Inf in q, k or v must therefore come out of the attention output (and a
    NaN / Inf in dO out of dq, dk, dv) and not be folded away by a max / select the compiler assumed NaN-free."""
    B, heads, L = 2, 3, 197
    E = heads * 64
    b, h = 1, 2                                                   # the (batch, head) pair that is poisoned
    rows = slice(b * L, (b + 1) * L)
    for which, row in (("q", 5), ("k", 100), ("v", 196)):
        qkv = rnd(B * L, 3 * E, dt=dt, seed=250)
        col = {"q": 0, "k": E, "v": 2 * E}[which] + h * 64 + 7
        qkv[b * L + row, col] = bad
        out = guard.out(B * L, E, dtype=dt)
        lse = guard.out(B, heads, L)
        ops.attention_fwd(qkv, out, lse, B, L, heads, False)
        guard.check()
        o = out[rows, h * 64:(h + 1) * 64].float()
        hit = ~torch.isfinite(o).all(dim=1)
        if which == "q":
            assert bool(hit[row]), (which, "the poisoned query's output row is finite")
        elif which == "k" and bad == float("inf"):
            # q . k = +inf where the query's element is positive (inf - inf in the softmax), -inf elsewhere: that key then
            # simply carries no weight, and the row is finite in exact arithmetic too
            pos = qkv[rows, h * 64 + 7].float() > 0
            assert bool(hit[pos].all()) and int(pos.sum()) > 0, (which, int(hit.sum()), int(pos.sum()))
        else:
            assert bool(hit.all()), (which, int(hit.sum()), "every query of the pair sees the poisoned key / value")
        # everything outside the pair stays finite
        out[rows, h * 64:(h + 1) * 64] = 0
        assert bool(torch.isfinite(out.float()).all())
    qkv = rnd(B * L, 3 * E, dt=dt, seed=251)
    out = guard.out(B * L, E, dtype=dt)
    lse = guard.out(B, heads, L)
    ops.attention_fwd(qkv, out, lse, B, L, heads, False)
    dout = rnd(B * L, E, dt=dt, seed=252)
    dout[b * L + 11, h * 64 + 3] = bad
    dqkv = guard.out(B * L, 3 * E, dtype=dt)
    delta = guard.scratch(B, heads, L)
    ops.attention_bwd(qkv, out, dout, lse, delta, dqkv, B, L, heads, False)
    dq = dqkv[rows, h * 64:(h + 1) * 64].float()
    dk = dqkv[rows, E + h * 64:E + (h + 1) * 64].float()
    dv = dqkv[rows, 2 * E + h * 64:2 * E + (h + 1) * 64].float()
    assert not bool(torch.isfinite(dq[11]).all()), "dq of the poisoned row"
    assert not bool(torch.isfinite(dk).all()) and not bool(torch.isfinite(dv).all()), "dk / dv of the pair"
    guard.check()


@pytest.mark.parametrize("L", [197, 130])
def test_attention3_running_maximum_and_rows(ops, guard, L):
    """The second DMA half can raise a row's maximum (the rescale path): one key of the second half is made to dominate
    chosen queries, another row peaks in the first half; per-row comparison so that one wrong row cannot hide."""
    dt, B, heads = torch.bfloat16, 2, 3
    E = heads * 64
    qkv = rnd(B * L, 3 * E, dt=dt, seed=77, scale=0.5)
    v = qkv.view(B, L, 3, heads, 64)
    v[0, 5, 0, 1] = 2.0                                    # query 5 of head 1 ...
    v[0, L - 2, 1, 1] = 3.0                                # ... against a key of the last tile: score 384 / 8
    v[1, 40, 0, 2] = -2.0
    v[1, 3, 1, 2] = -3.0                                   # query 40 of head 2 peaks at key 3 (first half)
    out = guard.out(B * L, E, dtype=dt)
    lse = guard.out(B, heads, L)
    ops.attention_fwd(qkv, out, lse, B, L, heads, False)
    ref, ref_lse = ref_attention(qkv.double(), B, L, heads, False)
    err = (out.double() - ref).abs().reshape(B, L, heads, 64).amax(-1)
    assert float(err.max()) <= 1.2e-2 * float(ref.abs().max()), (float(err.max()), err.argmax())
    assert float((lse.double() - ref_lse).abs().max()) <= 2e-3 * float(ref_lse.abs().max())
    assert float(lse[0, 1, 5]) > 40.0                      # the spike really is the row maximum
    guard.check()


def test_attention3_is_the_kernel_that_runs_and_matches_the_second_generation():
    """attn3_* must be what the vision tower's shape launches (no silent fallback), and it agrees with attn2_* run in a
    child process under FFM_ATTN=v2 to 16-bit rounding."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import torch, sys; sys.path.insert(0, %r); from fairfedmed_amd import ops\n"
            "g = torch.Generator(device='cuda').manual_seed(5)\n"
            "qkv = torch.randn(2 * 197, 2304, device='cuda', generator=g).bfloat16()\n"
            "out = torch.empty(2 * 197, 768, device='cuda', dtype=torch.bfloat16); lse = torch.empty(2, 12, 197, device='cuda')\n"
            "ops.attention_fwd(qkv, out, lse, 2, 197, 12, False); torch.cuda.synchronize()\n"
            "torch.save({'out': out.cpu(), 'lse': lse.cpu()}, sys.argv[1])\n" % root)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        res = {}
        for gen in ("v2", "v3"):
            f = os.path.join(d, gen + ".pt")
            r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, FFM_ATTN=gen), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            res[gen] = torch.load(f)
    a, b = res["v2"], res["v3"]
    assert not torch.equal(a["out"], b["out"]), "FFM_ATTN=v2 / v3 ran the same kernel"
    assert float((a["out"].double() - b["out"].double()).abs().max()) <= 2e-2 * float(a["out"].double().abs().max())
    assert float((a["lse"] - b["lse"]).abs().max()) <= 2e-3 * float(a["lse"].abs().max())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_attention3_race_screen_bitwise_repeatable(ops, guard, dt):
    """attn3_* order their LDS-DMA by hand-counted s_waitcnt vmcnt(N) + raw s_barrier (no compiler-inserted waits): a read
    placed one phase early passes a reference check whenever the DMA happens to land first.  Screen: the bench shape (768
    blocks, three per CU) 30 times back to back, with a cache-flushing write between launches on every third run (the DMA then
    comes from HBM instead of the Infinity Cache: different landing order), every output bit-identical to the first run's -
    the kernels have no atomics and no run-dependent summation order."""
    B, L, heads = 32, 197, 12
    E = heads * 64
    qkv = rnd(B * L, 3 * E, dt=dt, seed=901)
    dout = rnd(B * L, E, dt=dt, seed=902)
    flush = torch.empty(320 << 20, device="cuda", dtype=torch.uint8)
    first = None
    for it in range(30):
        out = guard.out(B * L, E, dtype=dt)
        lse = guard.out(B, heads, L)
        dqkv = guard.out(B * L, 3 * E, dtype=dt)
        delta = guard.out(B, heads, L)
        if it % 3 == 1:
            flush.fill_(it)
        ops.attention_fwd(qkv, out, lse, B, L, heads, False)
        if it % 3 == 2:
            flush.fill_(it)
        ops.attention_bwd(qkv, out, dout, lse, delta, dqkv, B, L, heads, False)
        cur = (out, lse, dqkv, delta)
        if first is None:
            first = cur
            assert all(bool(torch.isfinite(t.float()).all()) for t in cur)
        else:
            for a, b, nm in zip(cur, first, ("out", "lse", "dqkv", "delta")):
                assert torch.equal(a, b), f"run {it}: {nm} differs from run 0 in {int((a != b).sum())} elements"
    guard.check()


# ------------------------------- QuickGELU with the derivative as the saved tensor (ffm_gemm_args.gelu_deriv) ---
def _qgelu64(x):
    return x * torch.sigmoid(1.702 * x)


def _qgelu_grad64(x):
    s = torch.sigmoid(1.702 * x)
    return s * (1 + 1.702 * x * (1 - s))


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,N,K,packed", [(333, 384, 256, False),        # 128 x 128 kernel
                                          (40, 512, 512, False),         # skinny kernel (text tower rows)
                                          (6304, 3072, 768, True)])      # panel kernel (16-bit: fragment-packed weights)
def test_gemm_gelu_derivative_form(ops, guard, dt, M, N, K, packed):
    """FFM_EPI_GELU with gelu_deriv: `out` = quick_gelu'(x), `gelu_out` = quick_gelu(x), x the product as it would have been
    stored; FFM_EPI_DGELU with gelu_deriv: out = (a b^T) * aux.  Chained, the two launches give the classic pair's result:
    g W^T * quick_gelu'(pre) - bit-identical in fp32, to one 16-bit rounding of the derivative otherwise."""
    if packed and dt == torch.float32:
        pytest.skip("packed weights are a 16-bit layout")
    a, w = rnd(M, K, dt=dt, seed=71), rnd(N, K, dt=dt, scale=K ** -0.5, seed=72)
    bias = rnd(N, seed=73)
    bp = ops.pack_b(w) if packed else None
    d = guard.out(M, N, dtype=dt)
    act = guard.out(M, N, dtype=dt)
    pre = guard.out(M, N, dtype=dt)
    act0 = guard.out(M, N, dtype=dt)
    kw = dict(bias=bias, b_packed=bp)
    if packed:                                   # the panel kernel's GELU epilogues are the FairLoRA ones: rank operand needed
        P = rnd(K, 8, scale=0.1, seed=74)
        rk = torch.zeros(16, K, device="cuda", dtype=dt)
        ops.PackPlan([(P, False, rk)], dt, "cuda").run()
        attr = torch.randint(0, 3, ((M + 196) // 197,), device="cuda", dtype=torch.int32)
        mk = lambda: ops.RankOp(rk, rnd(3, 8, seed=75), attr, 197, 0.25, 0.7, t_out=guard.out(M, 8),
                                ts_out=guard.out(M, 8))
        kw.update(lw=rnd(8, N, scale=0.1, seed=76))
        ops.gemm_nt(a, w, pre, gelu_out=act0, rankop=mk(), **kw)
        ops.gemm_nt(a, w, d, gelu_out=act, rankop=mk(), gelu_deriv=True, **kw)
        assert ops.gemm_tiles_m(M, N, K, 1 | 2 | 16 | 64, 8, dt, True) != ops.gemm_tiles_m(M, N, K, 1 | 2 | 16 | 64, 8, dt, False)
    else:
        ops.gemm_nt(a, w, pre, gelu_out=act0, **kw)
        ops.gemm_nt(a, w, d, gelu_out=act, gelu_deriv=True, **kw)
    assert torch.equal(act, act0), "the activation must not depend on which tensor is saved"
    x = pre.double()                             # the stored (rounded) pre-activation of the classic launch
    check(d, _qgelu_grad64(x), 1e-6 if dt == torch.float32 else tol(dt), "saved derivative")
    check(act, _qgelu64(x), 1e-6 if dt == torch.float32 else tol(dt), "activation")
    # backward: g W * saved tensor, both forms
    g, wt = rnd(M, 64, dt=dt, seed=77), rnd(N, 64, dt=dt, scale=0.125, seed=78)
    o0 = guard.out(M, N, dtype=dt)
    o1 = guard.out(M, N, dtype=dt)
    ops.gemm_nt(g, wt, o0, dgelu_aux=pre)
    ops.gemm_nt(g, wt, o1, dgelu_aux=d, gelu_deriv=True)
    if dt == torch.float32:
        assert torch.equal(o0, o1), "fp32: the derivative form is the same arithmetic"
    check(o1, (g.double() @ wt.double().t()) * _qgelu_grad64(x), tol(dt) * 2, "dX with the saved derivative")
    check(o1, o0.double(), tol(dt) * 2, "derivative form vs classic form")
    guard.check()
