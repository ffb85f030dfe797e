"""Client-level differential privacy at the round boundary, on the GPU: the generator, the noise, the norm and the
privatise pass of csrc/dp.hip against the float64 reference of tests/dp_ref.py, and FedAvgAggregator(dp=...) on device
tensors against that reference and against the same object on CPU tensors."""
import functools
import math

import numpy as np
import pytest
import torch

from fairfedmed_amd import _lib
from fairfedmed_amd import config as C
from fairfedmed_amd import dp as D
from fairfedmed_amd.fedavg import FedAvgAggregator, element_weights, is_group_s_block
from tests import dp_ref as R
from tests.test_fedavg_gloo import _layout

gpu = pytest.mark.gpu
SIZES = [1, 3, 4, 5, 1022, 2049, 70001]          # below one group, around a group, tails of 2 / 1 / 1, more than one block
FULL = 741952                                    # the ViT-B/16 rank-8 trainable buffer
SENT = 12345.0                                   # guard value around every output: nothing may be written outside [0, n)
SEED = 0x1234567890abcdef
TINY = float(np.finfo(np.float32).tiny)


def _place(x, shift):
    """x (numpy fp32 or None: guards only) on the device at `shift` elements behind a 16-byte boundary; (buffer, view)."""
    n = len(x)
    buf = torch.full((n + 8,), SENT, dtype=torch.float32, device="cuda")
    view = buf[shift:shift + n]
    assert view.data_ptr() % 16 == (4 * shift) % 16
    view.copy_(torch.from_numpy(np.array(x, dtype=np.float32)))         # (a writable copy: the shared inputs are read-only)
    return buf, view


def _guards_intact(buf, shift, n):
    return bool((buf[:shift] == SENT).all()) and bool((buf[shift + n:] == SENT).all())


@functools.lru_cache(maxsize=None)
def _data(n):
    rng = np.random.default_rng(1000 + n)
    g = (0.1 * rng.standard_normal(n)).astype(np.float32)
    theta = (g + 0.01 * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    w = rng.uniform(0.1, 0.9, n).astype(np.float32)
    start = rng.standard_normal(n).astype(np.float32)
    for a in (g, theta, w, start):
        a.setflags(write=False)
    return theta, g, w, start, R.norm(theta, g)


@functools.lru_cache(maxsize=None)
def _xi(n, t, k):
    z = R.gaussians(n, SEED, t, k)
    z.setflags(write=False)
    return z


def _privatise(n, shift, clip, sigma=0.0, t=0, k=0, accumulate=False, theta=None, g=None):
    from fairfedmed_amd import ops
    th0, g0, w0, start, _ = _data(n)
    theta = th0 if theta is None else theta
    g = g0 if g is None else g
    (_, th), (_, gg), (_, ww) = _place(theta, shift), _place(g, shift), _place(w0, shift)
    obuf, out = _place(start, shift)
    scratch = ops.dp_scratch(n, "cuda")
    stats = torch.full((2,), SENT, device="cuda")
    ops.dp_norm(th, gg, scratch)
    ops.dp_privatise(th, gg, ww, out, scratch, clip, sigma, SEED, t, k, accumulate=accumulate, stats=stats)
    torch.cuda.synchronize()
    assert _guards_intact(obuf, shift, n)
    return out, stats.cpu(), scratch, (th, gg, ww)


@gpu
def test_raw_philox_words():
    from fairfedmed_amd import ops
    for counter, key, want in R.KAT:
        out = torch.zeros(4, dtype=torch.int32, device="cuda")
        ops.dp_philox(out, key[0] | (key[1] << 32), *counter)
        assert tuple(int(v) for v in out.cpu().numpy().view(np.uint32)) == want
    for n in (4096, 4093):
        out = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
        ops.dp_philox(out[:n], SEED, 0, 7, 2, 0)
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:n], R.words(n, SEED, 0, 7, 2, 0)) and not got[n:].any()
    # the counter's first word is taken modulo 2^32
    out = torch.zeros(8, dtype=torch.int32, device="cuda")
    ops.dp_philox(out, SEED, 0xffffffff, 1, 2, 3)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), R.words(8, SEED, 0xffffffff, 1, 2, 3))


@gpu
@pytest.mark.parametrize("t,k", [(0, 0), (41, 3)])
@pytest.mark.parametrize("n", SIZES)
def test_noise_alone_against_the_float64_reference(n, t, k):
    from fairfedmed_amd import ops
    sigma = 0.75
    got = []
    for shift in (0, 1):
        buf, out = _place(np.zeros(n, np.float32), shift)
        ops.dp_noise(out, sigma, SEED, t, k)
        torch.cuda.synchronize()
        assert _guards_intact(buf, shift, n)
        got.append(out.cpu())
    ref = float(np.float32(sigma)) * _xi(n, t, k)
    dev = float(np.abs(got[0].numpy().astype(np.float64) - ref).max())
    print(f"sigma*xi n={n} (t,k)=({t},{k}): max |gpu - fp64| = {dev / sigma:.3e} sigma")
    assert dev <= 1e-5 * sigma
    assert torch.equal(got[0], got[1])               # the index counts from the pointer passed, aligned or not


@gpu
@pytest.mark.parametrize("n", SIZES + [FULL])
def test_norm_against_the_float64_reference(n):
    _, _, _, _, ref = _data(n)
    seen = []
    for shift in (0, 1):
        for _ in range(2):
            _, stats, scratch, _ = _privatise(n, shift, clip=1e6)
            seen.append((float(stats[0]), scratch.cpu()))
            assert float(stats[1]) == 1.0
    print(f"norm n={n}: gpu {seen[0][0]:.9g} ref {ref:.9g} rel {abs(seen[0][0] - ref) / ref:.2e}")
    assert abs(seen[0][0] - ref) <= 5e-7 * ref
    for nu, part in seen[1:]:                        # two calls, and the two access paths: the same bits
        assert nu == seen[0][0] and torch.equal(part, seen[0][1])
    assert seen[0][1].numel() * 8 == _lib.load().ffm_dp_norm_ws_bytes(n)


@gpu
def test_norm_whose_sum_of_squares_leaves_the_fp32_range():
    n = 1000
    pattern = np.cos(0.37 * np.arange(n)).astype(np.float32)
    theta = (np.float32(3e19) * pattern).astype(np.float32)
    g = np.zeros(n, np.float32)
    ref = R.norm(theta, g)
    assert float(np.sum(theta.astype(np.float64) ** 2)) > float(np.finfo(np.float32).max) > ref
    _, stats, _, _ = _privatise(n, 0, clip=1e6, theta=theta, g=g)
    assert math.isfinite(float(stats[0])) and abs(float(stats[0]) - ref) <= 5e-7 * ref
    assert float(stats[1]) == pytest.approx(1e6 / ref, rel=1e-6)


@gpu
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_privatise_below_the_clip_is_scale_by(n, shift):
    from fairfedmed_amd import ops
    _, _, _, start, nu = _data(n)
    out, stats, _, (th, gg, ww) = _privatise(n, shift, clip=2.0 * nu)
    want = torch.empty(n, device="cuda")
    ops.scale_by(th.clone(), ww.clone(), want)
    assert torch.equal(out, want) and float(stats[1]) == 1.0
    acc, _, _, _ = _privatise(n, shift, clip=2.0 * nu, accumulate=True)
    want = torch.from_numpy(start.copy()).cuda()
    ops.scale_acc(th.clone(), ww.clone(), want)
    assert torch.equal(acc, want)


@gpu
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_privatise_above_the_clip(n, shift):
    theta, g, w, start, nu = _data(n)
    clip = nu / 3.0
    out, stats, _, _ = _privatise(n, shift, clip=clip)
    ref, _, s = R.contribution(theta, g, w, clip)
    assert 0.0 < s < 1.0 and float(stats[1]) == pytest.approx(s, rel=2e-7)
    bound = 1e-6 * w.astype(np.float64) * np.maximum(np.abs(theta), np.abs(g)).astype(np.float64) + TINY
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print(f"clipped n={n} shift={shift}: max err / bound = {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)
    # accumulate: out = start + c with the sum rounded once more (half an ulp of the result)
    acc, _, _, _ = _privatise(n, shift, clip=clip, accumulate=True)
    want = start.astype(np.float64) + out.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(acc.cpu().numpy().astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + TINY)


@gpu
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [5, 2049])
def test_privatise_with_a_nan_and_an_inf_releases_w_times_g(n, shift):
    theta, g, w, _, nu = _data(n)
    bad = theta.copy()
    bad[n // 2] = np.nan
    bad[n - 1] = np.inf
    out, stats, _, (_, gg, ww) = _privatise(n, shift, clip=2.0 * nu, theta=bad)
    assert torch.equal(out, ww * gg) and float(stats[1]) == 0.0 and not math.isfinite(float(stats[0]))
    only_inf = theta.copy()
    only_inf[0] = -np.inf
    out, stats, _, _ = _privatise(n, shift, clip=2.0 * nu, theta=only_inf)
    assert torch.equal(out, ww * gg) and float(stats[1]) == 0.0


@gpu
@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("n", [5, 1022, 70001])
def test_privatise_with_noise_is_the_quiet_result_plus_the_noise_entry(n, clipped):
    from fairfedmed_amd import ops
    _, _, _, _, nu = _data(n)
    clip, sigma, t, k = (nu / 3.0 if clipped else 2.0 * nu), 0.02, 41, 3
    for shift in (0, 1):
        quiet, _, _, _ = _privatise(n, shift, clip=clip)
        loud, _, _, _ = _privatise(n, shift, clip=clip, sigma=sigma, t=t, k=k)
        nz = torch.empty(n, device="cuda")
        ops.dp_noise(nz, sigma, SEED, t, k)
        want = quiet.cpu().numpy().astype(np.float64) + nz.cpu().numpy().astype(np.float64)     # exact in float64
        err = np.abs(loud.cpu().numpy().astype(np.float64) - want)
        assert np.all(err <= 2.0 ** -24 * np.abs(want) + TINY)                                  # one fp32 rounding
        assert float(np.abs(nz.cpu().numpy().astype(np.float64) - float(np.float32(sigma)) * _xi(n, t, k)).max()) <= 1e-5 * sigma


@gpu
def test_aggregator_on_the_gpu_against_the_reference_and_the_cpu():
    mcfg = C.vit_b16(rank=8)
    offsets, numel = _layout(mcfg)
    assert numel == FULL
    G, r = mcfg.lora.num_groups, mcfg.lora.rank
    part, n_client, by_attr = [0, 1, 2], [120, 80, 50], [[60, 40, 20], [10, 30, 40], [5, 25, 20]]
    gen = torch.Generator().manual_seed(3)
    g = 0.05 * torch.randn(numel, generator=gen)
    thetas = [g + step * torch.randn(numel, generator=gen) for step in (1e-4, 2e-3, 1e-2)]
    norms = sorted(R.norm(th.numpy(), g.numpy()) for th in thetas)
    cfg = D.DPCfg(clip=0.5 * (norms[0] + norms[1]), noise_multiplier=0.5, seed=SEED)
    t, rounds = 2, 5

    def run(device):
        agg = FedAvgAggregator(g.clone().to(device), offsets, G, r, shared_half_s=True, dp=cfg)
        agg.begin(round=t)
        for k, th in zip(part, thetas):
            agg.add(th.to(device), k, part, n_client, by_attr)
        return agg.finish(t, rounds, grouped=True).cpu().clone(), agg.dp_stats

    got, stats = run("cuda")
    host, host_stats = run("cpu")
    ws = [element_weights(offsets, numel, k, part, n_client, by_attr).numpy() for k in part]
    sig = R.sigma(cfg.noise_multiplier, cfg.clip, R.w_max(ws), len(part))
    total, ref_stats = 0.0, {}
    for k, (th, w) in enumerate(zip(thetas, ws)):
        c, nu, s = R.contribution(th.numpy(), g.numpy(), w, cfg.clip, sig, SEED, t, k)
        total, ref_stats[k] = total + c, (nu, s)
    s_off = [off for key, (off, shp) in offsets.items() if is_group_s_block(key, shp, G)]
    assert s_off and sig > 0
    ref = R.finish(total, g.numpy(), s_off, G, r, True, 0.999 * t / rounds)
    assert [ref_stats[k][1] == 1.0 for k in part] == [True, False, False]
    assert np.allclose(got.numpy().astype(np.float64), ref, rtol=1e-5, atol=1e-7 + 1e-5 * sig)
    assert torch.allclose(got, host, rtol=1e-5, atol=1e-7 + 1e-5 * sig)
    for k in part:
        assert stats[k][0] == pytest.approx(ref_stats[k][0], rel=5e-7) and stats[k][1] == pytest.approx(ref_stats[k][1], rel=1e-6)
        assert host_stats[k][0] == pytest.approx(ref_stats[k][0], rel=5e-7)


@gpu
def test_drivers_on_the_hip_trainer_with_dp():
    """The round loop on the real trainer (device-resident flat buffer): with a clip that never binds and no noise the
    one-process driver's flat-buffer boundary reproduces its average_weights_ema result; with clip and noise on, the
    one-process driver and the torch.distributed driver (world 1) release the same weights."""
    import os
    import torch.distributed as dist
    from fairfedmed_amd import federated as F
    from tests.test_trainer_gpu import _fed_setup, rel

    def args(**kw):
        return F.FedArgs(num_users=2, frac=1.0, round=2, shared_half_s=True, seed=0, **kw)

    plain = F.run_fedotplora(_fed_setup(), args(), log=lambda *_: None)
    loose = F.run_fedotplora(_fed_setup(), args(dp_clip=1e9), log=lambda *_: None)
    assert "dp_norms" not in plain and len(loose["dp_norms"]) == 2 and loose["dp_epsilon"] == [math.inf, math.inf]
    for k, v in plain["global_weights"].items():
        assert rel(loose["global_weights"][k], v) < 1e-5, k
    norms = [v for r in loose["dp_norms"] for v in r.values()]
    assert all(math.isfinite(v) and v > 0 for v in norms)
    first = sorted(loose["dp_norms"][0].values())                             # round 0 starts from the same weights in every run
    on = args(dp_clip=0.5 * (first[0] + first[1]), dp_noise=0.5)              # one of its two updates passes, one is clipped
    one = F.run_fedotplora(_fed_setup(), on, log=lambda *_: None)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        tr = _fed_setup()
        ranks = F.run_fedotplora_ranks(tr, on, log=lambda *_: None)
    finally:
        if created:
            dist.destroy_process_group()
    seen = [v for r in one["dp_norms"] for v in r.values()]
    assert min(seen) <= on.dp_clip < max(seen)
    for a, b in zip(one["dp_norms"], ranks["dp_norms"]):
        assert sorted(a) == sorted(b) == [0, 1] and all(a[c] == pytest.approx(b[c], rel=1e-5) for c in a)
    assert one["dp_epsilon"] == ranks["dp_epsilon"] == [D.epsilon(0.5, 1, 1e-5), D.epsilon(0.5, 2, 1e-5)]
    moved = 0.0
    for k, v in one["global_weights"].items():
        off, shp = tr.engine.params.offsets[k]
        got = ranks["global_flat"][off:off + v.numel()].view(shp).cpu()
        assert bool(torch.isfinite(got).all()) and rel(got, v.cpu()) < 1e-5, k
        moved = max(moved, float((v.cpu() - loose["global_weights"][k].cpu()).abs().max()))
    assert moved > 0                                                          # the clip and the noise reached the weights


def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    p = 4096                                         # a non-NULL address: every call below returns before touching it
    assert lib.ffm_dp_norm(None, p, 4, p, None) == -1 and lib.ffm_dp_norm(p, None, 4, p, None) == -1
    assert lib.ffm_dp_norm(p, p, 4, None, None) == -1 and lib.ffm_dp_norm(p, p, 0, p, None) == -1
    ok = [p, p, p, p, 4, p, 1.0, 0.0, 7, 0, 0, 0, None, None]
    for i in (0, 1, 2, 3, 5):
        a = list(ok)
        a[i] = None
        assert lib.ffm_dp_privatise(*a) == -1, i
    for i, v in ((4, 0), (4, -3), (6, 0.0), (6, -1.0), (6, float("nan")), (7, -0.5), (7, float("nan")), (7, float("inf"))):
        a = list(ok)
        a[i] = v
        assert lib.ffm_dp_privatise(*a) == -1, (i, v)
    assert lib.ffm_dp_noise(None, 4, 1.0, 7, 0, 0, None) == -1 and lib.ffm_dp_noise(p, 0, 1.0, 7, 0, 0, None) == -1
    assert lib.ffm_dp_noise(p, 4, -1.0, 7, 0, 0, None) == -1
    assert lib.ffm_dp_philox(None, 4, 7, 0, 0, 0, 0, None) == -1 and lib.ffm_dp_philox(p, 0, 7, 0, 0, 0, 0, None) == -1
    assert lib.ffm_dp_norm_ws_bytes(0) == -1 and lib.ffm_dp_norm_ws_bytes(FULL) == 8 * 256
