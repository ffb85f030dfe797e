"""Client-level differential privacy at the round boundary, on the CPU: the generator's known answers, the host restatement
(fairfedmed_amd/dp.py) against the float64 reference of tests/dp_ref.py, the accounting, FedAvgAggregator(dp=...) on CPU
tensors, and the two drivers - two gloo ranks against one process - with noise on."""
import math
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fairfedmed_amd import config as C
from fairfedmed_amd import dp as D
from fairfedmed_amd.fedavg import FedAvgAggregator, element_weights, is_group_s_block
from tests import dp_ref as R
from tests.test_fedavg_gloo import _FlatTrainer, _client_state, _flatten, _free_port, _layout

N3 = [120, 80, 50]
BY3 = [[60, 40, 20], [10, 30, 40], [5, 25, 20]]
PART = [0, 1, 2]
STEP = [0.02, 0.3, 1.0]                   # client k's update is STEP[k] * (a random state - g): three well separated norms


def _setup():
    mcfg = C.vit_tiny(rank=4)
    offsets, numel = _layout(mcfg)
    g = _flatten(_client_state(mcfg, 99, 0), offsets, numel)
    thetas = [g + STEP[k] * (_flatten(_client_state(mcfg, k, 0), offsets, numel) - g) for k in PART]
    ws = [element_weights(offsets, numel, k, PART, N3, BY3) for k in PART]
    return mcfg, offsets, numel, g, thetas, ws


def _run(g, offsets, mcfg, thetas, dp, t=1, rounds=3):
    agg = FedAvgAggregator(g.clone(), offsets, mcfg.lora.num_groups, mcfg.lora.rank, shared_half_s=True, dp=dp)
    agg.begin(round=t)
    for k, th in zip(PART, thetas):
        agg.add(th, k, PART, N3, BY3)
    return agg.finish(t, rounds, grouped=True).clone(), agg


def _ref(g, offsets, mcfg, thetas, ws, clip, z, seed, t=1, rounds=3):
    sig = R.sigma(z, clip, R.w_max([w.numpy() for w in ws]), len(PART))
    total, stats = 0.0, {}
    for k, (th, w) in enumerate(zip(thetas, ws)):
        c, nu, s = R.contribution(th.numpy(), g.numpy(), w.numpy(), clip, sig, seed, t, k)
        total, stats[k] = total + c, (nu, s)
    G, r = mcfg.lora.num_groups, mcfg.lora.rank
    s_off = [off for key, (off, shp) in offsets.items() if is_group_s_block(key, shp, G)]
    return R.finish(total, g.numpy(), s_off, G, r, True, 0.999 * t / rounds), stats, sig


@pytest.mark.parametrize("philox", [R.philox_one, lambda c, k: tuple(int(v) for v in D.philox4x32_10(np.array(c, np.uint32), k)[0])],
                         ids=["dp_ref", "fairfedmed_amd.dp"])
def test_philox_known_answers(philox):
    for counter, key, out in R.KAT:
        assert tuple(philox(counter, key)) == out
    # ... and the two vectorised word streams are the block function, lane by lane, low word of the seed first
    seed = 0x299f31d0a4093822
    got_r, got_d = R.words(9, seed, 0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), D.philox_words(9, seed, 0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)
    assert tuple(int(v) for v in got_r[:4]) == R.KAT[2][2] and np.array_equal(got_r, got_d)
    assert tuple(int(v) for v in got_r[4:8]) == R.philox_one((0x243f6a89, 0x85a308d3, 0x13198a2e, 0x03707344), R.KAT[2][1])


def test_host_gaussian_against_the_float64_reference():
    n = 1 << 20
    got = D.gaussians(n, 7, 3, 2)
    ref = R.gaussians(n, 7, 3, 2)
    assert got.dtype == np.float32 and np.all(np.isfinite(got))
    dev = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"host Gaussian: max |fp32 - fp64| = {dev:.3e}")
    assert dev <= 1e-5
    assert abs(float(ref.mean())) < 5e-3 and abs(float(ref.std()) - 1.0) < 5e-3          # five sigma of either estimate
    sig = 0.37
    assert torch.equal(D.noise(1001, sig, 7, 3, 2), torch.from_numpy(np.float32(sig) * got[:1001]))


def test_epsilon_is_the_zcdp_closed_form():
    for z, rounds, delta in [(1.0, 10, 1e-5), (0.5, 3, 1e-5), (4.0, 200, 1e-6)]:
        rho = rounds / (2 * z * z)
        assert D.epsilon(z, rounds, delta) == pytest.approx(rho + 2 * math.sqrt(rho * math.log(1 / delta)), rel=1e-12)
    eps = [D.epsilon(1.3, r, 1e-5) for r in range(0, 12)]
    assert eps[0] == 0.0 and all(a < b for a, b in zip(eps, eps[1:]))
    assert D.epsilon(0.0, 5, 1e-5) == math.inf
    with pytest.raises(ValueError):
        D.DPCfg(clip=0.0)
    with pytest.raises(ValueError):
        D.DPCfg(clip=1.0, noise_multiplier=-1.0)


@pytest.mark.parametrize("z", [0.0, 0.5])
def test_aggregator_on_the_cpu_against_the_reference(z):
    mcfg, offsets, numel, g, thetas, ws = _setup()
    norms = sorted(R.norm(th.numpy(), g.numpy()) for th in thetas)
    clip = 0.5 * (norms[0] + norms[1])                   # the smallest update passes, the other two are clipped
    got, agg = _run(g, offsets, mcfg, thetas, D.DPCfg(clip=clip, noise_multiplier=z, seed=11))
    ref, stats, sig = _ref(g, offsets, mcfg, thetas, ws, clip, z, 11)
    scales = [stats[k][1] for k in PART]
    assert any(s == 1.0 for s in scales) and any(0.0 < s < 1.0 for s in scales)
    assert (sig > 0) == (z > 0)
    # rtol / atol of test_fedavg_gloo.py; each unit of sigma adds the host Gaussian's 1e-5 bound
    assert np.allclose(got.numpy().astype(np.float64), ref, rtol=1e-5, atol=1e-7 + 1e-5 * sig)
    for k in PART:
        nu, s = agg.dp_stats[k]
        assert nu == pytest.approx(stats[k][0], rel=1e-6) and s == pytest.approx(stats[k][1], rel=1e-6)
    if z > 0:                                            # the noise is really there: the result moved by about sigma sqrt(K)
        quiet, _ = _run(g, offsets, mcfg, thetas, D.DPCfg(clip=clip, seed=11))
        moved = float((got - quiet).std())
        assert 0.3 * sig < moved < 3.0 * sig * math.sqrt(len(PART))


def test_clip_not_binding_without_noise_changes_no_bit():
    mcfg, offsets, numel, g, thetas, ws = _setup()
    clip = 10.0 * max(R.norm(th.numpy(), g.numpy()) for th in thetas)
    plain, _ = _run(g, offsets, mcfg, thetas, None)
    got, agg = _run(g, offsets, mcfg, thetas, D.DPCfg(clip=clip))
    assert torch.equal(got, plain)
    assert all(s == 1.0 for _, s in agg.dp_stats.values())


def test_a_nan_in_one_client_counts_as_a_zero_update():
    mcfg, offsets, numel, g, thetas, ws = _setup()
    clip = 10.0 * max(R.norm(th.numpy(), g.numpy()) for th in thetas)
    bad = [th.clone() for th in thetas]
    bad[1][numel - 3] = float("nan")
    bad[1][7] = float("inf")
    got, agg = _run(g, offsets, mcfg, bad, D.DPCfg(clip=clip))
    zeroed, _ = _run(g, offsets, mcfg, [thetas[0], g.clone(), thetas[2]], D.DPCfg(clip=clip))
    assert bool(torch.isfinite(got).all()) and torch.equal(got, zeroed)
    assert agg.dp_stats[1][1] == 0.0 and not math.isfinite(agg.dp_stats[1][0])
    assert agg.dp_stats[0][1] == 1.0 == agg.dp_stats[2][1]


def test_noise_streams_are_named_by_seed_round_and_client():
    n = 4099
    a = D.noise(n, 1.0, 5, 2, 1)
    assert torch.equal(a, D.noise(n, 1.0, 5, 2, 1))
    for other in (D.noise(n, 1.0, 6, 2, 1), D.noise(n, 1.0, 5, 3, 1), D.noise(n, 1.0, 5, 2, 0), D.noise(n, 1.0, 5 + (1 << 32), 2, 1)):
        assert float((a - other).abs().max()) > 1.0 and int((a == other).sum()) < n // 100
    # element i of a stream does not depend on how many elements are drawn
    assert torch.equal(a[:1001], D.noise(1001, 1.0, 5, 2, 1))
    # through the aggregator: the same round twice gives the same bits, another round another draw
    mcfg, offsets, numel, g, thetas, ws = _setup()
    cfg = D.DPCfg(clip=1.0, noise_multiplier=1.0, seed=3)
    r1, _ = _run(g, offsets, mcfg, thetas, cfg, t=1)
    r1b, _ = _run(g, offsets, mcfg, thetas, cfg, t=1)
    r2, _ = _run(g, offsets, mcfg, thetas, cfg, t=2, rounds=6)         # the same EMA factor, another stream
    assert torch.equal(r1, r1b) and not torch.equal(r1, r2)
    with pytest.raises(ValueError):
        FedAvgAggregator(g.clone(), offsets, 3, 4, dp=cfg).begin()   # the round must be named


# ----------------------------------------------------------------------------------------------------------------
# the two drivers: three clients dealt to two gloo ranks against the one-process loop, clip and noise on
# ----------------------------------------------------------------------------------------------------------------
DP_CLIP, DP_NOISE = 1.0, 0.5           # the stand-in trainer's updates have norms 0.7 .. 2.4: some pass, some are clipped


def _fed_args():
    from fairfedmed_amd import federated as F
    return F.FedArgs(num_users=3, frac=0.7, round=3, shared_half_s=True, seed=5, dp_clip=DP_CLIP, dp_noise=DP_NOISE)


def _dp_worker(rank, world, port, outdir):
    from fairfedmed_amd import federated as F
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    hist = F.run_fedotplora_ranks(_FlatTrainer(3), _fed_args(), log=lambda *_: None)
    torch.save({"flat": hist["global_flat"], "norms": hist["dp_norms"], "eps": hist["dp_epsilon"]},
               os.path.join(outdir, f"dp{rank}.pt"))
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_the_one_process_driver_with_noise():
    from fairfedmed_amd import federated as F
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dp_worker, args=(2, _free_port(), d), nprocs=2, join=True)
        got = [torch.load(os.path.join(d, f"dp{r}.pt")) for r in range(2)]
    assert torch.equal(got[0]["flat"], got[1]["flat"]) and got[0]["norms"] == got[1]["norms"]
    tr = _FlatTrainer(3)
    lines = []
    hist = F.run_fedotplora(tr, _fed_args(), log=lines.append)
    p = tr.engine.params
    for k, v in hist["global_weights"].items():
        o, s = p.offsets[k]
        ref = v.reshape(-1)
        assert torch.allclose(got[0]["flat"][o:o + ref.numel()], ref, rtol=1e-5, atol=1e-7), k
    # the accounting: one dict of norms per round, the same clients with the same norms in both drivers, some clipped and
    # some not, and the running bound of `epsilon`
    assert len(hist["dp_norms"]) == 3 == len(got[0]["norms"])
    for a, b in zip(hist["dp_norms"], got[0]["norms"]):
        assert sorted(a) == sorted(b) and all(a[c] == pytest.approx(b[c], rel=1e-5) for c in a)
    assert sorted(hist["dp_norms"][0]) == [0, 1, 2] and all(len(r) == 2 for r in hist["dp_norms"][1:])     # frac 0.7 of 3
    every = [v for r in hist["dp_norms"] for v in r.values()]
    assert min(every) <= DP_CLIP < max(every)
    assert hist["dp_epsilon"] == got[0]["eps"] == [D.epsilon(DP_NOISE, r + 1, 1e-5) for r in range(3)]
    assert any("epsilon" in str(l) for l in lines)
    # and the noise is in the result: the same run without it differs by far more than the tolerance above
    tr0 = _FlatTrainer(3)
    args0 = _fed_args()
    args0.dp_noise = 0.0
    h0 = F.run_fedotplora(tr0, args0, log=lambda *_: None)
    k = "prompt_learner.ctx"
    assert float((h0["global_weights"][k] - hist["global_weights"][k]).abs().max()) > 1e-3


def test_flags_reach_fedargs_and_batchnorm_buffers_are_refused():
    from fairfedmed_amd import federated as F
    from fairfedmed_amd import federated_main as M
    a = M.fed_args(M.build_parser().parse_args(["--num_users", "3", "--dp_clip", "2.5", "--dp_noise", "0.8", "--dp_seed", "77",
                                                "--dp_delta", "1e-6", "--seed", "4"]))
    assert (a.dp_clip, a.dp_noise, a.dp_seed, a.dp_delta, a.seed) == (2.5, 0.8, 77, 1e-6, 4)
    assert F.dp_config(a) == D.DPCfg(clip=2.5, noise_multiplier=0.8, seed=77, delta=1e-6)
    b = M.fed_args(M.build_parser().parse_args(["--num_users", "3", "--seed", "4"]))
    assert (b.dp_clip, b.dp_noise, b.dp_seed, b.dp_delta) == (0.0, 0.0, None, 1e-5) and F.dp_config(b) is None
    assert F.FedArgs(num_users=2).dp_clip == 0.0
    assert F.dp_config(F.FedArgs(num_users=2, seed=9, dp_clip=1.0)).seed == 9          # dp_seed defaults to seed ...
    assert F.dp_config(F.FedArgs(num_users=2, dp_clip=1.0)).seed == 0                  # ... else 0
    tr = _FlatTrainer(3)
    tr.engine.buffers_flat = lambda: torch.zeros(4)                                    # the RN50 engine's surface
    with pytest.raises(ValueError, match="BatchNorm"):
        F.dp_config(_fed_args(), tr)
    before = tr.engine.params.flat.clone()
    with pytest.raises(ValueError, match="BatchNorm"):
        F.run_fedotplora(tr, _fed_args(), log=lambda *_: None)
    assert torch.equal(tr.engine.params.flat, before)                                  # refused before anything trained
    args = _fed_args()
    args.dp_clip = 0.0                                                                 # off: the same trainer is fine
    assert F.dp_config(args, tr) is None


def test_abi_is_additive_and_validates_without_a_gpu():
    from fairfedmed_amd import _lib
    from fairfedmed_amd import build as B
    lib = _lib.load()
    assert lib.ffm_abi_version() == 14
    assert "dp.hip" in B.SOURCES and "dp.hip" not in B.TWIN_SOURCES
    for name in ("ffm_dp_norm_ws_bytes", "ffm_dp_norm", "ffm_dp_privatise", "ffm_dp_noise", "ffm_dp_philox"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ffm_dp_norm_ws_bytes(741952) > 0 and lib.ffm_dp_norm_ws_bytes(741952) % 8 == 0
    assert lib.ffm_dp_norm_ws_bytes(1) == 8 and lib.ffm_dp_norm_ws_bytes(0) == -1
    assert lib.ffm_dp_norm(None, None, 4, None, None) == -1
