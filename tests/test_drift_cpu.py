"""Client-drift correction in the local step (fairfedmed_amd/drift.py, ffm_drift_correct) without a
GPU: the entry point's argument checks, the host twin against the float64 formulas of tests/drift_ref.py, the behaviour on
heterogeneous quadratics through the real FedAvgAggregator, the round protocol, both drivers (world 2 over gloo against one
process) and the command line."""
import ctypes
import os
import socket
import tempfile
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fairfedmed_amd import _lib
from fairfedmed_amd import drift as D
from fairfedmed_amd.fedavg import FedAvgAggregator
from tests import drift_ref as R

F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the entry point
# ---------------------------------------------------------------------------------------------------------------------
def test_drift_source_is_built_once_and_bound():
    from fairfedmed_amd import build as B
    assert "drift.hip" in B.SOURCES and "drift.hip" not in B.TWIN_SOURCES
    protos = {n: (rt, params) for rt, n, params in B.api_prototypes()}
    rt, params = protos["ffm_drift_correct"]
    assert rt == "int" and [a for _, a in params] == ["g", "p", "anchor", "mu", "c_diff", "gsum", "count", "scale_state", "n",
                                                      "stream"]
    assert len(_lib.SIGNATURES["ffm_drift_correct"]) == len(params)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ffm_drift_correct")
    assert _lib.ABI_VERSION == 14 == _lib.load().ffm_abi_version()          # additive: the version stays


def test_argument_checks_need_no_gpu():
    """Every refusal of include/ffm_hip.h comes back before anything is launched: the pointers below are never dereferenced."""
    f = _lib.load().ffm_drift_correct
    P = 0x1000                                        # a non-NULL, 16-byte aligned address that is never read
    inf, nan = float("inf"), float("nan")
    #        g     p     anchor mu   c_diff gsum  count st    n
    einval = {
        "g NULL": (None, P, P, 0.5, None, None, None, None, 8),
        "n == 0": (P, P, P, 0.5, None, None, None, None, 0),
        "n < 0": (P, P, P, 0.5, None, None, None, None, -3),
        "mu inf": (P, P, P, inf, None, None, None, None, 8),
        "mu -inf": (P, P, P, -inf, None, None, None, None, 8),
        "mu nan": (P, P, P, nan, None, None, None, None, 8),
        "anchor without p": (P, None, P, 0.5, None, None, None, None, 8),
        "mu != 0 without anchor": (P, P, None, 0.5, P, None, None, None, 8),
        "gsum without count": (P, None, None, 0.0, P, P, None, None, 8),
        "count without gsum": (P, None, None, 0.0, P, None, P, None, 8),
        "no operand": (P, None, None, 0.0, None, None, None, None, 8),
        "no operand, p alone": (P, P, None, 0.0, None, None, None, P, 8),
    }
    for what, a in einval.items():
        assert f(*a, None) == -1, what
    assert f(P, None, None, 0.0, P, None, None, None, (1 << 34) + 1, None) == -2      # FFM_EUNSUP: the size limit of dp.hip
    assert f(P, None, None, 0.0, P, None, None, None, 0, None) == -1                  # (n <= 0 comes first)


def test_cfg_refuses_what_it_cannot_mean():
    for bad in (dict(name="fedavg"), dict(name="fedprox", mu=-0.1), dict(name="fedprox", mu=float("nan")),
                dict(name="fedprox", mu=float("inf"))):
        with pytest.raises(ValueError):
            D.DriftCfg(**bad)
    assert D.DriftCfg().name == "none" and D.DriftCfg("scaffold").mu == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the host twin, one application, against the float64 formula
# ---------------------------------------------------------------------------------------------------------------------
def _operands(n, seed):
    """Mixed magnitudes (2^-20 .. 2^10), p close to anchor (a cancelling difference), a few exact zeros and -0.0."""
    gen = torch.Generator().manual_seed(seed)
    mag = lambda: torch.exp2(torch.randint(-20, 11, (n,), generator=gen).to(F32))
    g = torch.randn(n, generator=gen) * mag()
    anchor = torch.randn(n, generator=gen) * mag()
    p = anchor + torch.randn(n, generator=gen) * mag() * 2.0 ** -6
    c_diff = torch.randn(n, generator=gen) * mag()
    gsum = torch.randn(n, generator=gen) * mag()
    for t in (g, c_diff, gsum):
        t[::97] = 0.0
    g[5::193] = -0.0
    return g, p, anchor, c_diff, gsum


@pytest.mark.parametrize("mode", ["anchor", "c_diff", "gsum", "all"])
@pytest.mark.parametrize("mu", [0.5, 0.01, 3.0])
def test_host_twin_against_float64(mode, mu):
    """|got - ref| <= 2^-22 (|g| + |mu (p - anchor)| + |c_diff|) per element: four roundings of at most 2^-24 relative each
    (drift_ref.bound); the running sum is one rounding of gsum + raw."""
    n = 4099
    g, p, anchor, c_diff, gsum = _operands(n, seed=11)
    kw, ref_kw = {}, {}
    if mode in ("anchor", "all"):
        kw.update(p=p, anchor=anchor, mu=mu)
        ref_kw.update(p=p.numpy(), anchor=anchor.numpy(), mu=mu)
    if mode in ("c_diff", "all"):
        kw.update(c_diff=c_diff)
        ref_kw.update(c_diff=c_diff.numpy())
    count = torch.tensor([41], dtype=torch.int64)
    if mode in ("gsum", "all"):
        kw.update(gsum=gsum.clone(), count=count)
    raw = g.clone()
    frozen = {k: v.clone() for k, v in kw.items() if k in ("p", "anchor", "c_diff")}
    D.host_correct(g, **kw)
    ref, tol = R.correct(raw.numpy(), **ref_kw), R.bound(raw.numpy(), **ref_kw)
    err = np.abs(g.numpy().astype(np.float64) - ref)
    assert (err <= tol).all(), (float((err - tol).max()), int((err > tol).sum()))
    if mode == "gsum":
        assert torch.equal(g, raw)                                    # nothing is added: the gradient keeps its bits
    if "gsum" in kw:
        s_ref = gsum.numpy().astype(np.float64) + raw.numpy().astype(np.float64)
        assert (np.abs(kw["gsum"].numpy().astype(np.float64) - s_ref) <= 2.0 ** -24 * np.abs(s_ref)).all()
        assert int(count) == 42
    else:
        assert int(count) == 41
    for k, v in frozen.items():
        assert torch.equal(kw[k], v), f"{k} is an input"


def test_host_twin_skips_an_overflowed_step_bit_for_bit():
    g, p, anchor, c_diff, gsum = _operands(1021, seed=12)
    g[7] = float("inf")
    st = torch.tensor([4096.0, 1 / 4096.0, 0.0, 0.0, 0.0, 4096.0, 2000.0, 1.0])
    count = torch.tensor([3], dtype=torch.int64)
    g0, s0 = g.clone(), gsum.clone()
    bits = lambda t: t.view(torch.int32)
    D.host_correct(g, p=p, anchor=anchor, mu=0.5, c_diff=c_diff, gsum=gsum, count=count, scale_state=st)
    assert torch.equal(bits(g), bits(g0)) and torch.equal(bits(gsum), bits(s0)) and int(count) == 3
    st[2] = 1.0
    D.host_correct(g, p=p, anchor=anchor, mu=0.5, c_diff=c_diff, gsum=gsum, count=count, scale_state=st)
    assert int(count) == 4 and not torch.equal(bits(gsum), bits(s0))


# ---------------------------------------------------------------------------------------------------------------------
# a stub trainer on heterogeneous quadratics: engine.params.flat, plain SGD, the correction where the engine applies it
# ---------------------------------------------------------------------------------------------------------------------
KEY = "prompt_learner.ctx"


class _QuadEngine:
    def __init__(self, d):
        # (one trainable tensor, under the name and shape the drivers expect of the prompts: [num_prompt, ...])
        self.params = NS(flat=torch.zeros(d), grad=torch.zeros(d), offsets={KEY: (0, (2, d // 2))}, keys=[KEY])
        self.cfg = NS(lora=NS(num_groups=1, rank=1))
        self._drift = self.last_drift = None

    def set_drift(self, corr):
        self._drift = corr
        if corr is not None:
            self.last_drift = corr

    def forward_backward(self, A, b):
        p = self.params
        torch.mul(A, p.flat - b, out=p.grad)                           # the gradient of 1/2 (x - b)^T A (x - b)
        if self._drift is not None:
            self._drift.apply(p.grad, p.flat, None)

    def sgd_step(self, lr):
        self.params.flat.sub_(self.params.grad * lr)


class _QuadTrainer:
    """What the drivers ask of a trainer, around _QuadEngine: train(idx) is K steps of plain SGD on client idx's quadratic."""

    def __init__(self, A, b, K=10, lr=0.05):
        self.A, self.b = torch.tensor(A, dtype=F32), torch.tensor(b, dtype=F32)
        self.K, self.lr = K, lr
        users, d = self.A.shape
        self.engine = _QuadEngine(d)
        self.cfg = NS(DATASET=NS(USERS=users, ATTRIBUTE_TYPE="race"))
        self.fed_train_loader_x_dict = {
            i: NS(dataset=type("D", (), {"__len__": lambda s: 10, "count_by_attribute": lambda s, a: [10]})())
            for i in range(users)}
        eng = self.engine

        class _Model:
            def state_dict(self):
                return {KEY: eng.params.flat.view(2, -1)}

            def load_state_dict(self, sd, strict=True):
                eng.params.flat.copy_(sd[KEY].reshape(-1))
        self.model = _Model()

    def fed_before_train(self): pass
    def fed_after_train(self): pass

    def train(self, idx, global_epoch=0, is_fed=True, is_last_client=False):
        for _ in range(self.K):
            self.engine.forward_backward(self.A[idx], self.b[idx])
            self.engine.sgd_step(self.lr)

    def test(self, idx, current_epoch=0):
        return [float(self.engine.params.flat.sum()), 0.0, 0.0, 0.5]


def _federate(mode, mu=0.0, rounds=200, sample=None):
    """4 clients, d = 8, equal counts, K = 10 local steps at lr 0.05 from 0, through FedAvgAggregator(beta=0, no
    shared_half_s); sample: clients drawn per round (None: all).  Returns (distance to the pooled optimum, corrector)."""
    A, b, rng = R.quadratics(4, 8, seed=0)
    tr = _QuadTrainer(A, b, K=10, lr=0.05)
    flat = tr.engine.params.flat
    agg = FedAvgAggregator(flat, tr.engine.params.offsets, 1, 1, shared_half_s=False, beta=0.0)
    corr = D.DriftCorrector(flat, 4, D.DriftCfg(mode, mu))
    tr.engine.set_drift(corr if mode != "none" else None)
    for r in range(rounds):
        part = list(range(4)) if sample is None else sorted(int(i) for i in rng.choice(4, sample, replace=False))
        agg.begin()
        for idx in part:
            flat.copy_(agg.global_prev)
            corr.begin_client(idx)
            tr.train(idx)
            corr.end_client(idx)
            agg.add(flat, idx, part, [10] * 4, None)
        agg.finish(r, rounds)
        corr.finish_round(part)
    x = agg.global_prev.numpy().astype(np.float64)
    return float(np.linalg.norm(x - R.pooled_optimum(A, b))), corr


@pytest.mark.parametrize("rounds,sample", [(200, None), (400, 2)], ids=["all_clients", "2_of_4"])
def test_scaffold_reaches_the_pooled_optimum_where_fedavg_does_not(rounds, sample):
    """Plain FedAvg with 10 local steps settles >= 1e-2 away from the optimum of the pooled objective (a float32 numpy probe
    gave 8.5e-2 with every client, 0.47 with 2 of 4 drawn per round; |x*| = 1.80); with the control variates the distance is
    <= 1e-4 (probe: 1.0e-6 and 8.6e-7)."""
    none, _ = _federate("none", rounds=rounds, sample=sample)
    scaf, corr = _federate("scaffold", rounds=rounds, sample=sample)
    print(f"distance to the pooled optimum: none {none:.3e}  scaffold {scaf:.3e}")
    assert none >= 1e-2, none
    assert scaf <= 1e-4, scaf
    assert float(corr.c.abs().max()) > 0


def test_fedprox_pulls_towards_the_start_of_the_round():
    """One client-round from the same start: every step's gradient carries mu (x - anchor), so the client ends closer to
    where it started than without the term, and mu = 0 adds exactly nothing."""
    A, b, _ = R.quadratics(4, 8, seed=0)
    ends = {}
    for mu in (None, 0.0, 0.5):
        tr = _QuadTrainer(A, b)
        flat = tr.engine.params.flat
        flat.fill_(0.25)
        if mu is not None:
            corr = D.DriftCorrector(flat, 4, D.DriftCfg("fedprox", mu))
            tr.engine.set_drift(corr)
            corr.begin_client(2)
            assert torch.equal(corr.anchor, flat)
        tr.train(2)
        ends[mu] = flat.clone()
    assert torch.equal(ends[0.0], ends[None])
    assert float((ends[0.5] - 0.25).norm()) < float((ends[None] - 0.25).norm())


# ---------------------------------------------------------------------------------------------------------------------
# the round protocol
# ---------------------------------------------------------------------------------------------------------------------
def test_round_protocol_rows_and_global_variate():
    A, b, _ = R.quadratics(4, 8, seed=0)
    tr = _QuadTrainer(A, b)
    flat = tr.engine.params.flat
    corr = D.DriftCorrector(flat, 4, D.DriftCfg("scaffold"))
    for t in (corr.anchor, corr.c_diff, corr.gsum, corr.c, corr.c_i, corr.count):
        assert t.device == flat.device and not bool(t.any())
    assert corr.count.dtype == torch.int64 and corr.c_i.shape == (4, 8)
    ptrs = [t.data_ptr() for t in (corr.anchor, corr.c_diff, corr.gsum, corr.c, corr.c_i, corr.count)]
    tr.engine.set_drift(corr)
    ref = R.Scaffold(4, 8)

    def client(idx, steps=True):
        flat.zero_()
        corr.begin_client(idx)
        cd = ref.begin(idx)
        assert np.abs(corr.c_diff.numpy() - cd).max() <= 1e-5
        if steps:
            for _ in range(tr.K):
                raw = (tr.A[idx] * (flat - tr.b[idx])).clone()
                ref.step(raw.numpy())
                tr.engine.forward_backward(tr.A[idx], tr.b[idx])
                assert torch.equal(tr.engine.params.grad, raw + corr.c_diff)
                tr.engine.sgd_step(tr.lr)
        corr.end_client(idx)
        ref.end(idx)

    # round 0, every client: c is the ascending-order mean of the rows
    for idx in (2, 0, 3, 1):                                          # (the order of training does not enter)
        client(idx)
    info = corr.finish_round([2, 0, 3, 1])
    ref.finish([0, 1, 2, 3])
    assert info["steps"] == {0: 10, 1: 10, 2: 10, 3: 10} and info["c_norm"] == float(corr.c.norm()) > 0
    four = torch.tensor(4.0)
    mean = torch.zeros(8)
    for i in range(4):
        mean = mean + corr.c_i[i] / four
    assert torch.equal(corr.c, mean)
    # round 1: client 1 makes steps, client 3 makes none (its row stays), clients 0 and 2 sit out (untouched)
    rows = corr.c_i.clone()
    client(1)
    client(3, steps=False)
    info = corr.finish_round([1, 3])
    ref.finish([1, 3])
    assert info["steps"] == {1: 10, 3: 0}
    for i in (0, 2, 3):
        assert torch.equal(corr.c_i[i], rows[i]), i
    assert not torch.equal(corr.c_i[1], rows[1])
    assert torch.equal(corr.c, mean + (corr.c_i[1] - rows[1]) / four)
    # against the float64 protocol: two rounds of ten float32 steps each, every value O(1) - rounding alone, far below 1e-5
    assert np.abs(corr.c.numpy() - ref.c).max() <= 1e-5 and np.abs(corr.c_i.numpy() - ref.c_i).max() <= 1e-5
    assert ptrs == [t.data_ptr() for t in (corr.anchor, corr.c_diff, corr.gsum, corr.c, corr.c_i, corr.count)]


# ---------------------------------------------------------------------------------------------------------------------
# both drivers: world 2 over gloo against one process
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fed_args(**kw):
    from fairfedmed_amd import federated as F
    return F.FedArgs(num_users=3, round=3, seed=5, **kw)


def _three_clients():
    A, b, _ = R.quadratics(3, 8, seed=0)
    return _QuadTrainer(A, b)


def _rank_worker(rank, world, port, outdir):
    from fairfedmed_amd import federated as F
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = _three_clients()
    hist = F.run_fedotplora_ranks(tr, _fed_args(drift="scaffold"), log=lambda *_: None)
    corr = tr.engine.last_drift
    torch.save({"flat": hist["global_flat"], "c": corr.c, "c_i": corr.c_i, "drift": hist["drift"],
                "off": tr.engine._drift is None}, os.path.join(outdir, f"r{rank}.pt"))
    dist.destroy_process_group()


_RUNS = {}


def _both_drivers():
    """(what the two ranks saved, the one-process history, its corrector): run once, shared by the tests below."""
    if not _RUNS:
        from fairfedmed_amd import federated as F
        with tempfile.TemporaryDirectory() as d:
            mp.spawn(_rank_worker, args=(2, _free_port(), d), nprocs=2, join=True)
            got = [torch.load(os.path.join(d, f"r{r}.pt")) for r in range(2)]
        tr = _three_clients()
        hist = F.run_fedotplora(tr, _fed_args(drift="scaffold"), log=lambda *_: None)
        assert tr.engine._drift is None                               # set_drift(None) at the end
        _RUNS["v"] = (got, hist, tr.engine.last_drift)
    return _RUNS["v"]


def test_scaffold_over_two_ranks_is_identical_on_both_ranks():
    """Three clients dealt to two ranks: global weights, c and c_i identical (torch.equal) on both ranks, every client's ten
    steps counted in every round, and all three within the tolerance tests/test_fedavg_gloo.py holds the two drivers to."""
    got, hist, corr = _both_drivers()
    for k in ("flat", "c", "c_i"):
        assert torch.equal(got[0][k], got[1][k]), f"ranks disagree on {k}"
    assert got[0]["drift"] == got[1]["drift"] and len(got[0]["drift"]) == 3 and got[0]["off"] and got[1]["off"]
    assert all(info["steps"] == {0: 10, 1: 10, 2: 10} for info in got[0]["drift"] + hist["drift"])
    for k, one in (("flat", hist["global_weights"][KEY].reshape(-1)), ("c", corr.c), ("c_i", corr.c_i)):
        assert torch.allclose(got[0][k], one, rtol=1e-5, atol=1e-7), k


def test_scaffold_over_two_ranks_equals_the_single_process_driver():
    """The same run against run_fedotplora in one process: torch.equal on the global weights, c and c_i.

    Without a correction the all-reduce of the per-rank partial sums forms (w0 x0 + w2 x2) + w1 x1 where one process forms
    (w0 x0 + w1 x1) + w2 x2 (tests/test_fedavg_gloo.py compares the two drivers with rtol 1e-5 for that reason; summed that
    way this run was 6.0e-8 / 3.0e-8 / 1.2e-7 off after three rounds).  With a correction run_fedotplora_ranks exchanges the
    trained buffers first and every rank adds all participants in the round's order, so the sum has one order."""
    got, hist, corr = _both_drivers()
    pairs = (("flat", hist["global_weights"][KEY].reshape(-1)), ("c", corr.c), ("c_i", corr.c_i))
    for k, one in pairs:
        print(f"{k}: max |ranks - one process| = {float((got[0][k] - one).abs().max()):.3e}")
    for k, one in pairs:
        assert torch.equal(got[0][k], one), k


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
def _cli(*argv):
    from fairfedmed_amd import federated_main as M
    a = M.build_parser().parse_args(list(argv))
    a.idxs_users_train = [int(i) for i in a.idxs_users_train]
    a.idxs_users_test = [int(i) for i in a.idxs_users_test]
    return M.fed_args(a)


def test_flags_reach_fedargs():
    from fairfedmed_amd import federated as F
    a = _cli()
    assert (a.drift, a.mu) == ("none", 0.5) == (F.FedArgs(num_users=2).drift, F.FedArgs(num_users=2).mu)
    a = _cli("--drift", "fedprox", "--mu", "0.25")
    assert (a.drift, a.mu) == ("fedprox", 0.25)
    assert _cli("--drift", "fedprox").mu == 0.5                       # the reference's default
    assert _cli("--drift", "scaffold").drift == "scaffold"
    assert _cli("--model", "fedprox", "--mu", "0.5").drift == "none"  # the reference's baseline flag selects nothing here
    with pytest.raises(SystemExit):
        _cli("--drift", "feddyn")


def test_refusals_name_the_setting():
    from fairfedmed_amd import federated as F
    tr = _three_clients()
    assert F.drift_corrector(F.FedArgs(num_users=3), tr, 3) is None
    assert F.drift_corrector(F.FedArgs(num_users=3, drift="fedprox", dp_clip=1.0), tr, 3).cfg == D.DriftCfg("fedprox", 0.5)
    assert F.drift_corrector(F.FedArgs(num_users=3, drift="scaffold", compat_sequential_optimizer=True), tr, 3).cfg.mu == 0.0
    bare = NS(engine=NS(params=tr.engine.params))                     # an engine without set_drift
    for mode in ("fedprox", "scaffold"):
        with pytest.raises(ValueError, match="set_drift"):
            F.drift_corrector(F.FedArgs(num_users=3, drift=mode), bare, 3)
        with pytest.raises(ValueError, match="set_drift"):
            F.drift_corrector(F.FedArgs(num_users=3, drift=mode), NS(), 3)
        with pytest.raises(ValueError, match="idxs_users_train"):
            F.drift_corrector(F.FedArgs(num_users=3, drift=mode, idxs_users_train=[0, 2]), tr, 3)
    with pytest.raises(ValueError, match="dp_clip"):
        F.drift_corrector(F.FedArgs(num_users=3, drift="scaffold", dp_clip=1.0), tr, 3)
    with pytest.raises(ValueError, match="drift"):
        F.drift_corrector(F.FedArgs(num_users=3, drift="feddyn"), tr, 3)
    # the drivers refuse at set-up, before anything trains
    with pytest.raises(ValueError, match="idxs_users_train"):
        F.run_fedotplora(tr, _fed_args(drift="scaffold", idxs_users_train=[0]), log=lambda *_: None)
    assert not bool(tr.engine.params.flat.any())


def test_mu_without_drift_changes_nothing():
    from fairfedmed_amd import federated as F
    runs = []
    for kw in ({}, {"mu": 0.7}):
        tr = _three_clients()
        hist = F.run_fedotplora(tr, _fed_args(**kw), log=lambda *_: None)
        assert "drift" not in hist and tr.engine.last_drift is None
        runs.append(hist["global_weights"][KEY].clone())
    assert torch.equal(runs[0], runs[1])
    tr = _three_clients()
    prox = F.run_fedotplora(tr, _fed_args(drift="fedprox", mu=0.7), log=lambda *_: None)
    assert not torch.equal(prox["global_weights"][KEY], runs[0]) and len(prox["drift"]) == 3
