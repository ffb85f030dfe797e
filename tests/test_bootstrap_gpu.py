"""ffm_eval_boot_counts on the GPU: every comparison is exact integer equality of [B, G + 2, 10]
against tests/boot_ref.py's brute force, and against ops.eval_counts(method="pairs") on the gathered tensors - the all-pairs
kernel, which knows nothing of sorting, multiplicities or prefix sums.  Shapes are the smallest at which the kernels can
still go wrong: one sample, the block (256) and scan-tile (1024) edges, more replicates than one chunk."""
import numpy as np
import pytest
import torch

from tests import boot_ref as R

pytestmark = pytest.mark.gpu


def make(N, G, seed, unknown=0, beyond=0):
    """Scores with many exact ties; the first `unknown` attributes are -1, the next `beyond` are >= G."""
    rng = np.random.default_rng(seed)
    logits = np.round(rng.normal(size=(N, 2)) * 2, 1)
    prob = torch.softmax(torch.from_numpy(logits).float(), -1).numpy()
    y = rng.integers(0, 2, N)
    a = rng.integers(0, G, N)
    a[:unknown] = -1
    a[unknown:unknown + beyond] = G + 2
    return prob, y, a


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(prob, y, a, G, B, seed, tag=0, chunk=None):
    from fairfedmed_amd import ops
    return ops.eval_boot_counts(dev(prob), dev(y), dev(a), G, B, seed, tag=tag, chunk=chunk).cpu().numpy()


def check(prob, y, a, G, B, seed, tag=0, chunk=None):
    """The device tables == the brute force of every resampled set == the all-pairs kernel on the gathered tensors."""
    from fairfedmed_amd import ops
    got = run(prob, y, a, G, B, seed, tag, chunk)
    want = R.boot_counts(prob, y, a, G, B, seed, tag)
    assert got.shape == want.shape == (B, G + 2, 10) and got.dtype == np.int64
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    p_d, y_d, a_d = dev(prob), dev(y), dev(a)
    for r, idx in enumerate(R.draws(len(y), B, seed, tag)):
        i = torch.from_numpy(idx).cuda()
        pairs = ops.eval_counts(p_d[i].contiguous(), y_d[i].contiguous(), None if a_d is None else a_d[i].contiguous(), G,
                                method="pairs")
        assert np.array_equal(got[r], pairs.cpu().numpy()), r
    return got, want


@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1025])
def test_sizes_over_block_and_tile_edges(N):
    check(*make(N, 3, seed=N, unknown=min(N // 8, 5)), 3, 3, seed=11 + N, tag=2)


@pytest.mark.parametrize("with_attr", [True, False])
def test_many_replicates_unknown_and_out_of_range_attributes(with_attr):
    prob, y, a = make(97, 3, seed=97, unknown=4, beyond=3)
    got, _ = check(prob, y, a if with_attr else None, 3, 64, seed=(9 << 32) | 5, tag=1)
    if with_attr:
        assert got[:, 3, :2].sum() > 0                                  # the 'unknown' row holds the -1 and the >= G values
    else:
        assert not got[:, :3].any() and np.array_equal(got[:, 3], got[:, 4])


def test_all_scores_equal_every_pair_is_a_tie():
    prob, y, a = make(130, 2, seed=1)
    prob[:] = 0.5
    got, _ = check(prob, y, a, 2, 4, seed=3)
    assert not got[:, :, [2, 4]].any() and np.array_equal(got[:, -1, 3], got[:, -1, 0] * got[:, -1, 1])


def test_all_labels_positive_no_negatives():
    prob, y, a = make(130, 2, seed=2)
    y[:] = 1
    got, _ = check(prob, y, a, 2, 4, seed=3)
    assert not got[:, :, 1:6].any() and (got[:, -1, 0] == 130).all()


def test_all_samples_in_one_group():
    prob, y, a = make(300, 3, seed=3)
    a[:] = 1
    got, _ = check(prob, y, a, 3, 4, seed=3)
    assert np.array_equal(got[:, 1], got[:, -1]) and not got[:, [0, 2, 3]].any()


def test_a_group_that_is_present_and_never_drawn():
    prob, y, _ = make(4, 4, seed=4)
    a = np.arange(4)
    got, want = check(prob, y, a, 4, 8, seed=21, tag=5)
    empty = (want[:, :4, :2].sum(-1) == 0).any(1)                       # some replicate misses one of the four samples
    assert empty.any()
    assert np.array_equal((got[:, :4, :2].sum(-1) == 0).any(1), empty)


def test_chunking_changes_nothing():
    prob, y, a = make(257, 3, seed=8, unknown=3)
    got = [torch.from_numpy(run(prob, y, a, 3, 5, seed=77, tag=1, chunk=c)) for c in (1, 2, 5, 8, None)]
    assert all(torch.equal(got[0], g) for g in got[1:])
    assert np.array_equal(got[0].numpy(), R.boot_counts(prob, y, a, 3, 5, 77, 1))


def test_draws_depend_on_seed_and_tag_and_on_nothing_else():
    prob, y, a = make(97, 3, seed=97, unknown=4, beyond=3)
    base = run(prob, y, a, 3, 6, seed=5, tag=1)
    assert not np.array_equal(base, run(prob, y, a, 3, 6, seed=5, tag=2))
    assert not np.array_equal(base, run(prob, y, a, 3, 6, seed=6, tag=1))
    assert not np.array_equal(base, run(prob, y, a, 3, 6, seed=5 | (1 << 32), tag=1))      # the high word is part of the key
    rng = np.random.default_rng(0)
    for G, other in ((3, rng.integers(0, 3, 97)), (8, rng.integers(0, 8, 97)), (2, a), (3, None)):
        assert np.array_equal(base[:, -1], run(prob, y, other, G, 6, seed=5, tag=1)[:, -1])
    # replicate r does not depend on how many replicates are asked for
    assert np.array_equal(base[:4], run(prob, y, a, 3, 4, seed=5, tag=1))


def test_two_calls_give_identical_tables():
    prob, y, a = make(1025, 3, seed=12)
    assert np.array_equal(run(prob, y, a, 3, 7, seed=1, chunk=3), run(prob, y, a, 3, 7, seed=1, chunk=3))


def test_no_side_effects_and_no_recording():
    from fairfedmed_amd import ops
    prob, y, a = make(300, 3, seed=13, unknown=2)
    p_d, y_d, a_d = dev(prob), dev(y), dev(a)
    before = ops.eval_counts(p_d, y_d, a_d, 3).clone()
    keep = [t.clone() for t in (p_d, y_d, a_d)]
    ops.eval_boot_counts(p_d, y_d, a_d, 3, 4, 9)
    assert all(torch.equal(t, k) for t, k in zip((p_d, y_d, a_d), keep))
    assert torch.equal(ops.eval_counts(p_d, y_d, a_d, 3), before)
    assert torch.equal(ops.eval_counts(p_d, y_d, a_d, 3, method="sort"), before)
    plan = []
    with ops.record(plan):
        with pytest.raises(RuntimeError, match="recorded"):
            ops.eval_boot_counts(p_d, y_d, a_d, 3, 4, 9)
    assert plan == []
    with pytest.raises(ValueError):
        ops.eval_boot_counts(p_d, y_d, a_d, 3, 0, 9)
    with pytest.raises(ValueError):
        ops.eval_boot_counts(p_d, y_d, a_d, 3, 4, 9, chunk=0)


def test_default_chunk_stays_under_the_budget():
    from fairfedmed_amd import _lib, ops
    lib = _lib.load()
    assert ops.eval_boot_chunk(2048, 1000) == 1000
    c = ops.eval_boot_chunk(200000, 1000)
    assert 1 <= c < 1000 and lib.ffm_eval_boot_ws_bytes(200000, c) <= ops.EVAL_BOOT_WS_BUDGET
    assert lib.ffm_eval_boot_ws_bytes(200000, c + 1) > ops.EVAL_BOOT_WS_BUDGET


def test_the_size_at_which_the_evaluator_itself_sorts():
    """40 000 samples: the 'all' row of each replicate against eval_counts(method="sort") on the gathered tensors."""
    from fairfedmed_amd import ops
    N = 40000
    prob, y, a = make(N, 3, seed=40, unknown=9)
    p_d, y_d, a_d = dev(prob), dev(y), dev(a)
    got = ops.eval_boot_counts(p_d, y_d, a_d, 3, 2, 31, tag=4)
    for r in range(2):
        i = torch.from_numpy(R.draw(N, 31, 4, r)).cuda()
        want = ops.eval_counts(p_d[i].contiguous(), y_d[i].contiguous(), a_d[i].contiguous(), 3, method="sort")
        assert torch.equal(got[r, -1], want[-1])
        assert torch.equal(got[r], want)                                # and the group rows with it


def _same(a, b, path="ci"):
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), path
        for j, (x, z) in enumerate(zip(a, b)):
            _same(x, z, f"{path}[{j}]")
    elif a is None or b is None:
        assert a is None and b is None, path
    else:
        assert abs(a - b) <= 1e-12, (path, a, b)


def test_trainer_test_adds_the_intervals_and_changes_nothing_else(monkeypatch):
    from tests.test_trainer_gpu import make_cfg
    from fairfedmed_amd import config as C
    from fairfedmed_amd import metrics as M
    from fairfedmed_amd import ops
    from fairfedmed_amd.trainer import GLP_OT_SVLoRA, SyntheticFedData
    mcfg = C.vit_tiny(rank=4)
    cfg = make_cfg(prec="fp32")
    cfg.TEST.NO_TEST = False
    data = SyntheticFedData(mcfg, num_clients=1, train_batches=2, test_batches=30, batch_size=8, signal=0.4)
    tr = GLP_OT_SVLoRA(cfg, data=data)
    tr.fed_before_train()
    tr.train(idx=0, global_epoch=0, is_fed=True)
    plain = tr.test(idx=0)
    plain_full = dict(tr.last_results)
    assert "ci" not in plain_full
    seen = []
    real = ops.eval_boot_counts

    def spy(prob, label, attr, G, B, seed, tag=0, **kw):
        seen.append((prob.cpu().numpy(), label.cpu().numpy(), attr.cpu().numpy(), G, B, seed, tag))
        return real(prob, label, attr, G, B, seed, tag=tag, **kw)

    monkeypatch.setattr(ops, "eval_boot_counts", spy)
    cfg.TEST.BOOTSTRAP, cfg.TEST.BOOTSTRAP_SEED, cfg.TEST.CI_LEVEL = 50, 17, 0.9
    boot = tr.test(idx=0)
    full = dict(tr.last_results)
    assert boot == plain
    ci = full.pop("ci")
    assert sorted(full) == sorted(plain_full)
    for k, v in plain_full.items():
        if isinstance(v, list):
            assert len(v) == len(full[k]) and all(np.array_equal(x, z) for x, z in zip(v, full[k])), k
        else:
            assert v == full[k], k
    assert len(seen) >= 1 and all(s[3:] == (8, 50, 17, 1) for s in seen)          # tag = client index + 1
    assert len(seen[0][1]) == 240
    tables = np.stack([R.counts(p, y, a, 8) for p, y, a, *_ in seen])
    reps = np.stack([R.boot_counts(p, y, a, 8, 50, 17, 1) for p, y, a, *_ in seen])
    _same(ci, M.bootstrap_intervals(tables, reps, level=0.9))
    assert ci["level"] == 0.9 and ci["replicates"] == 50 and len(ci["degenerate"]) == len(seen)


def test_driver_keeps_one_entry_per_client_and_round():
    from tests.test_trainer_gpu import _fed_setup
    from fairfedmed_amd import federated as F
    tr = _fed_setup(users=2)
    tr.cfg.TEST.BOOTSTRAP = 20
    lines = []
    hist = F.run_fedotplora(tr, F.FedArgs(num_users=2, frac=1.0, round=1, seed=0), log=lambda *a: lines.append(" ".join(map(str, a))))
    assert len(hist["ci"]) == 1 and sorted(hist["ci"][0]) == [0, 1]
    for c in (0, 1):
        assert hist["ci"][0][c]["replicates"] == 20
        assert sum(f"client {c}:" in l and "bootstrap" in l for l in lines) == 1
    tr.cfg.TEST.BOOTSTRAP = 0
    assert "ci" not in F.run_fedotplora(tr, F.FedArgs(num_users=2, frac=1.0, round=1, seed=0), log=lambda *_: None)
