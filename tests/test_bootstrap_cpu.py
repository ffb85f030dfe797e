"""Bootstrap confidence intervals, the parts that need no GPU: the two entry points and their
argument validation, metrics.bootstrap_intervals against numpy percentiles of the host scores on the gathered arrays, the
degenerate-replicate rule, the trainer's refusals and the command line."""
import logging
from types import SimpleNamespace as NS

import numpy as np
import pytest

from tests import boot_ref as R

N, B, SEED, TAG = 600, 200, 1234, 1


def _fixture():
    """600 samples, three groups of 200, labels Bernoulli(0.45), scores on a 1/64 grid so that ties abound."""
    rng = np.random.default_rng(0)
    y = (rng.random(N) < 0.45).astype(np.int64)
    z = rng.normal(size=N)
    p1 = np.round(np.clip(0.5 + 0.2 * (y - 0.5) + 0.25 * z, 0.01, 0.99) * 64) / 64
    prob = np.stack([1 - p1, p1], 1).astype(np.float32)
    return prob, y, np.repeat([0, 1, 2], 200)


@pytest.fixture(scope="module")
def boot():
    """(prob, y, attrs [2, N], draws [B, N], full tables, replicate tables) - computed once, read-only."""
    prob, y, a = _fixture()
    b = np.where(np.arange(N) % 12 == 0, -1, np.arange(N) % 2)       # two groups and 50 'unknown' samples
    attrs = np.stack([a, b])
    idx = R.draws(N, B, SEED, TAG)
    full = np.stack([R.counts(prob, y, at, 3) for at in attrs])
    rep = np.stack([np.stack([R.counts(prob[i], y[i], at[i], 3) for i in idx]) for at in attrs])
    for arr in (prob, y, attrs, idx, full, rep):
        arr.setflags(write=False)
    return prob, y, attrs, idx, full, rep


def _close(got, want):
    assert got is not None and len(got) == len(want) == 3
    assert np.allclose(got, want, rtol=0, atol=1e-12), (got, want)


def _triple(v, level=0.95):
    v = np.asarray(v, dtype=np.float64)
    return (np.percentile(v, 100 * (1 - level) / 2), np.percentile(v, 100 * (1 + level) / 2), np.std(v, ddof=1))


def test_exports_and_argument_validation_without_a_gpu():
    from fairfedmed_amd import _lib
    from fairfedmed_amd import build as Bd
    lib = _lib.load()
    assert lib.ffm_abi_version() == 14                                  # additive: the version stays
    assert "evalboot.hip" in Bd.SOURCES and "evalboot.hip" not in Bd.TWIN_SOURCES
    for name in ("ffm_eval_boot_ws_bytes", "ffm_eval_boot_counts"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ffm_eval_boot_ws_bytes(0, 4) == -1 and lib.ffm_eval_boot_ws_bytes(16, 0) == -1
    p, big = 256, 1 << 40                                               # a non-null, 256-byte aligned address; never read

    def call(prob=p, label=p, attr=None, n=16, g=3, b=5, chunk=2, out=p, ws=p, nbytes=big):
        return lib.ffm_eval_boot_counts(prob, label, attr, n, g, b, chunk, 7, 1, out, ws, nbytes, None)

    assert call(prob=None) == -1 and call(label=None) == -1 and call(out=None) == -1 and call(ws=None) == -1
    assert call(n=0) == -1 and call(n=-3) == -1 and call(b=0) == -1 and call(chunk=0) == -1 and call(chunk=-1) == -1
    assert call(g=9) == -1 and call(g=-1) == -1                         # FFM_MAX_GROUPS = 8
    assert call(ws=p + 8) == -1                                         # misaligned workspace
    assert call(nbytes=64) == -1 and call(nbytes=0) == -1               # short workspace


def test_intervals_equal_numpy_percentiles_of_the_host_scores(boot):
    from fairfedmed_amd import metrics as M
    prob, y, attrs, idx, full, rep = boot
    assert abs(M.auc_macro_ovr(prob, y) - 0.7224) < 5e-5
    ci = M.bootstrap_intervals(full, rep)
    assert ci["level"] == 0.95 and ci["replicates"] == B
    assert ci["degenerate"] == [0, 0]
    # the host route: every score recomputed from the gathered arrays
    acc, f1, auc, comp = [], [], [], []
    for i in idx:
        p, yy = prob[i], y[i]
        pred = p.argmax(-1)
        acc.append(100.0 * float((pred == yy).mean()))
        f1.append(100.0 * M.macro_f1(pred, yy, 2))
        auc.append(100.0 * M.auc_macro_ovr(p, yy))
        comp.append(M.comprehensive_scores(p, yy, attrs[:, i]))
    _close(ci["accuracy"], _triple(acc))
    _close(ci["macro_f1"], _triple(f1))
    _close(ci["auc"], _triple(auc))
    assert 68.0 < ci["auc"][0] < 68.2 and 76.6 < ci["auc"][1] < 76.8
    for a in range(2):
        ga = np.array([c["aucs_by_attrs"][a] for c in comp])
        assert ga.shape == (B, 3 if a == 0 else 2) and len(ci["aucs_by_attrs"][a]) == ga.shape[1]
        for g in range(ga.shape[1]):
            _close(ci["aucs_by_attrs"][a][g], _triple(ga[:, g]))
        _close(ci["auc_gap_by_attrs"][a], _triple(ga.max(1) - ga.min(1)))
        for k in ("esaucs_by_attrs", "dpds", "eods"):
            _close(ci[k][a], _triple([c[k][a] for c in comp]))
    # another level: narrower, from the same replicates
    ci80 = M.bootstrap_intervals(full, rep, level=0.8)
    _close(ci80["auc"], _triple(auc, 0.8))
    assert ci["auc"][0] < ci80["auc"][0] < ci80["auc"][1] < ci["auc"][1] and ci80["auc"][2] == ci["auc"][2]


def test_a_group_of_three_samples_gets_no_interval(boot, caplog):
    """87 of the 200 resamples leave the three-sample group empty or with one class: over the cap, so no interval is
    formed from the thinned set - None, a warning, and the count."""
    from fairfedmed_amd import metrics as M
    prob, y, attrs, idx, full, rep = boot
    small = attrs[0].copy()
    small[:3] = 3                                                       # groups of 197, 200, 200 and 3
    full4 = np.stack([R.counts(prob, y, a, 4) for a in (attrs[0], small)])
    rep4 = np.stack([np.stack([R.counts(prob[i], y[i], a[i], 4) for i in idx]) for a in (attrs[0], small)])
    want = sum(1 for i in idx if len(set(y[i][small[i] == 3])) < 2)     # the reference's count, from the gathered labels
    assert want == 87
    with caplog.at_level(logging.WARNING, logger="fairfedmed_amd.metrics"):
        ci = M.bootstrap_intervals(full4, rep4)
    assert ci["degenerate"] == [0, want]
    assert any("degenerate" in r.getMessage() for r in caplog.records)
    for k in ("aucs_by_attrs", "esaucs_by_attrs", "auc_gap_by_attrs", "dpds", "eods"):
        assert ci[k][1] is None and ci[k][0] is not None
    assert ci["auc"] is not None                                        # the 'all' row has both classes in every replicate
    # under a cap that admits them the interval is formed from the 113 others, and says so
    loose = M.bootstrap_intervals(full4, rep4, max_degenerate=0.5)
    assert loose["degenerate"] == [0, want] and loose["esaucs_by_attrs"][1] is not None
    keep = [r for r, i in enumerate(idx) if len(set(y[i][small[i] == 3])) == 2]
    es = [M.comprehensive_scores(prob[idx[r]], y[idx[r]], small[idx[r]][None])["esaucs_by_attrs"][0] for r in keep]
    _close(loose["esaucs_by_attrs"][1], _triple(es))


def test_bootstrap_intervals_rejects_mismatched_tables(boot):
    from fairfedmed_amd import metrics as M
    _, _, _, _, full, rep = boot
    with pytest.raises(ValueError):
        M.bootstrap_intervals(full[:1], rep)
    with pytest.raises(ValueError):
        M.bootstrap_intervals(full, rep, level=1.0)


def test_trainer_refuses_host_metrics_and_three_classes():
    """TEST.BOOTSTRAP > 0 is never ignored: test() raises before anything runs."""
    from fairfedmed_amd.trainer import GLP_OT_SVLoRA

    def fail(*a, **k):
        raise AssertionError("test() went on past the refusal")

    for classes, host in ((2, True), (3, False)):
        me = NS(cfg=NS(TEST=NS(BOOTSTRAP=10, HOST_METRICS=host)), num_classes=classes, set_model_mode=fail)
        with pytest.raises(NotImplementedError, match="BOOTSTRAP"):
            GLP_OT_SVLoRA.test(me, idx=0)
    me = NS(cfg=NS(TEST=NS(BOOTSTRAP=0, HOST_METRICS=True)), num_classes=3, set_model_mode=fail)
    with pytest.raises(AssertionError, match="went on"):               # off: nothing is refused
        GLP_OT_SVLoRA.test(me, idx=0)


def test_flags_reach_the_configuration():
    from fairfedmed_amd import federated_main as M
    base = ["--num_users", "2", "--unfreeze_image_encoder", "1"]
    cfg = M.setup_cfg(M.build_parser().parse_args(base + ["--bootstrap", "500", "--bootstrap_seed", "9", "--ci_level", "0.9"]))
    assert (cfg.TEST.BOOTSTRAP, cfg.TEST.BOOTSTRAP_SEED, cfg.TEST.CI_LEVEL) == (500, 9, 0.9)
    cfg = M.setup_cfg(M.build_parser().parse_args(base))
    assert (cfg.TEST.BOOTSTRAP, cfg.TEST.BOOTSTRAP_SEED, cfg.TEST.CI_LEVEL) == (0, 0, 0.95)


def test_draws_follow_the_definition():
    """boot_ref.draw against the definition spelled out with dp_ref.philox_one, draw by draw."""
    from tests import dp_ref
    n, seed, tag, r = 11, (5 << 32) | 77, 3, 2
    got = R.draw(n, seed, tag, r)
    for k in range(n):
        x = dp_ref.philox_one((k >> 1, r, tag, 0x544F4F42), dp_ref.key_of(seed))
        x64 = x[2 * (k & 1)] | (x[2 * (k & 1) + 1] << 32)
        assert got[k] == (x64 * n) >> 64
    assert got.min() >= 0 and got.max() < n
