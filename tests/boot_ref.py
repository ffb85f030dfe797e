"""Reference of the bootstrap evaluator (ffm_eval_boot_counts), written from its definition in include/ffm_hip.h: the
draws in Python integers on top of tests/dp_ref.py's Philox, and the count table of a resampled set by brute force.

    replicate r, draw k:  x = Philox4x32-10(counter (k >> 1, r, tag, 0x544F4F42), key (seed low, seed high))
                          x64 = x[2 (k & 1)] | x[2 (k & 1) + 1] << 32        idx_k = (x64 * N) >> 64
"""
import numpy as np

from tests import dp_ref

BOOT_WORD = 0x544F4F42


def draw(N, seed, tag, r):
    """idx_0 .. idx_{N-1} of replicate r (int64 array)."""
    w = dp_ref.words(4 * ((N + 1) // 2), seed, 0, r, tag, BOOT_WORD)
    return np.array([((int(w[2 * k]) | (int(w[2 * k + 1]) << 32)) * N) >> 64 for k in range(N)], dtype=np.int64)


def draws(N, B, seed, tag):
    """[B, N]."""
    return np.stack([draw(N, seed, tag, r) for r in range(B)])


def counts(prob, y, attr, G):
    """The table ffm_eval_counts produces (include/ffm_hip.h), by brute force: rows groups 0..G-1, unknown, all; columns
    n_pos n_neg win1 tie1 win0 tie0 TP FP TN FN.  attr None: every sample is 'unknown'."""
    prob, y = np.asarray(prob), np.asarray(y)
    attr = np.full(len(y), -1) if attr is None else np.asarray(attr)
    t = np.zeros((G + 2, 10), dtype=np.int64)
    slot = np.where((attr >= 0) & (attr < G), attr, G)
    pred = prob[:, 1] > prob[:, 0]
    for row, sel in [(g, slot == g) for g in range(G + 1)] + [(G + 1, np.ones(len(y), bool))]:
        p, yy, pr = prob[sel], y[sel], pred[sel]
        pos, neg = p[yy == 1], p[yy != 1]
        t[row, 0], t[row, 1] = len(pos), len(neg)
        t[row, 2] = (pos[:, None, 1] > neg[None, :, 1]).sum()
        t[row, 3] = (pos[:, None, 1] == neg[None, :, 1]).sum()
        t[row, 4] = (neg[None, :, 0] > pos[:, None, 0]).sum()
        t[row, 5] = (neg[None, :, 0] == pos[:, None, 0]).sum()
        t[row, 6], t[row, 7] = (pr & (yy == 1)).sum(), (pr & (yy != 1)).sum()
        t[row, 8], t[row, 9] = (~pr & (yy != 1)).sum(), (~pr & (yy == 1)).sum()
    return t


def boot_counts(prob, y, attr, G, B, seed, tag):
    """[B, G + 2, 10]: counts() of every resampled set (labels in {0, 1})."""
    prob, y = np.asarray(prob), np.asarray(y)
    out = []
    for idx in draws(len(y), B, seed, tag):
        out.append(counts(prob[idx], y[idx], None if attr is None else np.asarray(attr)[idx], G))
    return np.stack(out)
