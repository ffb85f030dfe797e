"""tests/ot_reference.py (the float64 restatement the OT head kernels are tested against) against the oracle's own
plans, oracle.fairlora_oracle.sinkhorn_plan / cot_plan, and the oracle's similarity layout."""
import pytest
import torch
import torch.nn.functional as F

from oracle import fairlora_oracle as O
from tests import ot_reference as R


def _problem(B, L, D, N, n_cls, eps, seed):
    f, tn = R.clip_like_inputs(B, L, D, N, n_cls, seed)
    sim, _ = R.similarities(f, tn, n_cls, N)
    P, M, _ = sim.shape
    K = torch.exp(-(1.0 - sim) / eps)
    return K, torch.full((P, M), 1.0 / M, dtype=torch.float64), torch.full((P, N), 1.0 / N, dtype=torch.float64)


def _oracle(mode, K, a, b, thresh, max_iter):
    return O.sinkhorn_plan(K, a, b, thresh, max_iter) if mode == "Sinkhorn" else O.cot_plan(a, b, K, thresh, max_iter)


def _rel(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("mode,top", [("Sinkhorn", 1.0), ("COT", 1.0), ("COT", 0.8)])
@pytest.mark.parametrize("stop", ["early", "max_iter"])
def test_restatement_matches_the_oracle_plans(mode, top, stop):
    """Same T to 1e-12 in float64 and the same number of iterations: the oracle run with exactly istop + 1 iterations
    (thresh 0) reproduces its stopped plan bit for bit, and with istop iterations it does not."""
    K, a, b = _problem(3, 50, 64, 2, 2, 0.1, seed=11)
    b = b * min(float(K.shape[0]), top)
    max_iter = 12
    probe = R.iterate(K, a, b, mode, 0.0, max_iter)
    assert probe.istop == max_iter - 1
    # early: the first iteration k >= 1 whose mean is below every earlier one (COT's means need not fall monotonically),
    # with the threshold halfway (geometrically) between it and the smallest earlier mean -> istop = k
    expect, thresh = max_iter - 1, 0.0
    if stop == "early":
        expect = next(k for k in range(2, max_iter - 1) if probe.means[k] < min(probe.means[:k]))
        thresh = (probe.means[expect] * min(probe.means[:expect])) ** 0.5
    r = R.iterate(K, a, b, mode, thresh, max_iter)
    assert r.istop == expect
    assert len(r.means) == r.istop + 1 and r.errs.shape == (r.istop + 1, K.shape[0])
    ref = _oracle(mode, K, a, b, thresh, max_iter)
    assert _rel(r.T, ref) <= 1e-12
    assert torch.equal(_oracle(mode, K, a, b, 0.0, r.istop + 1), ref)
    assert not torch.equal(_oracle(mode, K, a, b, 0.0, r.istop), ref)
    # the per-problem sums are what the means average: Sinkhorn over the M tokens, COT over the N prompts
    width = K.shape[1] if mode == "Sinkhorn" else K.shape[2]
    torch.testing.assert_close(r.errs.sum(1) / (K.shape[0] * width), torch.tensor(r.means, dtype=torch.float64),
                               rtol=1e-13, atol=0)


@pytest.mark.parametrize("mode", ["Sinkhorn", "COT"])
def test_restatement_head_matches_the_oracle_logits(mode):
    """The whole forward head (similarities, plan, logits) against oracle.clip_logits's head arithmetic."""
    B, L, D, N, n_cls, eps, ls = 2, 9, 16, 3, 2, 0.1, 2.5
    f, tn = R.clip_like_inputs(B, L, D, N, n_cls, seed=5)
    r = R.head(f, tn, ls, n_cls, N, mode, eps, 1e-3, 100, top=0.8)
    feats = F.normalize(f[:, 1:].permute(1, 0, 2), dim=2)
    sim = torch.einsum("mbd,ncd->mnbc", feats, tn.view(N, n_cls, D)).contiguous().view(L - 1, N, -1).permute(2, 0, 1)
    K = torch.exp(-(1.0 - sim) / eps)
    xx = torch.full((B * n_cls, L - 1), 1.0 / (L - 1), dtype=torch.float64)
    yy = torch.full((B * n_cls, N), 1.0 / N, dtype=torch.float64)
    if mode == "COT":
        yy = yy * min(float(torch.sum(xx)), 0.8)
    T = _oracle(mode, K, xx, yy, 1e-3, 100)
    logits = torch.exp(torch.tensor(ls, dtype=torch.float64)) * torch.sum(T * sim, dim=(1, 2))
    assert _rel(r.T, T) <= 1e-12 and _rel(r.logits, logits) <= 1e-12


def test_similarity_layout_matches_the_oracle():
    """sim[(b * n_cls + c), m, n] = <f^[b, 1 + m], tn[n * n_cls + c]> is the oracle's einsum("mbd,ncd->mnbc") / view /
    permute on a case with every dimension distinct."""
    B, L, D, N, n_cls = 2, 5, 8, 3, 4
    g = torch.Generator().manual_seed(3)
    f = torch.randn(B, L, D, generator=g, dtype=torch.float64) * 3
    tn = F.normalize(torch.randn(N * n_cls, D, generator=g, dtype=torch.float64), dim=1)
    sim, rnorm = R.similarities(f, tn, n_cls, N)
    feats = F.normalize(f[:, 1:].permute(1, 0, 2), dim=2)                     # [M, B, D], class token dropped
    ref = torch.einsum("mbd,ncd->mnbc", feats, tn.view(N, n_cls, D)).contiguous()
    ref = ref.view(L - 1, N, -1).permute(2, 0, 1)
    assert sim.shape == ref.shape == (B * n_cls, L - 1, N)
    torch.testing.assert_close(sim, ref, rtol=0, atol=1e-14)
    for b, c, m, n in [(0, 0, 0, 0), (1, 3, 3, 2), (1, 2, 0, 1), (0, 1, 2, 2)]:
        direct = float(F.normalize(f[b, 1 + m], dim=0) @ tn[n * n_cls + c])
        assert abs(float(sim[b * n_cls + c, m, n]) - direct) <= 1e-14
    assert torch.all(rnorm[:, 0] == 0)
    torch.testing.assert_close(rnorm[:, 1:], 1 / f[:, 1:].norm(dim=-1), rtol=1e-15, atol=0)


def test_backward_restatement_matches_autograd_through_the_oracle_head():
    """The per-image text partials sum to the gradient of the shared tn, and df matches autograd through
    F.normalize / einsum with T held constant."""
    B, L, D, N, n_cls, ls = 3, 6, 8, 2, 2, 2.0
    f, tn = R.clip_like_inputs(B, L, D, N, n_cls, seed=8)
    g = torch.Generator().manual_seed(1)
    T = torch.rand(B * n_cls, L - 1, N, generator=g, dtype=torch.float64)
    dl = torch.randn(B * n_cls, generator=g, dtype=torch.float64)
    df, dtn_part = R.backward(f, tn, ls, T, dl, n_cls, N)
    fx, tx = f.clone().requires_grad_(True), tn.clone().requires_grad_(True)
    feats = F.normalize(fx[:, 1:].permute(1, 0, 2), dim=2)
    sim = torch.einsum("mbd,ncd->mnbc", feats, tx.view(N, n_cls, D)).contiguous().view(L - 1, N, -1).permute(2, 0, 1)
    (dl * torch.exp(torch.tensor(ls, dtype=torch.float64)) * (T * sim).sum(dim=(1, 2))).sum().backward()
    torch.testing.assert_close(df, fx.grad, rtol=1e-12, atol=1e-15)
    assert torch.all(df[:, 0] == 0)
    torch.testing.assert_close(dtn_part.sum(0), tx.grad, rtol=1e-12, atol=1e-15)
