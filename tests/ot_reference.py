"""A float64 restatement of the Sinkhorn / COT logits head (csrc/head_ot.hip), in the layouts the kernels use.

Not a test module: tests/test_ot_reference_cpu.py holds it to oracle.fairlora_oracle.sinkhorn_plan / cot_plan, and
tests/test_ot_head_gpu.py holds the kernels to it.

  sim[(b * n_cls + c), m, n] = <f^[b, 1 + m], tn[n * n_cls + c]>        f^ = f / max(|f|, 1e-12), class token dropped
  K = exp(-(1 - sim) / eps); T = diag(x) K diag(y) after the scaling iterations (x, y) = (r, c) Sinkhorn, (u, v) COT
  logits[b * n_cls + c] = exp(logit_scale) * sum_{m, n} T * sim

The whole batch stops at one iteration: the first whose batch mean of the change (Sinkhorn mean|r - r0|, COT
mean|v - v0|) is below `thresh`, else max_iter - 1 - the index the kernels report as `istop`.  `iters` runs a fixed
number of iterations instead (no stopping test), so that the same restatement run in float32 gives the rounding error
of float32 arithmetic at the float64 run's iteration count.
"""
import math
from types import SimpleNamespace

import torch


def similarities(f, tn, n_cls, N, dtype=torch.float64):
    """f [B, L, D] token features (row 0 = class token), tn [N * n_cls, D] or per image [B, N * n_cls, D].
    Returns sim [B * n_cls, L - 1, N] and rnorm [B, L] (class-token entries 0)."""
    B, L, D = f.shape
    x = f[:, 1:].to(dtype)
    rn = 1.0 / x.norm(dim=-1).clamp_min(1e-12)
    fh = x * rn[..., None]
    if tn.dim() == 2:
        sim = torch.einsum("bmd,ncd->bcmn", fh, tn.to(dtype).view(N, n_cls, D))
    else:
        sim = torch.einsum("bmd,bncd->bcmn", fh, tn.to(dtype).view(B, N, n_cls, D))
    rnorm = torch.cat([torch.zeros(B, 1, dtype=dtype), rn.detach()], dim=1)
    return sim.reshape(B * n_cls, L - 1, N), rnorm


def iterate(K, a, b, mode, thresh, max_iter, iters=None):
    """The scaling iterations on K [P, M, N] with marginals a [P, M], b [P, N] (oracle.sinkhorn_plan(K, a, b, ...) /
    oracle.cot_plan(a, b, K, ...)).  Returns T, the batch means and per-problem sums of the change, the max |iterate|
    after every iteration, the stop index and the final iterates."""
    assert mode in ("Sinkhorn", "COT")
    n = max_iter if iters is None else iters
    Kt = K.transpose(1, 2)
    ones_a, ones_b = torch.ones_like(a), torch.ones_like(b)
    x, y = ones_a, ones_b
    if mode == "COT":
        Kp, Kq = K * (1 / a)[..., None], Kt * (1 / b)[..., None]
    means, errs, itmax, istop = [], [], [], n - 1
    for it in range(n):
        if mode == "Sinkhorn":
            x0 = x
            x = a / (K @ y[..., None])[..., 0]                       # r = u / (K c)
            y = b / (Kt @ x[..., None])[..., 0]                      # c = v / (K^T r)
            d, cur = (x - x0).abs(), x
        else:
            y0 = y
            x = torch.minimum(ones_a / (Kp @ y[..., None])[..., 0], ones_a)   # u = min(dx / (Kp v), dx)
            y = ones_b / (Kq @ x[..., None])[..., 0]                          # v = dy / (Kq u)
            d, cur = (y - y0).abs(), y
        errs.append(d.sum(1))
        means.append(float(d.mean()))
        itmax.append(float(cur.abs().max()))
        if iters is None and means[-1] < thresh:
            istop = it
            break
    T = x[:, :, None] * K * y[:, None, :]
    return SimpleNamespace(T=T, means=means, errs=torch.stack(errs), itmax=itmax, istop=istop, x=x, y=y)


def head(f, tn, logit_scale, n_cls, N, mode, eps, thresh, max_iter, top=1.0, iters=None, dtype=torch.float64):
    """The forward head of ffm_ot_head_fwd on f [B, L, D], tn [N * n_cls, D], everything computed in `dtype`."""
    sim, rnorm = similarities(f, tn, n_cls, N, dtype)
    P, M, _ = sim.shape
    K = torch.exp(-(1.0 - sim) / eps)
    a = torch.full((P, M), 1.0 / M, dtype=dtype)
    b = torch.full((P, N), 1.0 / N, dtype=dtype)
    if mode == "COT":
        b = b * min(float(P), top)                                   # top_percent = min(sum(xx) = #problems, TOP_PERCENT)
    r = iterate(K, a, b, mode, thresh, max_iter, iters)
    r.sim, r.rnorm, r.K = sim, rnorm, K
    r.tsum = (r.T * sim).sum(dim=(1, 2))
    r.logits = torch.exp(torch.tensor(logit_scale, dtype=dtype)) * r.tsum
    return r


def backward(f, tn, logit_scale, T, dlogits, n_cls, N, dtype=torch.float64):
    """Gradients of sum(dlogits * exp(ls) * sum T * sim(f, tn)) with T held constant: df [B, L, D] (class-token rows 0)
    and the per-image partials dtn_part [B, N * n_cls, D] (ffm_ot_head_bwd's layout), computed in `dtype`."""
    B, L, D = f.shape
    fx = f.to(dtype).clone().requires_grad_(True)
    tx = tn.to(dtype).reshape(1, N * n_cls, D).repeat(B, 1, 1).requires_grad_(True)
    sim, _ = similarities(fx, tx, n_cls, N, dtype)
    es = torch.exp(torch.tensor(logit_scale, dtype=dtype))
    logits = es * (T.to(dtype).view_as(sim) * sim).sum(dim=(1, 2))
    (logits * dlogits.to(dtype).flatten()).sum().backward()
    return fx.grad.detach(), tx.grad.detach()


def clip_like_inputs(B, L, D, N, n_cls, seed):
    """Float64 features shaped like CLIP's: random directions plus a shared component along the mean text direction, so
    that sim lies roughly in [0, 0.3] (a few tokens up to 0.5); rows left unnormalised with norms in about [0.5, 20];
    tn rows of unit length.

    Token mix: about 90 % background tokens - one direction per image plus 2 % noise, as the large uniform regions of
    fundus / OCT images give - and 10 % foreground tokens, each its own random direction with a small component along
    the prompt directions.  Both the mix and the interaction matter for the stopping tests: COT's clamp u <= 1 is
    active at these similarities, and near its fixed point the change falls by about the clamped fraction per iteration
    (slowly when the clamped tokens are all different); Sinkhorn on a nearly rank-one K converges within two iterations
    to rounding noise.  With this mix both still change clearly at iteration 2 and fall by 2-5x per iteration."""
    g = torch.Generator().manual_seed(seed)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    mu = unit(randn(D))
    h = unit(randn(N * n_cls, D))
    tn = unit(0.8 * mu + 0.6 * h)
    w = 0.45 * rand(B, L, 1)
    fg = unit(w * mu + 0.1 * randn(B, L, N * n_cls) @ h + unit(randn(B, L, D)))
    bg = unit(0.2 * mu + unit(randn(B, 1, D)))
    bg = unit(bg + 0.02 * unit(randn(B, L, D)))
    is_bg = (rand(B, L, 1) >= 0.1).double()
    f = is_bg * bg + (1 - is_bg) * fg
    norms = torch.exp(math.log(0.5) + math.log(40.0) * rand(B, L, 1))
    return f * norms, tn
