"""References for the fairness term of the loss (ffm_ce_fair_loss; include/ffm_hip.h has the formulas), shared by
tests/test_fairness_loss_cpu.py and tests/test_fairness_loss_gpu.py.  Everything here is float64 torch on the CPU.

`autograd_ref` is the loss of trainers/GLP_OT_SVLoRA.py:908-948 with the term NOT detached (torch.stack where the reference
has torch.tensor); `closed_form` restates the header's formulas without autograd.  Groups are the g in [0, G) present in
the batch; a sample outside [0, G) takes part in the cross-entropy only.
"""
import torch

# (nb, C, G, seed) of the kernel cases; draws in this order: z = randn(nb, C) * 3, y = randint(C), a = randint(G)
KERNEL_CASES = [(8, 2, 3, 11), (7, 2, 3, 5), (32, 2, 3, 1), (100, 2, 3, 2), (300, 3, 8, 3), (5, 2, 2, 4)]
ABSENT_CASE = (6, 2, 3, 7)                      # with a = [0, 0, 2, 2, 0, 2]: group 1 is absent
ABSENT_ATTR = [0, 0, 2, 2, 0, 2]
SLICES_CASE = (9, 2, 3, 6)                      # S = 2: logits_img repeats z plus a per-slice offset
SLICE_OFFSETS = [[0.25, -0.5], [-0.25, 0.5]]    # [S, C]
LAMBDA = 0.5
MIN_GAP = 1e-4                                  # min_g |m_g - M| every compared input must keep, so no sign flips on rounding


def draw(nb, C, G, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(nb, C, generator=g) * 3
    y = torch.randint(C, (nb,), generator=g)
    a = torch.randint(G, (nb,), generator=g)
    return z, y, a


def all_kernel_inputs():
    """[(id, logits_img fp32 [nb*S, C], y int64 [nb], a int64 [nb], G, S)] of every kernel case of the issue."""
    out = []
    for nb, C, G, seed in KERNEL_CASES:
        z, y, a = draw(nb, C, G, seed)
        out.append((f"nb{nb}-c{C}-g{G}-s{seed}", z, y, a, G, 1))
    nb, C, G, seed = ABSENT_CASE
    z, y, _ = draw(nb, C, G, seed)
    out.append(("absent-group", z, y, torch.tensor(ABSENT_ATTR), G, 1))
    nb, C, G, seed = SLICES_CASE
    z, y, a = draw(nb, C, G, seed)
    off = torch.tensor(SLICE_OFFSETS)
    out.append(("two-slices", (z[:, None, :] + off[None]).reshape(nb * 2, C).contiguous(), y, a, G, 2))
    return out


def slice_mean(logits_img, nb, S):
    return logits_img.double().view(nb, S, -1).mean(1)


def group_stats(z, y, a, G):
    """float64: (present groups, m_g of them, M, F)."""
    p = torch.softmax(z.double(), 1)
    c = p[torch.arange(len(y)), y]
    present = [g for g in range(G) if bool((a == g).any())]
    if not present:
        return present, torch.zeros(0, dtype=torch.float64), torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    m = torch.stack([1 - c[a == g].mean() for g in present])
    M = m.mean()
    F = (m - M).abs().mean() if len(present) > 1 else torch.zeros((), dtype=torch.float64)
    return present, m, M, F


def min_gap(z, y, a, G):
    present, m, M, _ = group_stats(z, y, a, G)
    return float((m - M).abs().min()) if len(present) > 1 else float("inf")


def fair_term(z, y, a, G):
    """The differentiable term F of logits z (any dtype, stays in the graph)."""
    p = torch.softmax(z, 1)
    c = p[torch.arange(len(y)), y]
    present = [g for g in range(G) if bool((a == g).any())]
    if len(present) <= 1:
        return z.sum() * 0
    m = torch.stack([1 - c[a == g].mean() for g in present])
    return (m - m.mean()).abs().mean()


def autograd_ref(z, y, a, G, lam):
    """float64 autograd through CE + lam * F: (loss, cls, F, dloss/dz)."""
    z = z.double().clone().requires_grad_(True)
    cls = torch.nn.functional.cross_entropy(z, y)
    F = fair_term(z, y, a, G)
    loss = cls + lam * F
    loss.backward()
    return loss.detach(), cls.detach(), F.detach(), z.grad.detach()


def closed_form(z, y, a, G, lam, with_grad=True, dtype=torch.float64):
    """The header's formulas, no autograd: (loss, cls, F, dloss/dz, gstat [G, 2])."""
    z = z.to(dtype)
    nb, C = z.shape
    p = torch.softmax(z, 1)
    onehot = torch.nn.functional.one_hot(y, C).to(dtype)
    c = (p * onehot).sum(1)
    cls = -(torch.log_softmax(z, 1) * onehot).sum(1).mean()
    n = torch.stack([(a == g).sum() for g in range(G)]).to(dtype)
    here = n > 0
    P = int(here.sum())
    m = torch.stack([1 - c[a == g].sum() / n[g] if here[g] else torch.zeros((), dtype=dtype) for g in range(G)])
    M = m[here].sum() / P if P else torch.zeros((), dtype=dtype)
    F = (m[here] - M).abs().sum() / P if P > 1 else torch.zeros((), dtype=dtype)
    sig = torch.where(here, torch.sign(m - M), torch.zeros_like(m))
    sbar = sig.sum() / P if P else torch.zeros((), dtype=dtype)
    kap = torch.where(here, -(sig - sbar) / (P * n.clamp_min(1)), torch.zeros_like(m)) if P > 1 else torch.zeros_like(m)
    inside = (a >= 0) & (a < G)
    kb = torch.where(inside, kap[a.clamp(0, G - 1)], torch.zeros((), dtype=dtype))
    dz = (p - onehot) / nb
    if with_grad:
        dz = dz + lam * (kb * c)[:, None] * (onehot - p)
    return cls + lam * F, cls, F, dz, torch.stack([m, n], 1)
