"""Client-level differential privacy at the FedAvg round boundary: configuration, accounting,
and the host restatement of the mechanism for CPU tensors (the gloo plumbing configuration; on a GPU the same mechanism is
ffm_dp_norm + ffm_dp_privatise, csrc/dp.hip).

For participant k of round t with flat buffer theta, previous global g, per-element weights w, K participants::

    nu = || theta - g ||_2                    difference in fp32, squares and sums in fp64
    s  = 1 | C / nu | 0                       nu <= C | C < nu < inf | nu not finite
    c  = w * theta | w * (g + s (theta - g)) | w * g      + sigma * xi   (z > 0)
    sigma = z C w_max / sqrt(K)               w_max: the largest finite weight of any participant on any element

The K noise shares add up to N(0, (z w_max C)^2) per element and zeroing one client's update moves the noiseless sum by at
most w_max C in L2: one round is a Gaussian mechanism with multiplier z (sample counts treated as public).

xi[i] is a function of (seed, t, k, i) alone - Philox4x32-10 with key = (low, high word of seed) and counter (i >> 2, t, k, 0),
uniforms u_j = ((x_j >> 9) + 0.5) 2^-23, Box-Muller in fp32 - so the noise does not depend on the rank, the world size or
the device that draws it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

Tensor = torch.Tensor

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)


@dataclass(frozen=True)
class DPCfg:
    clip: float                       # C: L2 bound on one client's update theta - g over the flat buffer
    noise_multiplier: float = 0.0     # z: 0 clips without noise (no generator runs, epsilon is infinite)
    seed: int = 0                     # 64-bit key of the noise generator
    delta: float = 1e-5               # the delta that `epsilon` reports against

    def __post_init__(self):
        if not (self.clip > 0 and math.isfinite(self.clip)):
            raise ValueError(f"DPCfg.clip must be a positive finite number (got {self.clip})")
        if not (self.noise_multiplier >= 0 and math.isfinite(self.noise_multiplier)):
            raise ValueError(f"DPCfg.noise_multiplier must be >= 0 (got {self.noise_multiplier})")
        if not 0 < self.delta < 1:
            raise ValueError(f"DPCfg.delta must lie in (0, 1) (got {self.delta})")


def epsilon(noise_multiplier: float, rounds: int, delta: float) -> float:
    """(epsilon, delta) after `rounds` Gaussian mechanisms of multiplier z, by zCDP composition (Bun & Steinke 2016):
    rho = rounds / (2 z^2), epsilon = rho + 2 sqrt(rho ln(1 / delta)); inf for z == 0.  An UPPER bound: it ignores the
    amplification by client sampling (frac < 1 only makes the true epsilon smaller)."""
    if rounds <= 0:
        return 0.0
    if noise_multiplier <= 0:
        return math.inf
    rho = rounds / (2.0 * noise_multiplier ** 2)
    return rho + 2.0 * math.sqrt(rho * math.log(1.0 / delta))


def philox4x32_10(counter: np.ndarray, key: Tuple[int, int]) -> np.ndarray:
    """Philox4x32-10 (Random123) on rows of four uint32 counter words; returns the four uint32 output words per row."""
    c = np.asarray(counter, dtype=np.uint32).reshape(-1, 4).astype(np.uint64)
    c0, c1, c2, c3 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _SH) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> _SH) ^ c3 ^ np.uint64(k1), p0 & _MASK
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def _key(seed: int) -> Tuple[int, int]:
    seed &= (1 << 64) - 1
    return seed & 0xFFFFFFFF, seed >> 32


def philox_words(n: int, seed: int, c0: int = 0, c1: int = 0, c2: int = 0, c3: int = 0) -> np.ndarray:
    """Word j = lane j & 3 of Philox4x32-10(counter (c0 + (j >> 2), c1, c2, c3)): what ffm_dp_philox writes."""
    groups = (n + 3) // 4
    ctr = np.empty((groups, 4), dtype=np.uint32)
    ctr[:, 0] = ((np.arange(groups, dtype=np.uint64) + np.uint64(c0 & 0xFFFFFFFF)) & _MASK).astype(np.uint32)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = c1 & 0xFFFFFFFF, c2 & 0xFFFFFFFF, c3 & 0xFFFFFFFF
    return philox4x32_10(ctr, _key(seed)).reshape(-1)[:n]


def gaussians(n: int, seed: int, round: int, client: int) -> np.ndarray:
    """xi[0:n] of the stream (seed, round, client) in fp32."""
    x = philox_words(4 * ((n + 3) // 4), seed, 0, round, client, 0).reshape(-1, 4)
    u = ((x >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    r = np.sqrt(np.float32(-2.0) * np.log(u[:, 0::2]))                    # [groups, 2]: r0, r2
    a = np.float32(2.0 * math.pi) * u[:, 1::2]
    z = np.stack([r[:, 0] * np.cos(a[:, 0]), r[:, 0] * np.sin(a[:, 0]),
                  r[:, 1] * np.cos(a[:, 1]), r[:, 1] * np.sin(a[:, 1])], axis=1)
    return z.astype(np.float32).reshape(-1)[:n]


def noise(n: int, sigma: float, seed: int, round: int, client: int) -> Tensor:
    """sigma * xi as an fp32 CPU tensor (what ffm_dp_noise writes)."""
    return torch.from_numpy(np.float32(sigma) * gaussians(n, seed, round, client))


def weight_max(participants: Sequence[int], n_client: Sequence[int],
               n_client_by_attr: Optional[Sequence[Sequence[int]]], has_group_blocks: bool) -> float:
    """w_max: the largest finite value fedavg.element_weights gives any participant on any element (the same fp32
    arithmetic).  A host scalar every rank computes from the public counts.  The per-attribute weights count only where
    the layout has per-group lora_S blocks to carry them."""
    total = float(sum(n_client[u] for u in participants))
    cand = [float(torch.tensor(n_client[u] / total, dtype=torch.float32)) for u in participants]
    if n_client_by_attr is not None and has_group_blocks:
        by = torch.tensor(n_client_by_attr)
        tot = by[list(participants)].sum(0)
        for u in participants:
            cand += (by[u] / tot).to(torch.float32).tolist()
    finite = [c for c in cand if math.isfinite(c)]
    return max(finite) if finite else 0.0


def sigma(cfg: DPCfg, n_participants: int, w_max: float) -> float:
    """Standard deviation of ONE participant's noise share, as the fp32 value the kernels receive."""
    if cfg.noise_multiplier == 0:
        return 0.0
    return float(np.float32(cfg.noise_multiplier * cfg.clip * w_max / math.sqrt(max(n_participants, 1))))


def clip_scale(theta: Tensor, g: Tensor, clip: float) -> Tuple[float, float]:
    """(nu, s): the update's L2 norm (fp32 difference, fp64 sum of squares) and the clip factor as an fp32 value."""
    with np.errstate(all="ignore"):
        d = (theta.detach().numpy() - g.detach().numpy()).astype(np.float64)
        nu = float(np.sqrt(np.sum(d * d)))
        c = float(np.float32(clip))
        if not math.isfinite(nu):
            return nu, 0.0
        if nu <= c:
            return nu, 1.0
        return nu, float(np.float32(c / nu))


def privatise(theta: Tensor, g: Tensor, w: Tensor, clip: float, sigma_: float, seed: int, round: int,
              client: int) -> Tuple[Tensor, float, float]:
    """(c_k, nu, s) for CPU tensors: every product and sum rounded to fp32 on its own, as the kernel rounds them."""
    nu, s = clip_scale(theta, g, clip)
    if s == 1.0:
        c = theta * w                                        # the product of the aggregator without dp
    elif s == 0.0:
        c = g * w                                            # theta is not read: no Inf * 0
    else:
        c = (g + (theta - g) * s) * w
    if sigma_ > 0:
        c = c + noise(theta.numel(), sigma_, seed, round, client)
    return c, nu, s
