"""float64 numpy reference of the client-level DP mechanism at the round boundary, written from its definition (it does
not import fairfedmed_amd.dp):

    Delta = theta - g (fp32)        nu = ||Delta||_2 (sum of squares in fp64)
    s = 1 (nu <= C) | C / nu (C < nu < inf) | 0 (nu not finite)
    c = w theta | w (g + s Delta) | w g,   + sigma xi when sigma > 0
    xi[i]: lane i & 3 of (r0 cos 2 pi u1, r0 sin 2 pi u1, r2 cos 2 pi u3, r2 sin 2 pi u3), r_j = sqrt(-2 ln u_j),
           u_j = ((x_j >> 9) + 0.5) 2^-23, x = Philox4x32-10(counter (i >> 2, t, k, 0), key (seed low, seed high))
"""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# Random123's known answers: (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox_one(counter, key):
    """One block with Python integers: the definition, for the known answers."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_blocks(c0, c1, c2, c3, key):
    """Vectorised over c0 (uint64 array of 32-bit values); c1..c3 scalars.  Returns uint32 [len(c0), 4]."""
    a = np.asarray(c0, dtype=np.uint64)
    b = np.full_like(a, int(c1) & MASK)
    c = np.full_like(a, int(c2) & MASK)
    d = np.full_like(a, int(c3) & MASK)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    m = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * a, np.uint64(M1) * c
        a, b, c, d = (p1 >> np.uint64(32)) ^ b ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ d ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([a, b, c, d], 1).astype(np.uint32)


def key_of(seed):
    seed = int(seed) & ((1 << 64) - 1)
    return seed & MASK, seed >> 32


def words(n, seed, c0=0, c1=0, c2=0, c3=0):
    """word j = lane j & 3 of the block with counter (c0 + (j >> 2), c1, c2, c3)."""
    groups = (n + 3) // 4
    ctr = (np.arange(groups, dtype=np.uint64) + np.uint64(int(c0) & MASK)) & np.uint64(MASK)
    return philox_blocks(ctr, c1, c2, c3, key_of(seed)).reshape(-1)[:n]


def gaussians(n, seed, t, k):
    """xi[0:n] in float64."""
    x = words(4 * ((n + 3) // 4), seed, 0, t, k, 0).reshape(-1, 4)
    u = ((x >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r0, r2 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a1, a3 = 2.0 * math.pi * u[:, 1], 2.0 * math.pi * u[:, 3]
    return np.stack([r0 * np.cos(a1), r0 * np.sin(a1), r2 * np.cos(a3), r2 * np.sin(a3)], 1).reshape(-1)[:n]


def norm(theta, g):
    """Delta formed in float32, squares and their sum in float64."""
    with np.errstate(all="ignore"):
        d = (np.asarray(theta, np.float32) - np.asarray(g, np.float32)).astype(np.float64)
        return float(np.sqrt(np.sum(d * d)))


def scale(nu, clip):
    clip = float(np.float32(clip))                       # the bound as the fp32 value every layer receives
    if not math.isfinite(nu):
        return 0.0
    return 1.0 if nu <= clip else clip / nu


def w_max(weights):
    """The largest finite weight of any participant on any element."""
    best = 0.0
    for w in weights:
        w = np.asarray(w, np.float64)
        f = w[np.isfinite(w)]
        if f.size:
            best = max(best, float(f.max()))
    return best


def sigma(z, clip, wmax, K):
    return float(np.float32(z * clip * wmax / math.sqrt(K))) if z > 0 else 0.0


def contribution(theta, g, w, clip, sig=0.0, seed=0, t=0, k=0):
    """(c_k in float64, nu, s)."""
    th, gg, ww = (np.asarray(a, np.float32).astype(np.float64) for a in (theta, g, w))
    nu = norm(theta, g)
    s = scale(nu, clip)
    if s == 1.0:
        c = ww * th
    elif s == 0.0:
        c = ww * gg
    else:
        with np.errstate(all="ignore"):
            d = (np.asarray(theta, np.float32) - np.asarray(g, np.float32)).astype(np.float64)
        c = ww * (gg + s * d)
    if sig > 0:
        c = c + float(np.float32(sig)) * gaussians(th.size, seed, t, k)
    return c, nu, s


def finish(total, g, s_offsets, G, r, shared_half, beta_decay):
    """shared_half_s column means on each [G, r] block, then the EMA with the previous global (float64)."""
    avg = np.array(total, np.float64)
    if shared_half:
        for off in s_offsets:
            blk = avg[off:off + G * r].reshape(G, r)
            blk[:, : r // 2] = blk[:, : r // 2].mean(0, keepdims=True)
    return (1.0 - beta_decay) * avg + beta_decay * np.asarray(g, np.float32).astype(np.float64)
