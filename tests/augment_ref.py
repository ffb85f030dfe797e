"""float64 numpy reference of the train-time augmentation, written from its definition (it does not import fairfedmed_amd):

    draws   x = Philox4x32-10(counter (sample id, epoch, a, 0x4D475541), key (seed low, seed high)),
            u_j = ((x_j >> 9) + 0.5) 2^-23                                       (dp_ref's generator)
    box     attempts a = 0..9 on the stored plane H x W, in double:
              area = H W (s0 + u0 (s1 - s0)),  asp = exp(ln r0 + u1 (ln r1 - ln r0)),
              w = floor(sqrt(area asp) + 0.5), h = floor(sqrt(area / asp) + 0.5),
              accepted when 0 < w <= W and 0 < h <= H: top = min(floor(u2 (H - h + 1)), H - h), left likewise from u3;
            after ten refusals torchvision's central box
    flip    attempt index 10, u0 < 0.5
    resize  Pillow's antialiased resample of the box to R x R: per axis scale = n / R, fs = max(1, scale), support = S fs,
            centre c = (o + 0.5) scale, taps x in [max(0, int(c - support + 0.5)), min(n, int(c + support + 0.5))) with
            weight filter((x + 0.5 - c) / fs) normalised to sum 1; horizontal pass, then vertical pass; clamp to [0, 255]
"""
import math
from collections import namedtuple

import numpy as np

from tests import dp_ref

TAG = 0x4D475541
ATTEMPTS = 10

Cfg = namedtuple("Cfg", "crop flip scale ratio", defaults=(True, True, (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)))
Box = namedtuple("Box", "top left h w flip attempt")


def draws(seed, epoch, sid, a):
    """u_0..u_3 of attempt a, float64."""
    x = dp_ref.philox_one((sid, epoch, a, TAG), dp_ref.key_of(seed))
    return [((xj >> 9) + 0.5) * 2.0 ** -23 for xj in x]


def attempts(seed, epoch, sid, H, W, cfg):
    """The ten candidate (w, h) before rounding, as (sqrt(area asp), sqrt(area / asp)): what a test of rounding ties reads."""
    (s0, s1), (r0, r1) = cfg.scale, cfg.ratio
    out = []
    for a in range(ATTEMPTS):
        u = draws(seed, epoch, sid, a)
        area = float(H) * float(W) * (s0 + u[0] * (s1 - s0))
        asp = math.exp(math.log(r0) + u[1] * (math.log(r1) - math.log(r0)))
        out.append((math.sqrt(area * asp), math.sqrt(area / asp), u))
    return out


def box(seed, epoch, sid, H, W, cfg=Cfg()):
    top, left, h, w, att = 0, 0, H, W, -1
    if cfg.crop:
        r0, r1 = cfg.ratio
        for att, (wf, hf, u) in enumerate(attempts(seed, epoch, sid, H, W, cfg)):
            wc, hc = int(math.floor(wf + 0.5)), int(math.floor(hf + 0.5))
            if 0 < wc <= W and 0 < hc <= H:
                w, h = wc, hc
                top = min(int(math.floor(u[2] * (H - h + 1))), H - h)
                left = min(int(math.floor(u[3] * (W - w + 1))), W - w)
                break
        else:
            att = ATTEMPTS
            if W / H < r0:
                w, h = W, int(math.floor(W / r0 + 0.5))
            elif W / H > r1:
                h, w = H, int(math.floor(H * r1 + 0.5))
            else:
                h, w = H, W
            top, left = (H - h) // 2, (W - w) // 2
    flip = int(cfg.flip and draws(seed, epoch, sid, ATTEMPTS)[0] < 0.5)
    return Box(top, left, h, w, flip, att)


def _filter(x, name):
    x = abs(x)
    if name == "bilinear":
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def taps(n, R, filter):
    """One axis, extent n -> R: (start int [R], weights float64 [R, T] zero-padded to the widest run T, counts int [R])."""
    S = {"bilinear": 1.0, "bicubic": 2.0}[filter]
    scale = n / R
    fs = max(1.0, scale)
    support = S * fs
    runs = []
    for o in range(R):
        c = (o + 0.5) * scale
        lo, hi = max(0, int(c - support + 0.5)), min(n, int(c + support + 0.5))
        w = np.array([_filter((x + 0.5 - c) / fs, filter) for x in range(lo, hi)], np.float64)
        runs.append((lo, w / w.sum()))
    T = max(len(w) for _, w in runs)
    start = np.array([lo for lo, _ in runs], np.int64)
    wt = np.zeros((R, T), np.float64)
    for o, (_, w) in enumerate(runs):
        wt[o, :len(w)] = w
    return start, wt, np.array([len(w) for _, w in runs], np.int64)


def matrix(n, R, filter):
    """The same axis as a dense [R, n] matrix."""
    start, wt, cnt = taps(n, R, filter)
    A = np.zeros((R, n), np.float64)
    for o in range(R):
        A[o, start[o]:start[o] + cnt[o]] = wt[o, :cnt[o]]
    return A


def resized_crop_unclamped(plane, box, flip, R, filter):
    """plane [H, W] (any real dtype); box (top, left, h, w).  float64 [R, R]."""
    top, left, h, w = (int(v) for v in box[:4])
    crop = np.asarray(plane, np.float64)[top:top + h, left:left + w]
    assert crop.shape == (h, w), "the box lies outside its plane"
    out = matrix(h, R, filter) @ (crop @ matrix(w, R, filter).T)          # horizontal pass, then vertical
    return out[:, ::-1] if flip else out


def resized_crop(plane, box, flip, R, filter):
    return np.clip(resized_crop_unclamped(plane, box, flip, R, filter), 0.0, 255.0)


def error_bound(box, R, filter):
    """|fp32 kernel - this reference| per plane: one rounding per term of the two sums plus the rounding of the two weights,
    (T_y + T_x + 2) 2^-23 255 L_y L_x with T the table widths and L the largest row sum of |w| (1 for the triangle); the
    factor 2 over the unit roundoff 2^-24 is the slack DESIGN.md section 4.16 keeps."""
    h, w = int(box[2]), int(box[3])
    _, wy, _ = taps(h, R, filter)
    _, wx, _ = taps(w, R, filter)
    Ly, Lx = np.abs(wy).sum(1).max(), np.abs(wx).sum(1).max()
    return (wy.shape[1] + wx.shape[1] + 2) * 2.0 ** -23 * 255.0 * Ly * Lx
