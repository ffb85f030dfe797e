"""Reference and inputs for the 3D OCT slice front end with TIED extrema (csrc/slice3d.hip; trainers/GLP_OT_SVLoRA.py:681-693),
shared by tests/test_slice3d_ref_cpu.py and tests/test_slice3d_ties_gpu.py.  Everything here is float64 torch on the CPU.

    c = conv5x5(image / 255; W [3,D,5,5], b [3], pad 2);  mn, mx = amin / amax of c over (3,H,W) per ViT image
    y = (c - mn) / (mx - mn + 1e-5);  z = (y - mean) / std;  cols = unfold(z, ps)

torch.amin / torch.amax send the gradient of mn / mx to the pixels that attain them, EVENLY when several tie.  `reference`
goes through autograd; `grads_with_counts` restates the backward with the tie counts explicit, so that a test can force them
to 1 (every tied pixel takes the whole gradient: the defect the GPU tests must be able to see).

`build_inputs` makes every convolution value EXACT in float32 and float64 alike, whatever the summation order, so that a tie
in the reference is a tie in the kernel:
  * image values are 0 or 255 only: 255 / 255.0 == 1.0 and 255 * fl32(1 / 255) == 1.0f (the kernels multiply);
  * weights are +-k * 2^-12 (k in 1..8; channel 2 of "saturated" +-k * 2^-13), biases multiples of 2^-8;
  * with D <= 16 a partial sum is a multiple of 2^-13 below 2: 14 bits.
The fourth image of a batch is the random-float one of test_slice3d_front_end; it is NOT exact and keeps that test's bounds.
"""
import functools
from types import SimpleNamespace as NS

import torch

F = torch.nn.functional
MEAN3 = (0.48145466, 0.4578275, 0.40821073)
STD3 = (0.26862954, 0.26130258, 0.27577711)
VARIANTS = ("saturated", "black")
# (D, H, W, ps) of the kernel cases: strips of 64 columns, forward blocks of 14 rows, weight-gradient blocks of 56 rows
SQUARE_CASES = [(4, 96, 96, 16), (16, 32, 32, 8), (5, 40, 40, 8)]
RECT_CASES = [(4, 48, 80, 8), (4, 80, 48, 8)]
N_IMAGES = 4
EXACT = slice(0, 3)                 # images (a), (b), (c): exact arithmetic; (d) is random floats
MIN_TIED = {96 * 96: 1000}          # image (a) must tie at least this often (100 at every other size)
GRAD_TOL = 2e-4                     # the GPU tests' bound on dW / dbias (max error / max |reference|)


def planted_rect(H, W):
    """(r0, r1, c0, c1), inclusive: rows 9..70, cols 37..90 at 96 x 96 and the same proportions elsewhere."""
    return H * 3 // 32, H * 70 // 96, W * 37 // 96, W * 90 // 96


def _q8(x):
    return torch.round(torch.as_tensor(x, dtype=torch.float64) * 256) / 256


@functools.lru_cache(maxsize=None)
def build_inputs(variant, D, H, W, seed=0):
    """(img fp32 [1, 4*D, H, W] raw 0..255, w fp32 [3,D,5,5], b fp32 [3]).  Images: (a) random 0/255 with the planted
    rectangle, (b) wholly saturated / black, (c) random 0/255, (d) rand * 255.  The weights' signs and the biases are chosen
    so that the planted interior attains BOTH extrema of its image (asserted here from the weight sums)."""
    assert variant in VARIANTS and 1 <= D <= 16
    g = torch.Generator().manual_seed(7919 * seed + 31 * D + H + 3 * W + (0 if variant == "saturated" else 1))
    k = torch.randint(1, 9, (3, D, 5, 5), generator=g).double()
    sign2 = torch.where(torch.rand(D, 5, 5, generator=g) < 0.5, -1.0, 1.0).double()
    if variant == "saturated":
        # channel 0 all positive: the maximum is where every tap sees 1; channel 1 all negative: the minimum is there too
        w = torch.stack([k[0], -k[1], 0.5 * k[2] * sign2]) * 2.0 ** -12
    else:
        # channel 0 all negative under the highest bias, channel 1 all positive over the lowest: both at all-black fields
        w = torch.stack([-k[0], k[1], k[2] * sign2]) * 2.0 ** -12
    S = w.abs().sum((1, 2, 3))
    p2, n2 = w[2].clamp_min(0).sum(), -w[2].clamp_max(0).sum()
    b2 = _q8((n2 - p2) / 2)                                         # centres channel 2's range on 0
    if variant == "saturated":
        b = torch.stack([_q8(S[0] / 4), -_q8(S[1] / 4), b2])
        top, bottom = b[0] + S[0], b[1] - S[1]
        assert top > b[1] and bottom < b[0]
    else:
        B = _q8(S.max()) + 2.0 ** -8
        b = torch.stack([B, -B, b2])
        top, bottom = b[0], b[1]
        assert b[0] - S[0] > bottom and b[1] + S[1] < top
    assert b[2] + p2 < top and b[2] - n2 > bottom                   # channel 2 strictly inside
    fill = 255.0 if variant == "saturated" else 0.0
    r0, r1, c0, c1 = planted_rect(H, W)
    img = torch.empty(N_IMAGES, D, H, W)
    img[0] = torch.randint(0, 2, (D, H, W), generator=g).float() * 255
    img[0, :, r0:r1 + 1, c0:c1 + 1] = fill
    img[1] = fill
    img[2] = torch.randint(0, 2, (D, H, W), generator=g).float() * 255
    img[3] = torch.rand(D, H, W, generator=g) * 255
    return img.reshape(1, N_IMAGES * D, H, W).contiguous(), w.float(), b.float()


@functools.lru_cache(maxsize=None)
def random_inputs(N, D, H, W, seed=0):
    """The inputs of test_slice3d_front_end: random floats, unique extrema."""
    g = torch.Generator().manual_seed(97 * seed + N + 31 * D + H + 3 * W)
    img = torch.rand(1, N * D, H, W, generator=g) * 255
    return img, torch.randn(3, D, 5, 5, generator=g) * D ** -0.5, torch.randn(3, generator=g) * 0.1


def analytic_counts(variant, H, W):
    """[[count of the minimum, count of the maximum]] of images (a) and (b)."""
    r0, r1, c0, c1 = planted_rect(H, W)
    a = (r1 - r0 + 1 - 4) * (c1 - c0 + 1 - 4)
    full = (H - 4) * (W - 4) if variant == "saturated" else H * W   # zero padding: a black image is black at its rim too
    return [[a, a], [full, full]]


def min_tied(H, W):
    return MIN_TIED.get(H * W, 100)


def make_dcols(N, H, W, ps, dt=torch.float32, seed=0):
    """The incoming gradient of cols, rounded to the storage type it is handed over in."""
    g = torch.Generator().manual_seed(1013 * seed + N + H + 3 * W + ps)
    return torch.randn(N * (H // ps) * (W // ps), 3 * ps * ps, generator=g).to(dt)


def _front(x, w, b, mn=None, mx=None):
    c = F.conv2d(x, w, b, padding=2)
    return c, (c.amin(dim=(1, 2, 3), keepdim=True) if mn is None else mn), \
        (c.amax(dim=(1, 2, 3), keepdim=True) if mx is None else mx)


def _cols(c, mn, mx, ps):
    y = (c - mn) / (mx - mn + 1e-5)
    z = (y - torch.tensor(MEAN3, dtype=c.dtype).view(1, 3, 1, 1)) / torch.tensor(STD3, dtype=c.dtype).view(1, 3, 1, 1)
    return F.unfold(z, kernel_size=ps, stride=ps).transpose(1, 2).reshape(-1, 3 * ps * ps)


def _x(img, D, dtype):
    H, W = img.shape[-2:]
    return (img.to(dtype) / 255.0).reshape(-1, D, H, W)


def reference(img, w, b, D, ps, dcols=None, dtype=torch.float64):
    """conv [N,3,H,W], mnmx [N,2], cnt [N,2] (ties of min, max), cols [N*P, 3 ps ps] and, given dcols, the autograd
    gradients dW [3,D,5,5] and db [3].  dtype=float32 evaluates the same formulas in float32 (for measuring a tolerance)."""
    wd, bd = w.to(dtype).clone().requires_grad_(), b.to(dtype).clone().requires_grad_()
    c, mn, mx = _front(_x(img, D, dtype), wd, bd)
    cols = _cols(c, mn, mx, ps)
    out = NS(conv=c.detach(), mnmx=torch.cat([mn, mx], 1).reshape(-1, 2).detach(), cols=cols.detach(),
             cnt=torch.stack([(c == mn).sum((1, 2, 3)), (c == mx).sum((1, 2, 3))], 1), dW=None, db=None)
    if dcols is not None:
        cols.backward(dcols.to(dtype))
        out.dW, out.db = wd.grad, bd.grad
    return out


def grads_with_counts(img, w, b, D, ps, dcols, counts=None):
    """(dW, db) with the backward of amin / amax written out: every pixel equal to the extremum takes gradient / count.
    counts=None: the true tie counts (equals `reference`); counts=1: the tied pixels each take ALL of it."""
    wd, bd = w.double().clone().requires_grad_(), b.double().clone().requires_grad_()
    c, mn, mx = _front(_x(img, D, torch.float64), wd, bd)
    c0, mn0, mx0 = (t.detach().clone().requires_grad_() for t in (c, mn, mx))
    gc, gmn, gmx = torch.autograd.grad(_cols(c0, mn0, mx0, ps), (c0, mn0, mx0), dcols.double())
    at_mn, at_mx = (c0 == mn0).double(), (c0 == mx0).double()
    n_mn = at_mn.sum((1, 2, 3), keepdim=True) if counts is None else torch.full_like(mn0, float(counts))
    n_mx = at_mx.sum((1, 2, 3), keepdim=True) if counts is None else torch.full_like(mx0, float(counts))
    dW, db = torch.autograd.grad(c, (wd, bd), gc + at_mn * gmn / n_mn + at_mx * gmx / n_mx)
    return dW, db


def rel_err(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def tied_reference(variant, D, H, W, ps, dt):
    """(inputs, dcols in dt, reference) of one tied case: computed once, shared by the tests, never written to."""
    img, w, b = build_inputs(variant, D, H, W)
    dcols = make_dcols(N_IMAGES, H, W, ps, dt)
    return img, w, b, dcols, reference(img, w, b, D, ps, dcols)


@functools.lru_cache(maxsize=None)
def random_reference(N, D, H, W, ps, dt):
    img, w, b = random_inputs(N, D, H, W)
    dcols = make_dcols(N, H, W, ps, dt, seed=1)
    return img, w, b, dcols, reference(img, w, b, D, ps, dcols)
