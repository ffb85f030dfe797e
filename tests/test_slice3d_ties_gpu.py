"""The 3D OCT slice front end (csrc/slice3d.hip) where real volumes put it and random floats never do: per-image extrema that
thousands of pixels attain (black borders, blank padding slices, saturated regions), and images that are not square.

tests/slice3d_ref.py builds inputs whose convolution is exact in float32 and float64 alike, so a tie in the float64 reference
is a tie in the kernel whatever its summation order, and holds the reference (torch autograd through amin / amax, which
spread the gradient evenly over tied extrema).  tests/test_slice3d_ref_cpu.py proves the preconditions without a GPU, among
them that dividing by a count of 1 instead of the tie count is at least 100x the bounds below away.

Bounds (max error / max |reference|): conv, min, max and the counts are EXACT on the exact images; cols 2e-5 in fp32 and
8e-3 in 16-bit storage, dW and dbias 2e-4 - the bounds of test_kernels_gpu.py::test_slice3d_front_end for the same
quantities; the random-float image of every batch keeps that test's 2e-6 on conv / min / max.
"""
from types import SimpleNamespace as NS

import pytest
import torch

from tests import slice3d_ref as R

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]


@pytest.fixture(scope="module")
def ops():
    from fairfedmed_amd import ops
    return ops


def cols_tol(dt):
    return 2e-5 if dt == torch.float32 else 8e-3


def check(got, ref, t, what):
    e = R.rel_err(got.cpu(), ref)
    assert e == e and e <= t, f"{what}: max err / scale = {e:.3e} > {t:.1e}"


class FrontEnd:
    """The buffers of one front end, sized by the library for H x W, and the three launches of a step."""

    def __init__(self, ops, img, w, b, D, ps, dt):
        self.ops, self.D, self.ps = ops, D, ps
        _, C, H, W = img.shape
        N = self.N = C // D
        self.img, self.w, self.b = img.cuda(), w.cuda(), b.cuda()
        P = (H // ps) * (W // ps)
        self.nw = 3 * D * 25 + 3
        self.nwb = ops.slice_wgrad_blocks(H, W)
        self.conv = torch.full((N, 3, H, W), float("nan"), device="cuda")
        self.mm_part = torch.empty(N * ops.slice_blocks(H, W) * 2, device="cuda")
        self.mnmx = torch.empty(N, 2, device="cuda")
        self.cnt = torch.full((N, 2), 77, device="cuda", dtype=torch.int32)          # the library zeroes the counters
        self.cols = torch.full((N * P, 3 * ps * ps), float("nan"), device="cuda", dtype=dt)
        self.dconv = torch.empty_like(self.conv)
        self.ab_part = torch.empty(N * ops.slice_bwd_ab_blocks() * 2, device="cuda")
        self.gmm = torch.empty(N, 2, device="cuda")
        self.wpart = torch.full((N * self.nwb * self.nw,), float("nan"), device="cuda")  # every entry must be written

    def forward(self):
        o = self.ops
        o.slice_conv_fwd(self.img, self.w, self.b, self.conv, self.mm_part, self.mnmx, self.cnt, self.D)
        o.patchify_minmax(self.conv, self.mnmx, self.cnt, self.cols, self.ps, R.MEAN3, R.STD3)
        return NS(conv=self.conv.cpu(), mnmx=self.mnmx.cpu(), cnt=self.cnt.cpu(), cols=self.cols.cpu())

    def backward(self, dcols):
        o = self.ops
        o.slice_bwd(dcols.cuda(), self.img, self.conv, self.mnmx, self.cnt, self.dconv, self.ab_part, self.gmm, self.wpart,
                    self.D, self.ps, R.STD3)
        got = torch.empty(self.nw, device="cuda")
        o.reduce_partials(self.wpart, self.N * self.nwb, self.nw, got)
        got = got.cpu()
        return NS(dW=got[:self.nw - 3].reshape(3, self.D, 5, 5), db=got[self.nw - 3:], gmm=self.gmm.cpu(), flat=got)


def check_tied_case(ops, variant, dt, D, H, W, ps):
    img, w, b, dcols, ref = R.tied_reference(variant, D, H, W, ps, dt)
    assert ref.cnt.tolist()[:2] == R.analytic_counts(variant, H, W) and min(ref.cnt[0].tolist()) >= R.min_tied(H, W)
    fe = FrontEnd(ops, img, w, b, D, ps, dt)
    f = fe.forward()
    # exact arithmetic: any tolerance would hide a dropped tap
    assert torch.equal(f.conv[R.EXACT].double(), ref.conv[R.EXACT]), "conv of the exact images"
    assert torch.equal(f.mnmx[R.EXACT].double(), ref.mnmx[R.EXACT]), (f.mnmx, ref.mnmx)
    check(f.conv[3], ref.conv[3], 2e-6, "conv of the random image")
    check(f.mnmx[3], ref.mnmx[3], 2e-6, "min / max of the random image")
    assert f.cnt.tolist() == ref.cnt.tolist()
    check(f.cols, ref.cols, cols_tol(dt), "patchify_minmax")
    g = fe.backward(dcols)
    print(f"dW err {R.rel_err(g.dW, ref.dW):.3e}  dbias err {R.rel_err(g.db, ref.db):.3e}")
    check(g.dW, ref.dW, R.GRAD_TOL, "slice conv dW")
    check(g.db, ref.db, R.GRAD_TOL, "slice conv dbias")
    # a second step on the same buffers: the counters are zeroed again, not accumulated
    f2 = fe.forward()
    g2 = fe.backward(dcols)
    assert torch.equal(f2.cnt, f.cnt) and torch.equal(g2.gmm, g.gmm) and torch.equal(g2.flat, g.flat)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("D,H,W,ps", R.SQUARE_CASES, ids=[f"d{D}-{H}x{W}" for D, H, W, _ in R.SQUARE_CASES])
def test_tied_extrema(ops, variant, dt, D, H, W, ps):
    """Four images per batch (tests/slice3d_ref.py): a planted saturated / black rectangle across a 64-column strip
    boundary, several 14-row forward blocks and (at 96 rows) the 56-row weight-gradient block boundary; a wholly saturated /
    black image; a random 0/255 image; a random-float image whose counts stay [1, 1]."""
    check_tied_case(ops, variant, dt, D, H, W, ps)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("D,H,W,ps", R.RECT_CASES, ids=[f"{H}x{W}" for _, H, W, _ in R.RECT_CASES])
def test_tied_extrema_on_rectangular_images(ops, dt, D, H, W, ps):
    """H != W: a swapped index or a buffer sized for a square shows here ("saturated": dW sees the division too)."""
    check_tied_case(ops, "saturated", dt, D, H, W, ps)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("H,W", [(48, 80), (80, 48)], ids=["48x80", "80x48"])
def test_random_floats_on_rectangular_images(ops, dt, H, W):
    """test_kernels_gpu.py::test_slice3d_front_end (its inputs' distribution, its bounds) with H != W."""
    N, D, ps = 2, 5, 8
    img, w, b, dcols, ref = R.random_reference(N, D, H, W, ps, dt)
    fe = FrontEnd(ops, img, w, b, D, ps, dt)
    f = fe.forward()
    check(f.conv, ref.conv, 2e-6, "slice conv")
    check(f.mnmx[:, 0], ref.mnmx[:, 0], 2e-6, "min")
    check(f.mnmx[:, 1], ref.mnmx[:, 1], 2e-6, "max")
    check(f.cols, ref.cols, cols_tol(dt), "patchify_minmax")
    assert f.cnt.tolist() == [[1, 1]] * N
    g = fe.backward(dcols)
    check(g.dW, ref.dW, R.GRAD_TOL, "slice conv dW")
    check(g.db, ref.db, R.GRAD_TOL, "slice conv dbias")


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_constant_image_forward(ops, dt):
    """w = 0 and equal biases: min == max, every value is both.  cols = (0 / 1e-5 - mean) / std, all finite, and both
    counters hold 3 H W.  Forward only: the backward is a cancellation over a 1e-5 denominator that float32 cannot hold."""
    N, D, H, W, ps = 2, 4, 40, 40, 8
    img, _, _ = R.random_inputs(N, D, H, W)
    fe = FrontEnd(ops, img, torch.zeros(3, D, 5, 5), torch.full((3,), 0.375), D, ps, dt)
    f = fe.forward()
    assert torch.equal(f.conv, torch.full_like(f.conv, 0.375)) and torch.equal(f.mnmx, torch.full_like(f.mnmx, 0.375))
    assert f.cnt.tolist() == [[3 * H * W, 3 * H * W]] * N
    assert bool(torch.isfinite(f.cols.float()).all())
    want = (-torch.tensor(R.MEAN3, dtype=torch.float64) / torch.tensor(R.STD3, dtype=torch.float64))
    want = want.repeat_interleave(ps * ps).expand(f.cols.shape[0], -1)
    check(f.cols, want, cols_tol(dt), "cols of a constant image")
