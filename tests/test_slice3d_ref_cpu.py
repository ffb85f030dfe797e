"""Preconditions of tests/test_slice3d_ties_gpu.py, on the reference alone and without a GPU: the built inputs are exact in
float32, their extrema are tied as often as stated, and a backward that hands every tied pixel the undivided gradient is at
least 100x the GPU tests' tolerance away from the true one.  If one of these fails the inputs are wrong, not the kernel."""
import pytest
import torch

from tests import slice3d_ref as R

F = torch.nn.functional
CASES = R.SQUARE_CASES + R.RECT_CASES
IDS = [f"d{D}-{H}x{W}" for D, H, W, _ in CASES]


def test_255_times_the_float32_reciprocal_is_exactly_one():
    """The second-generation kernels multiply by fl32(1/255) where the reference divides by 255."""
    r = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(255.0, dtype=torch.float32)
    assert float(torch.tensor(255.0, dtype=torch.float32) * r) == 1.0 and 255.0 / 255.0 == 1.0


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("D,H,W,ps", CASES, ids=IDS)
def test_built_convolution_is_exact_in_float32(variant, D, H, W, ps):
    img, w, b = R.build_inputs(variant, D, H, W)
    vals = img.reshape(R.N_IMAGES, D, H, W)[R.EXACT].unique().tolist()
    assert set(vals) <= {0.0, 255.0}
    x32 = (img / 255.0).reshape(-1, D, H, W)
    c32 = F.conv2d(x32, w, b, padding=2)
    c64 = F.conv2d(x32.double(), w.double(), b.double(), padding=2)
    assert torch.equal(c32[R.EXACT].double(), c64[R.EXACT])
    # another summation order (taps reversed) gives the same bits: no partial sum rounds
    c32r = F.conv2d(x32.flip(1, 2, 3), w.flip(1, 2, 3), b, padding=2).flip(2, 3)
    assert torch.equal(c32r[R.EXACT], c32[R.EXACT])


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("D,H,W,ps", CASES, ids=IDS)
def test_tie_counts_are_the_analytic_ones(variant, D, H, W, ps):
    img, w, b = R.build_inputs(variant, D, H, W)
    ref = R.reference(img, w, b, D, ps)
    cnt = ref.cnt.tolist()
    assert cnt[:2] == R.analytic_counts(variant, H, W), cnt
    assert min(cnt[0]) >= R.min_tied(H, W)
    assert cnt[3] == [1, 1]                                          # the random-float image keeps unique extrema
    # both extrema of image (a) sit in the planted interior, on channel 1 (minimum) and channel 0 (maximum)
    r0, r1, c0, c1 = R.planted_rect(H, W)
    inner = ref.conv[0, :, r0 + 2:r1 - 1, c0 + 2:c1 - 1]
    assert bool((inner[1] == ref.mnmx[0, 0]).all()) and bool((inner[0] == ref.mnmx[0, 1]).all())


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("D,H,W,ps", CASES, ids=IDS)
def test_forcing_the_counts_to_one_is_far_outside_the_gpu_tolerance(variant, D, H, W, ps):
    img, w, b, dcols, ref = R.tied_reference(variant, D, H, W, ps, torch.float32)
    dW, db = R.grads_with_counts(img, w, b, D, ps, dcols)           # the written-out backward is autograd's
    assert R.rel_err(dW, ref.dW) < 1e-9 and R.rel_err(db, ref.db) < 1e-9
    dW1, db1 = R.grads_with_counts(img, w, b, D, ps, dcols, counts=1)
    assert R.rel_err(db1, ref.db) >= 100 * R.GRAD_TOL, R.rel_err(db1, ref.db)
    if variant == "saturated":                                      # ("black": the tied pixels see x = 0, dW cannot tell)
        assert R.rel_err(dW1, ref.dW) >= 100 * R.GRAD_TOL, R.rel_err(dW1, ref.dW)


def test_random_inputs_have_unique_extrema():
    for N, D, H, W, ps in ((2, 5, 48, 80, 8), (2, 5, 80, 48, 8)):
        img, w, b = R.random_inputs(N, D, H, W)
        assert R.reference(img, w, b, D, ps).cnt.tolist() == [[1, 1]] * N
