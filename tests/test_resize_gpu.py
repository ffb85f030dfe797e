"""ffm_resize_u8 (csrc/resize.hip) against ``data.resize_image``, plane by plane.

The bound.  An output is sum_x a_x (sum_y a_y p_xy) with convex weights and p <= 255, formed in fp32 one rounding per term:
T_y roundings in the vertical sums, T_x in the horizontal one, and one relative 2^-24 each for the rounding of the two
tap weights themselves - (T_y + T_x + 2) * 2^-23 * 255 with a factor 2 of margin on the half-ulp roundings, where T_y and
T_x are the tap counts of the image's own geometry (not the batch's padded T).  Nothing here is fitted to the kernel."""
import numpy as np
import pytest
import torch

from fairfedmed_amd import data as D

pytestmark = pytest.mark.gpu


def run(nb, fill=float("nan")):
    from fairfedmed_amd import ops
    dst = torch.full((len(nb), nb.C1 * nb.rep, nb.R, nb.R), fill, device="cuda")
    return ops.resize_u8(nb.to("cuda"), dst)


def check_against_host(samples, out, rep, R):
    """Every plane of every image within its geometry's bound of resize_image; repeated channels equal."""
    out = out.cpu().double().numpy()
    worst = 0.0
    for b, s in enumerate(samples):
        Ty, Tx = D.resize_taps(s.shape[1], R)[1].shape[1], D.resize_taps(s.shape[2], R)[1].shape[1]
        bound = (Ty + Tx + 2) * 2.0 ** -23 * 255
        for c in range(s.shape[0]):
            ref = D.resize_image(s[c].astype(np.float64), (R, R))
            for k in range(rep):
                err = float(np.abs(out[b, c * rep + k] - ref).max())
                worst = max(worst, err / bound)
                assert err <= bound, (b, c, k, s.shape, err, bound)
            for k in range(1, rep):
                assert np.array_equal(out[b, c * rep + k], out[b, c * rep])
    return worst


def planes(g, c1, h, w):
    return g.integers(0, 256, size=(c1, h, w), dtype=np.uint8)


def test_ragged_batch_matches_resize_image_and_identity_is_expand_u8():
    from fairfedmed_amd import ops
    g = np.random.default_rng(11)
    samples = [planes(g, 1, h, w) for h, w in ((20, 20), (24, 20), (48, 48), (50, 37), (32, 32))]
    nb = D.NativeBatch.from_planes(samples, 3, 32)
    assert nb.T == 4 and nb.w.shape[0] == 5
    out = run(nb)
    assert tuple(out.shape) == (5, 3, 32, 32) and bool(torch.isfinite(out).all())
    print("worst error / bound:", check_against_host(samples, out, 3, 32))
    u8 = torch.from_numpy(samples[4])[None].cuda()
    assert torch.equal(out[4:5], ops.expand_u8(u8, torch.empty(1, 3, 32, 32, device="cuda"), 3))


def test_bscan_form_clips_per_plane():
    """C1 = 4, rep = 1: planes of different ranges inside one image - the clip is the plane's own."""
    g = np.random.default_rng(12)
    samples = []
    for h, w in ((40, 28), (21, 45)):
        s = np.empty((4, h, w), np.uint8)
        s[0] = g.integers(10, 51, size=(h, w))
        s[1] = g.integers(100, 256, size=(h, w))
        s[2] = 77
        s[3] = g.integers(0, 2, size=(h, w)) * 255
        samples.append(s)
    nb = D.NativeBatch.from_planes(samples, 1, 32)
    out = run(nb)
    check_against_host(samples, out, 1, 32)
    for b in range(2):
        assert 10 <= float(out[b, 0].min()) and float(out[b, 0].max()) <= 50
        assert 100 <= float(out[b, 1].min()) and float(out[b, 1].max()) <= 255
        assert bool((out[b, 2] == 77).all())                                       # a constant plane stays constant, exactly
        assert 0 <= float(out[b, 3].min()) and float(out[b, 3].max()) <= 255


def test_real_sizes():
    g = np.random.default_rng(13)
    samples = [planes(g, 1, 336, 336), planes(g, 1, 320, 390)]
    nb = D.NativeBatch.from_planes(samples, 3, 224)
    print("worst error / bound:", check_against_host(samples, run(nb), 3, 224))


def test_an_image_does_not_depend_on_its_batch_or_the_run():
    g = np.random.default_rng(14)
    samples = [planes(g, 2, h, w) for h, w in ((20, 20), (70, 52), (32, 32), (33, 31), (70, 52))]
    nb = D.NativeBatch.from_planes(samples, 1, 32)
    out = run(nb).clone()
    assert torch.equal(out, run(nb))
    for b, s in enumerate(samples):
        alone = D.NativeBatch.from_planes([s], 1, 32)                              # (its own T, not the batch's padded one)
        assert alone.T <= nb.T
        assert torch.equal(run(alone)[0], out[b]), b


def test_odd_byte_offsets():
    """A 1-byte sample in front: every later plane starts at an odd address."""
    g = np.random.default_rng(15)
    samples = [planes(g, 1, 1, 1), planes(g, 1, 37, 41), planes(g, 1, 32, 32), planes(g, 1, 9, 7)]
    nb = D.NativeBatch.from_planes(samples, 3, 32)
    assert nb.geom[:, 0].tolist() == [0, 1, 1 + 37 * 41, 1 + 37 * 41 + 1024]
    out = run(nb)
    check_against_host(samples, out, 3, 32)
    assert bool((out[0] == float(samples[0][0, 0, 0])).all())
    assert torch.equal(out[2, 0].cpu(), torch.from_numpy(samples[2][0]).float())


def test_unsupported_geometry_launches_nothing():
    from fairfedmed_amd import _lib as L, ops
    g = np.random.default_rng(16)
    nb = D.NativeBatch.from_planes([planes(g, 1, 20, 20)], 3, 30)                  # R % 4 != 0
    assert not nb.supported()
    d = nb.to("cuda")
    dst = torch.full((1, 3, 30, 30), -5.0, device="cuda")
    rc = L.load().ffm_resize_u8(L.ptr(d.pix), L.ptr(d.geom), L.ptr(d.start), L.ptr(d.w), L.ptr(dst), 1, 1, 3, 30, d.T,
                                L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -2 and bool((dst == -5.0).all())
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.resize_u8(d, dst)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.resize_u8(nb, dst)                                                     # a host batch: there is no CPU path
