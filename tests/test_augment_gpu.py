"""Train-time augmentation on the GPU (csrc/augment.hip) against tests/augment_ref.py.

Boxes are integers: ffm_augment_boxes is held to the float64 reference exactly.  The resample is held, plane by plane, to

    |out - ref| <= (T_y + T_x + 2) * 2^-23 * 255 * L_y * L_x

with T the widths of the reference's two tap tables for that box and L the largest row sum of |w| (1 for the triangle): one
fp32 rounding per term of the two sums plus the rounding of the two weights, with the factor 2 on the half-ulp roundings that
section 4.16 keeps.  Through the engines and the trainer everything is held to torch.equal against the float32 tensor
ops.augment_u8 leaves.  Nothing here is fitted to the kernel."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from fairfedmed_amd import config as C
from fairfedmed_amd import data as D
from fairfedmed_amd import synth
from tests import augment_ref as A

pytestmark = pytest.mark.gpu

GEOMS = ((40, 56), (224, 224), (512, 664), (96, 20))
SEED = 5


@pytest.fixture(scope="module")
def ref_boxes():
    """{epoch: int32 [4 * 64, 6]} of the float64 reference with crop and flip both on: geometry-major, 64 ids each."""
    return {e: np.array([tuple(A.box(SEED, e, i, H, W)) for H, W in GEOMS for i in range(64)], np.int32) for e in range(3)}


@pytest.mark.parametrize("crop,flip", [(True, False), (False, True), (True, True), (False, False)],
                         ids=["crop", "flip", "both", "neither"])
def test_boxes_equal_the_reference(ref_boxes, crop, flip):
    from fairfedmed_amd import ops
    geom = torch.tensor([[0, H, W, -1] for H, W in GEOMS for _ in range(64)], dtype=torch.int32, device="cuda")
    ids = torch.arange(64, dtype=torch.int32).repeat(4).cuda()
    cfg = C.AugmentCfg(crop=crop, flip=flip)
    for e in range(3):
        want = ref_boxes[e].copy()
        if not crop:
            want[:, 0:2], want[:, 2], want[:, 3], want[:, 5] = 0, geom[:, 1].cpu().numpy(), geom[:, 2].cpu().numpy(), -1
        if not flip:
            want[:, 4] = 0
        got = ops.augment_boxes(geom, ids, SEED, e, cfg).cpu().numpy()
        assert np.array_equal(got[:, 6:], np.zeros((256, 2), np.int32))
        bad = np.nonzero((got[:, :6] != want).any(1))[0]
        assert bad.size == 0, (e, bad[:4], got[bad[:4]], want[bad[:4]])
    if crop:
        assert (ref_boxes[0][:, 5] == 10).any() and ((ref_boxes[0][:, 5] > 0) & (ref_boxes[0][:, 5] < 10)).any()
    # another seed, and a 64-bit one: the key is both words of the seed
    s2 = (3 << 32) | 9
    got = ops.augment_boxes(geom[:4], ids[:4], s2, 1, C.AugmentCfg(crop=True, flip=True)).cpu().numpy()
    assert np.array_equal(got[:, :6], np.array([tuple(A.box(s2, 1, i, 40, 56)) for i in range(4)], np.int32))


def _boxes(rows):
    return torch.tensor([list(r) + [0, 0, 0] for r in rows], dtype=torch.int32, device="cuda")


# (stored size, box (top, left, h, w), flip): a shrink inside a plane, a 3x shrink of a whole plane, an enlargement, a constant,
# the identity and its mirror; and the first one mirrored
CASES = (((40, 56), (3, 5, 30, 41), 0), ((96, 64), (0, 0, 96, 64), 0), ((96, 64), (7, 1, 9, 11), 0), ((64, 64), (5, 6, 1, 1), 0),
         ((32, 32), (0, 0, 32, 32), 0), ((32, 32), (0, 0, 32, 32), 1), ((40, 56), (3, 5, 30, 41), 1))


@pytest.fixture(scope="module")
def case_planes():
    g = np.random.default_rng(31)
    planes = [g.integers(0, 256, size=(3, h, w), dtype=np.uint8) for (h, w), _, _ in CASES]
    planes[5] = planes[4].copy()                                        # the mirror is of the same bytes
    return planes


@pytest.fixture(scope="module")
def case_refs(case_planes):
    """{filter: per case [3 planes of float64 [32, 32]]}, computed once."""
    return {f: [[A.resized_crop(p[c], box, flip, 32, f) for c in range(3)] for p, (_, box, flip) in zip(case_planes, CASES)]
            for f in ("bilinear", "bicubic")}


@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
@pytest.mark.parametrize("C1,rep", [(1, 3), (3, 1)], ids=["slo", "bscans"])
def test_resample_at_supplied_boxes(case_planes, case_refs, filter, C1, rep):
    from fairfedmed_amd import ops
    samples = [p[:C1] for p in case_planes]
    nb = D.NativeBatch.from_planes(samples, rep, 32, tables=False).to("cuda")
    boxes = _boxes([box + (flip,) for _, box, flip in CASES])
    dst = torch.full((len(CASES), 3, 32, 32), float("nan"), device="cuda")
    out = ops.crop_resize_u8(nb, boxes, dst, filter)
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 255.0
    o = out.cpu().double().numpy()
    worst = 0.0
    for b, (_, box, flip) in enumerate(CASES):
        bound = A.error_bound(box, 32, filter)
        for c in range(C1):
            for k in range(rep):
                err = float(np.abs(o[b, c * rep + k] - case_refs[filter][b][c]).max())
                worst = max(worst, err / bound)
                assert err <= bound, (b, c, k, box, filter, err, bound)
            for k in range(1, rep):
                assert np.array_equal(o[b, c * rep + k], o[b, c * rep])
    print("worst error / bound:", worst)
    assert bool((out[3] == out[3, :, :1, :1]).all())                    # a 1 x 1 box: the constant, exactly
    assert np.array_equal(o[3, 0], np.full((32, 32), float(samples[3][0, 5, 6])))
    u8 = torch.from_numpy(samples[4])[None].cuda()
    same = ops.expand_u8(u8, torch.empty(1, 3, 32, 32, device="cuda"), rep)
    assert torch.equal(out[4:5], same) and torch.equal(out[5:6], same.flip(-1))


def test_cubic_overshoot_is_clamped():
    from fairfedmed_amd import ops
    plane = (np.kron(np.indices((8, 8)).sum(0) % 2, np.ones((8, 8))) * 255).astype(np.uint8)        # 8 x 8 blocks of 0 and 255
    box = (3, 5, 50, 41)
    raw = A.resized_crop_unclamped(plane, box, 0, 32, "bicubic")
    assert raw.min() < -1.0 and raw.max() > 256.0                       # the unclamped reference leaves [0, 255]
    nb = D.NativeBatch.from_planes([plane[None]], 3, 32, tables=False).to("cuda")
    out = ops.crop_resize_u8(nb, _boxes([box + (0,)]), torch.empty(1, 3, 32, 32, device="cuda"), "bicubic")
    assert float(out.min()) == 0.0 and float(out.max()) == 255.0
    err = float(np.abs(out[0, 0].cpu().double().numpy() - np.clip(raw, 0, 255)).max())
    print("error", err, "bound", A.error_bound(box, 32, "bicubic"))
    assert err <= A.error_bound(box, 32, "bicubic")


def test_what_the_kernel_does_not_serve_is_refused():
    from fairfedmed_amd import _lib as L, ops
    g = np.random.default_rng(33)
    nb = D.NativeBatch.from_planes([g.integers(0, 256, size=(1, 20, 24), dtype=np.uint8)], 3, 32, tables=False).to("cuda")
    dst = torch.full((1, 3, 32, 32), -5.0, device="cuda")
    for bad in ((0, 0, 21, 24), (1, 0, 20, 24), (0, 5, 20, 20), (-1, 0, 4, 4), (0, 0, 0, 4)):
        with pytest.raises(RuntimeError, match="outside its 20 x 24 plane"):
            ops.crop_resize_u8(nb, _boxes([bad + (0,)]), dst)
    # the launch itself cannot read a box: on the device such a block reads no pixel and leaves NaN, never a wrong image
    nan = ops.crop_resize_u8(nb, _boxes([(1, 0, 20, 24, 0)]), torch.zeros(1, 3, 32, 32, device="cuda"), check_boxes=False)
    assert bool(torch.isnan(nan).all())
    wide = D.NativeBatch.from_planes([g.integers(0, 256, size=(1, 4, 32 * 40), dtype=np.uint8)], 3, 32, tables=False).to("cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.crop_resize_u8(wide, _boxes([(0, 0, 4, 1280, 0)]), dst, "bicubic")
    odd = D.NativeBatch.from_planes([g.integers(0, 256, size=(1, 20, 24), dtype=np.uint8)], 3, 30, tables=False).to("cuda")
    d30 = torch.full((1, 3, 30, 30), -5.0, device="cuda")
    rc = L.load().ffm_crop_resize_u8(L.ptr(odd.pix), L.ptr(odd.geom), L.ptr(_boxes([(0, 0, 20, 24, 0)])), L.ptr(d30), 1, 1, 3, 30,
                                     0, 24, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -2 and bool((d30 == -5.0).all()) and bool((dst == -5.0).all())     # nothing was launched


def _aug_batch(samples, ids, epoch=2, seed=SEED, R=32, rep=3, cfg=C.AugmentCfg(crop=True, flip=True)):
    return D.NativeBatch.augmented(samples, rep, R, ids, epoch, seed, cfg).to("cuda")


def _run(nb):
    from fairfedmed_amd import ops
    return ops.augment_u8(nb, torch.full((len(nb), nb.C1 * nb.rep, nb.R, nb.R), float("nan"), device="cuda")).clone()


def test_a_sample_does_not_depend_on_its_batch_or_the_run():
    g = np.random.default_rng(34)
    mk = lambda h, w: g.integers(0, 256, size=(1, h, w), dtype=np.uint8)
    s = mk(70, 52)
    alone = _run(_aug_batch([s], [11]))
    five = [mk(40, 56), mk(33, 31), mk(96, 64), s, mk(32, 32)]
    a = _run(_aug_batch(five, [3, 4, 5, 11, 6]))
    others = [mk(20, 90), s, mk(64, 64), mk(9, 7), mk(50, 50)]
    b = _run(_aug_batch(others, [40, 11, 41, 42, 43]))
    assert torch.equal(alone[0], a[3]) and torch.equal(alone[0], b[1])
    assert torch.equal(a, _run(_aug_batch(five, [3, 4, 5, 11, 6])))      # two calls
    # and it is the reference's box for (seed, epoch, id), resampled within the bound
    box = A.box(SEED, 2, 11, 70, 52)
    ref = A.resized_crop(s[0], box, box.flip, 32, "bilinear")
    assert float(np.abs(alone[0, 0].cpu().double().numpy() - ref).max()) <= A.error_bound(box, 32, "bilinear")
    assert not torch.equal(alone[0], _run(_aug_batch([s], [11], epoch=3))[0])        # another epoch: another crop
    assert not torch.equal(alone[0], _run(_aug_batch([s], [12]))[0])                 # another id


@pytest.mark.parametrize("case", ["vit", "rn"])
def test_engines_take_an_augmenting_batch_as_the_augmented_tensor(case):
    from fairfedmed_amd import ops
    from fairfedmed_amd.engine_rn import create_engine
    mcfg = C.rn_tiny(rank=4, num_groups=2) if case == "rn" else C.vit_tiny(rank=4)
    g = np.random.default_rng(35)
    samples = [g.integers(0, 256, size=(1, h, w), dtype=np.uint8) for h, w in ((40, 40), (96, 96), (64, 64), (50, 70))]
    nb = _aug_batch(samples, [8, 1, 5, 2], R=64, cfg=C.AugmentCfg(crop=True, flip=True, filter="bicubic"))
    f32 = ops.augment_u8(nb, torch.empty(4, 3, 64, 64, device="cuda")).clone()
    tg = torch.Generator().manual_seed(3)
    attr = torch.randint(0, mcfg.lora.num_groups, (4,), generator=tg).cuda()
    label = torch.randint(0, 2, (4,), generator=tg).cuda()
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    ea = create_engine(mcfg, sd, dtype=torch.float32, max_images=8)
    eb = create_engine(mcfg, sd, dtype=torch.float32, max_images=8)
    # what the engines took before, they take as before (first: a training step moves RN50's BatchNorm statistics)
    plain = D.NativeBatch.from_planes(samples[:3], 3, 64).to("cuda")
    r32 = ops.resize_u8(plain, torch.empty(3, 3, 64, 64, device="cuda")).clone()
    assert torch.equal(ea.forward(r32, attr[:3]), eb.forward(plain, attr[:3]))
    u8 = torch.from_numpy(samples[2])[None].cuda()
    e32 = ops.expand_u8(u8, torch.empty(1, 3, 64, 64, device="cuda"), 3).clone()
    assert torch.equal(ea.forward(e32, attr[:1]), eb.forward(u8, attr[:1]))
    oa, ob = ea.forward_backward(f32, attr, label), eb.forward_backward(nb, attr, label)
    assert torch.equal(oa["loss"], ob["loss"]) and torch.equal(oa["logits"], ob["logits"])
    assert torch.equal(ea.params.grad, eb.params.grad) and float(ea.params.grad.abs().max()) > 0
    ob2 = eb.forward_backward(nb, attr, label)                          # (the replayed plan: inputs load outside it)
    assert torch.equal(ob2["loss"], oa["loss"])
    with pytest.raises(ValueError, match="resizes to 32"):
        eb.forward(_aug_batch(samples, [8, 1, 5, 2], R=32), attr)


def make_cfg(root, transforms, bs=8):
    return NS(
        SEED=1, OUTPUT_DIR="", VERBOSE=False,
        INPUT=NS(PIXEL_MEAN=list(C.CLIP_PIXEL_MEAN), PIXEL_STD=list(C.CLIP_PIXEL_STD), SIZE=(64, 64), TRANSFORMS=transforms),
        DATASET=NS(NAME="FairFedMed", ROOT=root, USERS=2, ATTRIBUTE_TYPE="race", ATTRIBUTES=["race", "gender"],
                   MODALITY_TYPE="slo_fundus"),
        MODEL=NS(BACKBONE=NS(NAME="tiny"), GEOMETRY=C.vit_tiny(), STATE_DICT=None),
        TRAINER=NS(NAME="GLP_OT_SVLoRA", LAMBDA_FAIRNESS=0.0,
                   GLP_OT=NS(N=2, N_CTX=4, PREC="fp32", OT="None"),
                   GLP_OT_LORA=NS(RANK=4, ALPHA=2.0, TYPE="FairLoRA", GLOBAL_S=False, DISABLE_ATTR=False,
                                  UNFREEZE_IMAGE_ENCODER=True)),
        OPTIM=NS(NAME="sgd", LR=1e-3, MOMENTUM=0.9, WEIGHT_DECAY=5e-4, LR_SCHEDULER="single_step", STEPSIZE=2,
                 GAMMA=0.1, MAX_EPOCH=1),
        DATALOADER=NS(TRAIN_X=NS(BATCH_SIZE=bs)), TEST=NS(BATCH_SIZE=bs, NO_TEST=True),
        TRAIN=NS(METRICS_EVERY=1, CHECKPOINT_FREQ=0),
    )


def test_trainer_with_transforms_is_reproducible_and_leaves_testing_alone(tmp_path):
    """Two clients read a FairFedMed tree stored at 40 and 64 pixels (tower: 64)."""
    from fairfedmed_amd import federated as F
    from fairfedmed_amd.registry import build_trainer
    import fairfedmed_amd.trainer  # noqa: F401  (registers GLP_OT_SVLoRA)
    D.write_synthetic_fairfedmed(str(tmp_path), sites=2, n_train=16, n_test=8, seed=4, sizes=[40, 64])
    sd = synth.make_state_dict(C.vit_tiny(rank=4), seed=1, lora_init="reference")
    both = ["random_resized_crop", "random_flip"]
    hist, tests = {}, {}
    for mode, transforms in (("a", both), ("b", both), ("plain", [])):
        cfg = make_cfg(str(tmp_path), transforms)
        cfg.DATA = D.FedData(cfg, transport="native")
        cfg.MODEL.STATE_DICT = sd
        tr = build_trainer(cfg)
        first = next(iter(tr.fed_train_loader_x_dict[0]))["img"]
        assert isinstance(first, D.NativeBatch) and (first.augment is not None) == bool(transforms)
        assert next(iter(tr.fed_test_loader_x_dict[0]))["img"].augment is None
        tests[mode] = list(tr.test(idx=0))                              # one fixed model: the weights every run starts from
        hist[mode] = F.run_fedotplora(tr, F.FedArgs(num_users=2, frac=1.0, round=2, shared_half_s=True, seed=0),
                                      log=lambda *_: None)
        assert tr.fed_train_loader_x_dict[0].epoch >= 2
    assert tests["a"] == tests["plain"] == tests["b"]
    differs = False
    for k, v in hist["a"]["global_weights"].items():
        assert torch.equal(v, hist["b"]["global_weights"][k]), k
        assert bool(torch.isfinite(v).all())
        differs = differs or not torch.equal(v, hist["plain"]["global_weights"][k])
    assert differs
    # a data manager whose loaders do not augment is refused, never trained un-augmented
    cfg = make_cfg(str(tmp_path), both)
    plain_data = D.FedData(make_cfg(str(tmp_path), []), transport="native")
    with pytest.raises(ValueError, match="do not augment"):
        build_trainer(NS(**{**vars(cfg), "DATA": plain_data}))
