"""Train-time augmentation without a GPU: the float64 restatement (tests/augment_ref.py) pinned against Pillow, its draws
against the Philox known answers, the statistics of its boxes, the parser / config / loader plumbing and the argument checks of
the three entry points."""
import ctypes
import math
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from fairfedmed_amd import _lib, config as C, data as D
from tests import augment_ref as A
from tests import dp_ref

GEOMS = ((40, 56), (224, 224), (512, 664), (96, 20))


@pytest.fixture(scope="module")
def boxes():
    """64 ids x 3 epochs at each geometry: {(H, W): [(id, epoch, Box), ...]}, computed once."""
    return {(H, W): [(i, e, A.box(5, e, i, H, W)) for e in range(3) for i in range(64)] for H, W in GEOMS}


def test_philox_known_answers_and_the_draw_rule():
    for ctr, key, out in dp_ref.KAT:
        assert dp_ref.philox_one(ctr, key) == out
    seed = (0x299f31d0 << 32) | 0xa4093822                              # the third known answer as (seed, id, epoch, a)
    x = dp_ref.philox_one((7, 2, 3, A.TAG), dp_ref.key_of(seed))
    assert A.draws(seed, 2, 7, 3) == [((v >> 9) + 0.5) * 2.0 ** -23 for v in x]
    assert A.TAG == 0x4D475541 and all(0.0 < u < 1.0 for u in A.draws(1, 0, 0, 0))


@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
def test_restatement_matches_pillow(filter):
    """Pillow resamples a mode-F image in fp32 (fp32 between the passes, double weights): it stays within the fp32 bound of
    the float64 restatement, plane by plane; the 224^2 identity is exact."""
    Image = pytest.importorskip("PIL.Image")
    pf = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[filter]
    g = np.random.default_rng(3)
    cases = [((40, 56), (3, 5, 30, 41), 32), ((96, 64), (0, 0, 96, 64), 32), ((96, 64), (7, 1, 9, 11), 32),
             ((64, 64), (5, 6, 1, 1), 32), ((336, 336), (0, 0, 336, 336), 224), ((512, 664), (69, 71, 407, 475), 224),
             ((512, 664), (0, 0, 512, 664), 224), ((224, 224), (0, 0, 224, 224), 224)]
    worst = 0.0
    for (H, W), box, R in cases:
        plane = g.integers(0, 256, size=(H, W), dtype=np.uint8)
        top, left, h, w = box
        crop = plane[top:top + h, left:left + w]
        ref = np.asarray(Image.fromarray(crop.astype(np.float32), "F").resize((R, R), pf), np.float64)
        got = A.resized_crop_unclamped(plane, box, 0, R, filter)
        err, bound = float(np.abs(got - ref).max()), A.error_bound(box, R, filter)
        worst = max(worst, err / bound)
        print((H, W), box, R, filter, "error", err, "bound", bound)
        assert err <= bound, ((H, W), box, err, bound)
        if (h, w) == (R, R):
            assert np.array_equal(got, crop.astype(np.float64)) and np.array_equal(ref, got)
        assert np.array_equal(A.resized_crop_unclamped(plane, box, 1, R, filter), got[:, ::-1])
    print("worst error / bound:", worst)


def test_identity_axis_is_one_tap_of_weight_one():
    for f in ("bilinear", "bicubic"):
        assert np.array_equal(A.matrix(32, 32, f), np.eye(32))
        start, w, cnt = A.taps(475, 224, f)
        assert np.allclose(w.sum(1), 1.0, atol=1e-15) and int(cnt.max()) == w.shape[1]
        assert (start >= 0).all() and (start + cnt <= 475).all()


def test_boxes_lie_inside_their_planes_and_cover_every_branch(boxes):
    fallbacks = later = 0
    for (H, W), rows in boxes.items():
        for i, e, b in rows:
            assert 0 <= b.top and 0 <= b.left and 0 < b.h <= H - b.top and 0 < b.w <= W - b.left, ((H, W), i, e, b)
            assert b.flip in (0, 1) and 0 <= b.attempt <= 10
            fallbacks += b.attempt == 10
            later += 0 < b.attempt < 10
    assert fallbacks >= 1 and later >= 1
    n9620 = sum(b.attempt == 10 for _, _, b in boxes[(96, 20)])
    print("fallbacks:", fallbacks, "of which 96 x 20:", n9620, "accepted after attempt 0:", later)
    for _, _, b in boxes[(96, 20)]:                                     # W/H < 3/4: the central box is full width
        if b.attempt == 10:
            assert (b.w, b.h, b.left, b.top) == (20, 27, 0, (96 - 27) // 2)


def test_no_accepted_draw_is_near_a_rounding_tie(boxes):
    """w and h are floor(x + 0.5): a draw whose x sits within 1e-6 of k + 0.5 could round the other way under another libm.
    None does, so the device's double exp / sqrt cannot move a box."""
    cfg, closest = A.Cfg(), 1.0
    for (H, W), rows in boxes.items():
        for i, e, b in rows:
            for a, (wf, hf, _) in enumerate(A.attempts(5, e, i, H, W, cfg)):
                if a > min(b.attempt, 9):
                    break
                for v in (wf, hf):                                      # (refused attempts count too: a tie could accept them)
                    closest = min(closest, abs(v + 0.5 - round(v + 0.5)))
    print("smallest distance to a tie:", closest)
    assert closest > 1e-6


def test_boxes_depend_on_id_and_epoch_and_flips_are_fair(boxes):
    rows = boxes[(512, 664)]
    by = {(i, e): b for i, e, b in rows}
    assert sum(by[(i, 0)][:4] != by[(i, 1)][:4] for i in range(64)) >= 60
    assert sum(by[(i, 0)][:4] != by[(i + 1, 0)][:4] for i in range(63)) >= 59
    assert by[(3, 1)] == A.box(5, 1, 3, 512, 664) and by[(3, 1)][:4] != A.box(6, 1, 3, 512, 664)[:4]
    flips = [b.flip for rows in boxes.values() for _, _, b in rows]
    share = sum(flips) / len(flips)
    print("share of flips:", share)
    assert len(flips) == 768 and 0.45 <= share <= 0.55
    off = A.Cfg(crop=False, flip=False)
    assert A.box(5, 0, 3, 40, 56, off) == A.Box(0, 0, 40, 56, 0, -1)
    assert A.box(5, 0, 3, 40, 56, A.Cfg(crop=False)).flip == by_flip(5, 0, 3)


def by_flip(seed, epoch, sid):
    return int(A.draws(seed, epoch, sid, 10)[0] < 0.5)


# ------------------------------------------------------------------------------------------- parser and config --
ARGV = ["--root", "DATA/", "--unfreeze_image_encoder", "True", "--OT", "None", "--transport", "native"]


def test_flags_reach_the_config_tree():
    from fairfedmed_amd import federated_main as FM
    args = FM.build_parser().parse_args(ARGV + ["--transforms", "random_resized_crop", "random_flip", "normalize",
                                                "--rrcrop_scale", "0.3", "0.9", "--interpolation", "bicubic"])
    cfg = FM.setup_cfg(args)
    FM.check_scope(args, cfg)
    assert cfg.INPUT.TRANSFORMS == ("random_resized_crop", "random_flip", "normalize")
    assert cfg.INPUT.RRCROP_SCALE == (0.3, 0.9) and cfg.INPUT.INTERPOLATION == "bicubic"
    aug = C.augment_from_cfg(cfg)
    assert aug == C.AugmentCfg(crop=True, flip=True, scale=(0.3, 0.9), filter="bicubic") and aug.active
    assert aug.ratio == (3.0 / 4.0, 4.0 / 3.0)
    # defaults: nothing configured, nothing changes
    cfg0 = FM.setup_cfg(FM.build_parser().parse_args(ARGV))
    assert cfg0.INPUT.TRANSFORMS == () and cfg0.INPUT.RRCROP_SCALE == (0.08, 1.0) and cfg0.INPUT.INTERPOLATION == "bilinear"
    assert C.augment_from_cfg(cfg0) is None
    cfg1 = FM.setup_cfg(FM.build_parser().parse_args(ARGV + ["--transforms", "normalize"]))
    assert C.augment_from_cfg(cfg1) is None                             # normalize alone: the towers already normalise
    flip = C.augment_from_cfg(FM.setup_cfg(FM.build_parser().parse_args(ARGV + ["--transforms", "random_flip"])))
    assert flip == C.AugmentCfg(flip=True) and not flip.crop and flip.scale == (0.08, 1.0)


def test_config_file_sets_the_transforms(tmp_path):
    from fairfedmed_amd import federated_main as FM
    (tmp_path / "tr.yaml").write_text('INPUT:\n  SIZE: (224, 224)\n  INTERPOLATION: "bicubic"\n  RRCROP_SCALE: (0.5, 1.0)\n'
                                      '  TRANSFORMS: ["random_resized_crop", "random_flip", "normalize"]\n')
    cfg = FM.setup_cfg(FM.build_parser().parse_args(ARGV + ["--config-file", str(tmp_path / "tr.yaml")]))
    assert C.augment_from_cfg(cfg) == C.AugmentCfg(crop=True, flip=True, scale=(0.5, 1.0), filter="bicubic")


def test_what_cannot_be_augmented_is_refused_by_name():
    from fairfedmed_amd import federated_main as FM

    def scope(extra):
        args = FM.build_parser().parse_args(extra)
        FM.check_scope(args, FM.setup_cfg(args))

    with pytest.raises(NotImplementedError, match="color_jitter"):
        scope(ARGV + ["--transforms", "random_flip", "color_jitter"])
    with pytest.raises(ValueError, match="NO_TRANSFORM"):
        scope(ARGV + ["--transforms", "random_flip", "--input_no_transform", "True"])
    with pytest.raises(ValueError, match="--transport native"):
        scope(ARGV[:-2] + ["--transforms", "random_resized_crop"])              # the default transport is uint8
    with pytest.raises(ValueError, match="--synthetic"):
        scope(ARGV + ["--transforms", "random_flip", "--synthetic"])
    scope(ARGV + ["--transforms", "normalize", "--input_no_transform", "True"])  # nothing random: nothing to refuse
    with pytest.raises(SystemExit):
        FM.build_parser().parse_args(ARGV + ["--interpolation", "lanczos"])
    with pytest.raises(NotImplementedError, match="INTERPOLATION"):
        C.augment_from_cfg(NS(INPUT=NS(TRANSFORMS=["random_flip"], INTERPOLATION="nearest")))
    with pytest.raises(ValueError, match="RRCROP_SCALE"):
        C.augment_from_cfg(NS(INPUT=NS(TRANSFORMS=["random_resized_crop"], RRCROP_SCALE=(0.5, 0.2))))
    with pytest.raises(ValueError, match="RRCROP_SCALE"):
        C.AugmentCfg(crop=True, scale=(0.0, 1.0))


# ----------------------------------------------------------------------------------------------------- loader --
def _tree(tmp_path, **kw):
    base = D.write_synthetic_fairfedmed(str(tmp_path), sites=1, n_train=10, n_test=6, seed=2, **kw)
    mk = lambda train: D.FairFedMedDataset(base, 1, attribute_type="race", attributes=["race"],
                                           modality_type=kw.get("modality", "slo_fundus"), resolution=16, train=train)
    return mk(True), mk(False)


def test_training_loader_ships_ids_epoch_and_seed(tmp_path):
    tr, te = _tree(tmp_path, sizes=[12, 20, (24, 12), 16])
    aug = C.AugmentCfg(crop=True, flip=True)
    ld = D.FedLoader(tr, 4, True, seed=1003, transport="native", pin_memory=False, augment=aug)
    assert ld.augment == aug and ld.epoch == 0 and ld.seed == 1003 and len(ld) == 2
    twin = D.FedLoader(tr, 4, True, seed=1003, transport="native", pin_memory=False)
    seen = []
    for p in range(3):
        plain = list(twin)
        for k, b in enumerate(ld):
            nb = b["img"]
            assert isinstance(nb, D.NativeBatch) and nb.augment == aug and nb.start is None and nb.w is None and nb.T == 0
            assert nb.ids.dtype == torch.int32 and tuple(nb.ids.shape) == (4,) and nb.epoch == p and nb.seed == 1003
            assert nb.geom[:, 3].tolist() == [-1] * 4 and nb.max_extent == max(max(s) for s in nb.sizes)
            for j, i in enumerate(nb.ids.tolist()):                     # the ids are the dataset indices of the batch's samples
                raw = tr.raw(i, native=True)[0]
                off, h, w = nb.geom[j, :3].tolist()
                assert (h, w) == raw.shape[1:] and np.array_equal(nb.pix[off:off + h * w].numpy().reshape(h, w), raw[0])
            # the same order and labels as the loader without augmentation: only the image form differs
            assert torch.equal(b["label"], plain[k]["label"]) and torch.equal(b["attrs"], plain[k]["attrs"])
            seen.append(nb.ids.tolist())
        assert ld.epoch == p + 1
    ld.epoch = 7                                                        # settable: a resumed run continues its draws
    assert next(iter(ld))["img"].epoch == 7
    moved = next(iter(ld))["img"].to("cpu")
    assert moved.augment == aug and moved.ids is not None and moved.epoch == 7 and moved.seed == 1003


def test_test_loaders_never_augment(tmp_path):
    tr, te = _tree(tmp_path, sizes=[12, 20])
    aug = C.AugmentCfg(crop=True, flip=True)
    a = D.FedLoader(te, 3, False, transport="native", pin_memory=False, augment=aug)
    b = D.FedLoader(te, 3, False, transport="native", pin_memory=False)
    assert a.augment is None
    for x, y in zip(a, b):
        assert x["img"].augment is None and x["img"].ids is None and x["img"].T == y["img"].T > 0
        assert torch.equal(x["img"].pix, y["img"].pix) and torch.equal(x["img"].w, y["img"].w)
    u8 = D.FedLoader(te, 3, False, transport="uint8", pin_memory=False, augment=aug)       # any transport: untouched
    assert u8.augment is None and next(iter(u8))["img"].dtype == torch.float32
    inactive = D.FedLoader(tr, 3, True, transport="uint8", pin_memory=False, augment=C.AugmentCfg())
    assert inactive.augment is None


def test_fed_data_passes_the_setting_to_training_loaders_only(tmp_path):
    D.write_synthetic_fairfedmed(str(tmp_path), sites=2, n_train=6, n_test=4, seed=3, sizes=[12, 20])
    cfg = NS(SEED=3, INPUT=NS(SIZE=(16, 16), TRANSFORMS=["random_resized_crop", "normalize"], RRCROP_SCALE=(0.25, 1.0)),
             DATASET=NS(NAME="FairFedMed", ROOT=str(tmp_path), USERS=2, ATTRIBUTE_TYPE="race", ATTRIBUTES=["race"],
                        MODALITY_TYPE="slo_fundus"),
             DATALOADER=NS(TRAIN_X=NS(BATCH_SIZE=3)), TEST=NS(BATCH_SIZE=4))
    fd = D.FedData(cfg, transport="native")
    want = C.AugmentCfg(crop=True, scale=(0.25, 1.0))
    assert [fd.fed_train_loader_x_dict[k].augment for k in (0, 1)] == [want, want]
    assert [fd.fed_train_loader_x_dict[k].seed for k in (0, 1)] == [3000, 3001]
    assert [fd.fed_test_loader_x_dict[k].augment for k in (0, 1)] == [None, None]
    with pytest.raises(ValueError, match="--transport native"):
        D.FedData(cfg, transport="uint8")
    cfg.INPUT.TRANSFORMS = ["normalize"]
    plain = D.FedData(cfg, transport="uint8")
    assert plain.fed_train_loader_x_dict[0].augment is None


def test_loader_refusals_name_the_setting(tmp_path):
    aug = C.AugmentCfg(crop=True)
    tr, _ = _tree(tmp_path / "a", sizes=[12, 20])
    for transport in ("uint8", "float32"):
        with pytest.raises(ValueError, match="--transport native"):
            D.FedLoader(tr, 4, True, transport=transport, pin_memory=False, augment=aug)
    vol, _ = _tree(tmp_path / "b", sizes=[8], modality="oct_bscans_3d")
    with pytest.raises(ValueError, match="oct_bscans_3d"):
        D.FedLoader(vol, 2, True, transport="native", pin_memory=False, augment=aug)
    tr.resolution = 18                                                  # INPUT.SIZE % 4 != 0
    with pytest.raises(ValueError, match="INPUT.SIZE"):
        D.FedLoader(tr, 4, True, transport="native", pin_memory=False, augment=aug)
    tr.resolution = 16

    class Floats:                                                       # a reader whose stored samples are not uint8
        resolution, modality_type = 16, "slo_fundus"

        def __len__(self):
            return 4

        def raw(self, item, native=False):
            return np.zeros((1, 12, 12), np.float32), 3, 0, [0]

    with pytest.raises(TypeError, match="not uint8"):
        next(iter(D.FedLoader(Floats(), 2, True, transport="native", pin_memory=False, augment=aug)))

    class Wide(Floats):                                                 # 16 * 40 pixels to 16 under the cubic: 161 taps
        def raw(self, item, native=False):
            return np.zeros((1, 4, 640), np.uint8), 3, 0, [0]

    with pytest.raises(ValueError, match="INTERPOLATION bicubic needs more filter taps"):
        next(iter(D.FedLoader(Wide(), 2, True, transport="native", pin_memory=False, augment=C.AugmentCfg(crop=True, filter="bicubic"))))
    assert D.augment_refusal(aug, 16, [(4, 400)]) is None               # the triangle at 25x: 51 taps


# ------------------------------------------------------------------------------------------------ entry points --
def test_entry_point_argument_checks_need_no_gpu():
    lib = _lib.load()
    i32 = lambda n: (ctypes.c_int32 * n)()
    geom, ids, bx = i32(4), i32(1), i32(8)
    rng = lambda *v: (ctypes.c_double * 4)(*v)
    ok = rng(0.08, 1.0, 0.75, 4.0 / 3.0)
    call = lambda g=geom, i=ids, B=1, r=ok, b=bx, epoch=0: lib.ffm_augment_boxes(g, i, B, 5, epoch, 1, 1, r, b, None)
    assert call(g=None) == call(i=None) == call(r=None) == call(b=None) == call(B=0) == call(epoch=-1) == -1
    for bad in ((0.0, 1.0, 0.75, 1.33), (0.5, 0.2, 0.75, 1.33), (0.08, 1.5, 0.75, 1.33), (0.08, 1.0, 0.0, 1.33),
                (0.08, 1.0, 1.5, 0.75), (float("nan"), 1.0, 0.75, 1.33), (0.08, 1.0, 0.75, float("inf"))):
        assert call(r=rng(*bad)) == -1, bad
    pix, dst = (ctypes.c_uint8 * 16)(), (ctypes.c_float * 64)()
    dst_p = ctypes.c_void_p((ctypes.addressof(dst) + 15) & ~15)
    crop = lambda p=pix, g=geom, b=bx, d=dst_p, B=1, C1=1, rep=1, R=4, f=0, n=4: \
        lib.ffm_crop_resize_u8(p, g, b, d, B, C1, rep, R, f, n, None)
    assert crop(p=None) == crop(g=None) == crop(b=None) == crop(d=None) == -1
    assert crop(B=0) == crop(C1=0) == crop(rep=0) == crop(R=0) == crop(n=0) == crop(f=2) == crop(f=-1) == -1
    assert crop(d=ctypes.c_void_p(dst_p.value + 4)) == -1               # dst: 16-byte stores
    assert crop(R=6) == -2                                              # R % 4
    assert crop(R=4, n=4 * 33, f=0) == -2 and crop(R=4, n=4 * 17, f=1) == -2        # beyond the tap limit: nothing launched
    # the limit and its query: the table width is 2 ceil(S max(1, n / R)) + 1
    T = lib.ffm_augment_taps
    assert T(224, 224, 0) == 3 and T(224, 224, 1) == 5 and T(100, 224, 1) == 5
    assert T(664, 224, 0) == 2 * math.ceil(664 / 224) + 1 == 7 and T(664, 224, 1) == 2 * math.ceil(2 * 664 / 224) + 1 == 13
    assert T(2000, 224, 1) == 37 and T(3472, 224, 1) == 63 and T(3473, 224, 1) == -2
    assert T(31 * 4, 4, 0) == 63 and T(32 * 4, 4, 0) == -2                                # FFM_AUGMENT_MAX_TAPS = 64
    assert T(3 * 1024, 1024, 1) == 13 and T(4 * 1024, 1024, 1) == -2                     # FFM_AUGMENT_MAX_LDS: 1152 x 18 x 4 bytes
    assert T(0, 224, 0) == T(224, 0, 0) == T(224, 224, 2) == -1
    assert all(T(n, 224, f) <= T(n + 1, 224, f) for f in (0, 1) for n in range(1, 3300, 7))
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffm_hip.h")).read()
    assert "#define FFM_AUGMENT_MAX_TAPS 64" in hdr and "#define FFM_AUGMENT_MAX_LDS 65536" in hdr
    assert _lib.FILTERS == {"bilinear": 0, "bicubic": 1} and "#define FFM_FILTER_BICUBIC 1" in hdr
    # every tap run of the restatement fits the width the library reserves for it
    for n, R in ((41, 32), (9, 32), (475, 224), (664, 224), (1, 32)):
        for f, name in enumerate(("bilinear", "bicubic")):
            assert A.taps(n, R, name)[1].shape[1] <= T(n, R, f), (n, R, name)


def test_ops_refuse_host_tensors():
    from fairfedmed_amd import ops
    nb = D.NativeBatch.augmented([np.zeros((1, 8, 8), np.uint8)], 3, 8, [0], 0, 1, C.AugmentCfg(flip=True))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.augment_u8(nb, torch.empty(1, 3, 8, 8))
    plain = D.NativeBatch.from_planes([np.zeros((1, 8, 8), np.uint8)], 3, 8)
    with pytest.raises(ValueError, match="carries ids"):
        ops.augment_u8(plain, torch.empty(1, 3, 8, 8))
    assert ops.augment_taps(664, 224, "bicubic") == 13
