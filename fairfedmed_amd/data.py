"""Data formats on the input side of the hot path.

Readers for the two benchmarks' on-disk layouts, mirroring ``FairFedMedDataset`` / ``FedChexMimicDataset``
(utils/data_utils.py:559-790) and the loader surface the trainer consumes
(Dassl/dassl/data/data_manager.py:20-59, 104-133, 435-502):

    <root>/fairfedmed/all/<file>.npz            slo_fundus u8 [H,W] | oct_bscans u8 [128,H,W], glaucoma, race, gender, ...
    <root>/fairfedmed/meta_site{k}_{attr}_{train|test}.csv      column 'filename'
    <root>/fedchexmimic/meta_{chexpert|mimic}_{attr}_{train|test}.csv   filename, disease_label, <attr>_label columns

``__getitem__`` returns what the reference returns: (float32 [C,H,W] raw 0..255, label int64, attrs int64 [n_attr]).
``raw(item)`` returns the same sample in its TRANSPORT form: uint8, before the float conversion and the channel
repeat (1 channel for SLO fundus / chest X-ray), 12x fewer bytes over PCIe; the engine expands it on the GPU
(``ffm_expand_u8``), bit-identically, because uint8 -> float32 is exact.  ``raw(item, native=True)`` is the stored uint8
sample BEFORE the resize: transport="native" ships a ragged ``NativeBatch`` of those with the tap tables of ``resize_taps`` and
the engine resizes on the GPU (``ffm_resize_u8``).

scikit-image is not in this image: ``resize_image`` restates ``skimage.transform.resize`` (order 1, mode 'reflect',
no anti-aliasing when enlarging, clip to the input range) on scipy.ndimage.zoom - parity for the resize branch is
unpinned; the branches without a resize - both readers, FairFedMedDataset and FedChexMimicDataset, with their
count_by_attribute - are pinned against the imported reference (tests/golden/make_golden.py -> dataset.json).
"""
from __future__ import annotations

import csv
import os
from types import SimpleNamespace as NS
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

CLASSNAMES = {"FairFedMed": ["NOT Glaucoma", "Glaucoma"],                        # datasets/FairFedMed.py:47-48
              "FedChexMimic": ["NOT Pleural Effusion", "Pleural Effusion"]}      # datasets/FedChexMimic.py:47-48
DATASET_DIRS = {"FairFedMed": "fairfedmed", "FedChexMimic": "fedchexmimic"}
_FILTERED = {"gender", "maritalstatus", "hispanic", "language", "ethnicity", "race"}   # utils/data_utils.py:582


def resize_image(img: np.ndarray, shape) -> np.ndarray:
    """skimage.transform.resize(img, shape) for a 2-D float image (defaults: order 1, mode='reflect', clip=True,
    anti-aliasing Gaussian with sigma = (in/out - 1) / 2 when an axis shrinks), restated on scipy.ndimage because
    scikit-image is not installable here; pinned by tests/test_data_cpu.py against values worked out by hand from the
    published algorithm and against a loop-level implementation of it that shares no code with this one."""
    from scipy import ndimage as ndi
    img = np.asarray(img)
    out_dtype = img.dtype if img.dtype.kind == "f" else np.float64
    src = img.astype(np.float64)
    factors = [o / i for o, i in zip(shape, img.shape)]
    if any(f < 1 for f in factors):                       # anti-aliasing filter when shrinking (skimage default)
        sigma = [max(0.0, (1 / f - 1) / 2) for f in factors]
        src = ndi.gaussian_filter(src, sigma, mode="mirror")
    out = ndi.zoom(src, factors, order=1, mode="mirror", grid_mode=True)
    out = np.clip(out, img.min(), img.max())
    return out.astype(out_dtype)


def _mirror(i: np.ndarray, n: int) -> np.ndarray:
    """scipy.ndimage's 'mirror' for integer indices: reflection about the centre of the edge sample, period 2n - 2."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


_TAPS: Dict[tuple, tuple] = {}
NATIVE_MAX_TAPS = 32                                      # FFM_RESIZE_MAX_TAPS (include/ffm_hip.h)


def resize_taps(n_in: int, n_out: int):
    """One axis of ``resize_image`` as a matrix A [n_out, n_in], float64, in its sparse form: (start int32 [n_out],
    w float64 [n_out, T]) with A[o, start[o] + t] = w[o, t] and zero elsewhere, start[o] + T <= n_in.

    A = Z G.  G [n_in, n_in] is ndimage.gaussian_filter1d(sigma = (n_in / n_out - 1) / 2, truncate 4, mode 'mirror') when the
    axis shrinks, else the identity.  Z [n_out, n_in] is ndimage.zoom(order 1, grid_mode=True, mode 'mirror'): output o
    reads the source coordinate (o + 1/2) n_in / n_out - 1/2, reflected into [0, n_in - 1] about the centres of the edge
    samples, and interpolates linearly between its two neighbours.  Rows sum to 1, weights are >= 0, the non-zeros of a
    row are one contiguous run (T = 1 for n_in == n_out: the identity; 2 when enlarging).  Cached per (n_in, n_out)."""
    key = (int(n_in), int(n_out))
    if key in _TAPS:
        return _TAPS[key]
    n, R = key
    if n < 1 or R < 1:
        raise ValueError(f"resize_taps({n_in}, {n_out})")
    G = np.eye(n)
    f = R / n
    if f < 1:
        sigma = max(0.0, (1 / f - 1) / 2)
        if sigma > 1e-15:
            lw = int(4.0 * sigma + 0.5)
            k = np.arange(-lw, lw + 1)
            phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
            phi /= phi.sum()
            G = np.zeros((n, n))
            rows = np.repeat(np.arange(n), k.size)
            np.add.at(G, (rows, _mirror(rows + np.tile(k, n), n)), np.tile(phi, n))
    Z = np.zeros((R, n))
    if n == 1:
        Z[:, 0] = 1.0
    else:
        cc = (np.arange(R) + 0.5) * (n / R) - 0.5
        p = 2.0 * (n - 1)
        cc = np.mod(cc, p)
        cc = np.where(cc > n - 1, p - cc, cc)                          # 'mirror' of the coordinate itself
        i0 = np.floor(cc).astype(np.int64)
        t = cc - i0
        o = np.arange(R)
        np.add.at(Z, (o, _mirror(i0, n)), 1.0 - t)
        np.add.at(Z, (o, _mirror(i0 + 1, n)), t)
    A = Z @ G
    nz = A > 0
    first = nz.argmax(1)
    last = n - 1 - nz[:, ::-1].argmax(1)
    T = int((last - first + 1).max())
    start = np.minimum(first, n - T).astype(np.int32)
    w = np.ascontiguousarray(A[np.arange(R)[:, None], start[:, None] + np.arange(T)[None, :]])
    start.setflags(write=False)
    w.setflags(write=False)
    _TAPS[key] = (start, w)
    return _TAPS[key]


class NativeBatch:
    """A ragged batch of stored uint8 samples and the resize that makes it a [B, C1 * rep, R, R] float32 batch on the GPU
    (ffm_resize_u8 through ops.resize_u8; the engines accept it where they accept an image tensor).

        pix    uint8 [bytes]          all planes of all images back to back; image b is [C1, H_b, W_b]
        geom   int32 [B, 4]           byte offset in pix, H_b, W_b, table id
        start  int32 [NG * 2 * R]     per distinct (H, W) of the batch and axis (0: rows over H, 1: columns over W)
        w      fp32  [NG, 2, R, T]    resize_taps of that axis, zero-padded to the batch's widest run T
        C1, rep, R, T                 planes per image, channel repeat, output size, taps
        sizes                         ((H_b, W_b), ...) on the host (checks without a device read)"""

    def __init__(self, pix, geom, start, w, C1: int, rep: int, R: int, sizes, ids=None, epoch: int = 0, seed: int = 0,
                 augment=None):
        self.pix, self.geom, self.start, self.w = pix, geom, start, w
        self.C1, self.rep, self.R, self.sizes = int(C1), int(rep), int(R), tuple(sizes)
        self.T = 0 if w is None else int(w.shape[-1])
        # train-time augmentation (section 4.20): the samples' dataset indices (int32 [B]), the loader's pass count and seed
        # and the config.AugmentCfg; such a batch carries no tap tables (start and w are None) and is resampled by
        # ops.augment_u8, every sample from a box of its own
        self.ids, self.epoch, self.seed, self.augment = ids, int(epoch), int(seed), augment

    @classmethod
    def from_planes(cls, samples: Sequence[np.ndarray], rep: int, R: int, tables: bool = True) -> "NativeBatch":
        """samples: uint8 arrays [C1, H_b, W_b].  A sample with H_b == R is one the readers do not resize (the decision is
        the readers' own, by height alone), so its width must be R as well: the ValueError an engine gives such a batch.
        tables=False: bytes and geometry alone (the form `augmented` takes; table id -1)."""
        C1 = samples[0].shape[0]
        ids: Dict[tuple, int] = {}
        geom, off = [], 0
        for s in samples:
            if s.dtype != np.uint8 or s.ndim != 3 or s.shape[0] != C1:
                raise TypeError("NativeBatch takes uint8 samples [C1, H, W] with one C1")
            h, wd = s.shape[1:]
            if tables and h == R and wd != R:
                raise ValueError(f"expected [B,{C1 * rep},{R},{R}], got {(1, C1 * rep, h, wd)}")
            geom.append([off, h, wd, ids.setdefault((h, wd), len(ids)) if tables else -1])
            off += s.size
        if off >= 2 ** 31:
            raise ValueError("a NativeBatch holds less than 2 GiB of pixels")
        if not tables:
            pix = np.concatenate([np.ascontiguousarray(s).reshape(-1) for s in samples])
            return cls(torch.from_numpy(pix), torch.tensor(geom, dtype=torch.int32), None, None, C1, rep, R,
                       [(g[1], g[2]) for g in geom])
        taps = [(resize_taps(h, R), resize_taps(wd, R)) for h, wd in ids]
        T = max(t[1].shape[1] for pair in taps for t in pair)
        start = np.zeros((len(taps), 2, R), np.int32)
        w = np.zeros((len(taps), 2, R, T), np.float32)
        for g, pair in enumerate(taps):
            for ax, (st, wt) in enumerate(pair):
                start[g, ax] = st
                w[g, ax, :, :wt.shape[1]] = wt
        pix = np.concatenate([np.ascontiguousarray(s).reshape(-1) for s in samples])
        return cls(torch.from_numpy(pix), torch.tensor(geom, dtype=torch.int32), torch.from_numpy(start.reshape(-1)),
                   torch.from_numpy(w), C1, rep, R, [(g[1], g[2]) for g in geom])

    def __len__(self):
        return self.geom.shape[0]

    @property
    def device(self):
        return self.pix.device

    @property
    def is_cuda(self):
        return self.pix.is_cuda

    @classmethod
    def augmented(cls, samples: Sequence[np.ndarray], rep: int, R: int, ids, epoch: int, seed: int, augment) -> "NativeBatch":
        """The batch a training loader with augmentation ships: stored bytes, geometry, and what keys the draws."""
        nb = cls.from_planes(samples, rep, R, tables=False)
        if len(ids) != len(samples):
            raise ValueError("one dataset index per sample")
        nb.ids = torch.as_tensor(np.asarray(ids, dtype=np.int64).astype(np.int32))
        nb.epoch, nb.seed, nb.augment = int(epoch), int(seed), augment
        return nb

    @property
    def max_extent(self) -> int:
        """The largest stored height or width of the batch: what sizes ffm_crop_resize_u8's tap tables."""
        return max(max(h, w) for h, w in self.sizes)

    def _map(self, fn) -> "NativeBatch":
        opt = lambda t: None if t is None else fn(t)
        return NativeBatch(fn(self.pix), fn(self.geom), opt(self.start), opt(self.w), self.C1, self.rep, self.R, self.sizes,
                           opt(self.ids), self.epoch, self.seed, self.augment)

    def to(self, device, non_blocking: bool = False) -> "NativeBatch":
        return self._map(lambda t: t.to(device, non_blocking=non_blocking))

    def pin_memory(self) -> "NativeBatch":
        return self._map(lambda t: t.pin_memory())

    def supported(self) -> bool:
        """Whether ffm_resize_u8 serves this batch (else it answers FFM_EUNSUP and the loader resizes on the host)."""
        return self.R % 4 == 0 and self.T <= NATIVE_MAX_TAPS


def augment_refusal(augment, R: int, sizes) -> Optional[str]:
    """Why ffm_crop_resize_u8 does not serve these stored sizes at output size R under `augment`, or None when it does."""
    from . import _lib
    if R % 4:
        return f"INPUT.SIZE {R} is not a multiple of 4 (the kernel stores 16 bytes at a time): change INPUT.SIZE"
    n = max(max(h, w) for h, w in sizes)
    if _lib.load().ffm_augment_taps(int(n), int(R), _lib.FILTERS[augment.filter]) < 0:
        return (f"a stored extent of {n} pixels resampled to INPUT.SIZE {R} with INPUT.INTERPOLATION {augment.filter} needs more "
                f"filter taps than the kernel tabulates: store smaller images, raise INPUT.SIZE"
                + (" or set INPUT.INTERPOLATION bilinear" if augment.filter != "bilinear" else ""))
    return None


def _read_csv(path: str) -> Dict[str, list]:
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    if not rows or "filename" not in rows[0]:
        raise AssertionError("filename must be included in the head")
    return {k: [r[k] for r in rows] for k in rows[0]}


class FairFedMedDataset:
    """utils/data_utils.py:559-726 for the modalities the FairLoRA scripts use."""

    def __init__(self, base_path, site, attribute_type=None, attributes=None, modality_type=None, resolution=224,
                 depth=3, train=True, transform=None):
        self.task = "cls"
        self.base_path, self.data_path = base_path, os.path.join(base_path, "all")
        self.modality_type, self.attribute_type, self.attributes = modality_type, attribute_type, attributes
        split = "train" if train else "test"
        files = _read_csv(os.path.join(base_path, f"meta_site{site}_{attribute_type}_{split}.csv"))["filename"]
        if modality_type is None:
            raise AssertionError("modality_type")
        if modality_type not in ("oct_bscans", "oct_bscans_3d", "slo_fundus"):
            raise NotImplementedError(modality_type)
        key = "oct_bscans" if modality_type.startswith("oct") else "slo_fundus"
        self.data_files, self.data_attrs = [], []
        for x in files:
            with np.load(os.path.join(self.data_path, x), allow_pickle=True) as raw:
                attr = raw[attribute_type].item()
                if attribute_type in _FILTERED and not attr > -1:      # -1 = unknown: dropped (:586)
                    continue
                if len(raw[key]) > 0:
                    self.data_files.append(x)
                    self.data_attrs.append(attr)
        self.depth, self.resolution, self.transform = depth, resolution, transform

    def __len__(self):
        return len(self.data_files)

    def _load(self, item):
        return np.load(os.path.join(self.data_path, self.data_files[item]), allow_pickle=True)

    def _meta(self, raw):
        label = int(float(raw["glaucoma"].item()))
        attrs = [int(raw[k]) for k in self.attributes] if (self.attribute_type is not None and self.attributes) else []
        return label, attrs

    def raw(self, item, native: bool = False):
        """(image in transport form [C1,H,W], channel repeat, label, attrs); uint8 when the file holds uint8 and no
        resize is needed, else float32.  native=True: a uint8 sample is returned at its stored size, unresized."""
        with self._load(item) as raw:
            label, attrs = self._meta(raw)
            if self.modality_type == "slo_fundus":
                img = np.transpose(raw["slo_fundus"])[None, :, :]
                rep = self.depth if self.depth > 1 else 1
            elif self.modality_type == "oct_bscans":
                img, rep = raw["oct_bscans"][::4], 1                   # 128 -> 32 B-scans (:639)
            else:                                                      # oct_bscans_3d: [1, D, H, W] volume
                img, rep = raw["oct_bscans"][None], 1
        if native and self.modality_type != "oct_bscans_3d" and img.dtype == np.uint8:
            return np.ascontiguousarray(img), rep, label, attrs
        if self.modality_type != "oct_bscans_3d" and img.shape[1] != self.resolution:
            img = np.stack([resize_image(s.astype(np.float32), (self.resolution, self.resolution)) for s in img])
        if img.dtype != np.uint8:
            img = img.astype(np.float32) if self.modality_type != "oct_bscans_3d" else img.astype(int).astype(np.float32)
        return np.ascontiguousarray(img), rep, label, attrs

    def __getitem__(self, item):
        img, rep, label, attrs = self.raw(item)
        data = img.astype(np.float32)
        if rep > 1:
            data = np.repeat(data, rep, axis=0)
        if self.transform is not None and self.modality_type != "slo_fundus":
            data = self.transform(data)
        return data, torch.tensor(label).long(), torch.tensor(attrs)

    def count_by_attribute(self, attr: str) -> List[int]:
        """Dassl/dassl/data/data_manager.py:443-460: samples per group id 0..max."""
        vals = []
        for item in range(len(self)):
            with self._load(item) as raw:
                vals.append(int(raw[attr]))
        return [vals.count(g) for g in range(max(vals) + 1)]


class FedChexMimicDataset:
    """utils/data_utils.py:729-790: gray-scale chest X-rays (jpg) listed in a csv with label columns."""

    def __init__(self, base_path, site, attribute_type, attributes, modality_type=None, resolution=224, depth=3,
                 train=True, transform=None):
        self.task = "cls"
        self.base_path = base_path
        if site == 1:
            name, self.data_path = "chexpert", base_path
        elif site == 2:
            name, self.data_path = "mimic", os.path.join(base_path, "files_336p")
        else:
            raise NotImplementedError(site)
        self.modality_type, self.attribute_type, self.attributes = modality_type, attribute_type, attributes
        cols = _read_csv(os.path.join(base_path, f"meta_{name}_{attribute_type}_{'train' if train else 'test'}.csv"))
        self.data_files = cols["filename"]
        self.data_attrs = [int(v) for v in cols[attribute_type + "_label"]]
        self.disease_labels = [int(v) for v in cols["disease_label"]]
        self.data_attributes = [[int(v) for v in cols[k + "_label"]] for k in attributes]
        self.depth, self.resolution, self.transform = depth, resolution, transform

    def __len__(self):
        return len(self.data_files)

    def raw(self, item, native: bool = False):
        from PIL import Image
        img = np.array(Image.open(os.path.join(self.data_path, self.data_files[item])).convert("L"))[None, :, :]
        if img.shape[1] != self.resolution and not (native and img.dtype == np.uint8):
            img = np.stack([resize_image(s.astype(np.float32), (self.resolution, self.resolution)) for s in img])
        attrs = [a[item] for a in self.data_attributes]
        return np.ascontiguousarray(img), (self.depth if self.depth > 1 else 1), self.disease_labels[item], attrs

    def __getitem__(self, item):
        img, rep, label, attrs = self.raw(item)
        data = img.astype(np.float32)
        if rep > 1:
            data = np.repeat(data, rep, axis=0)
        return data, torch.tensor(label).long(), torch.tensor(attrs)

    def count_by_attribute(self, attr: str) -> List[int]:
        """Dassl/dassl/data/data_manager.py:462-473."""
        vals = self.data_attributes[list(self.attributes).index(attr)]
        return [vals.count(g) for g in range(max(vals) + 1)]


class FedLoader:
    """The DataLoader the trainer iterates (build_data_loader, data_manager.py:20-59): random order and drop_last for
    training, sequential for testing, batches in the dict contract {"img", "label", "attrs"}.

    transport="uint8" ships the sample's transport form when it is uint8 (``img`` is then uint8 [B,C1,H,W] and the
    engine expands / repeats the channels on the GPU); "float32" ships what the reference ships; "native" ships the
    stored uint8 samples at their stored sizes as a ``NativeBatch`` (``img`` has len() = B and .to() / .pin_memory(), no
    shape) and the engine resizes them on the GPU - a batch with a sample that is not uint8, or one ffm_resize_u8 does not
    serve, is resized on the host and shipped as float32; the 3D volumes are never resized and go as uint8.  Batches are
    assembled in pinned memory so that the trainer's ``.to(device, non_blocking=True)`` is an asynchronous copy.

    augment=config.AugmentCfg (INPUT.TRANSFORMS; training loaders only, transport "native"): every batch is a ``NativeBatch`` that
    carries ``ids`` (the dataset indices of its samples), ``epoch`` (the passes this loader has completed) and ``seed`` (this
    loader's) and no tap tables, and the engine crops, resamples and flips it on the GPU.  What
    cannot be augmented raises here, naming the setting to change; nothing is shipped un-augmented."""

    def __init__(self, dataset, batch_size: int, train: bool, seed: int = 0, transport: str = "float32",
                 pin_memory: Optional[bool] = None, augment=None):
        assert transport in ("float32", "uint8", "native")
        self.dataset, self.batch_size, self.train, self.transport = dataset, batch_size, train, transport
        # augment (config.AugmentCfg): training loaders only - a test loader never augments.  Its batches are NativeBatches
        # that carry ids / epoch / seed and no tap tables; what cannot be augmented is refused, never shipped un-augmented
        self.augment = augment if (train and augment is not None and augment.active) else None
        self.seed, self.epoch = int(seed), 0                          # epoch: passes completed (settable)
        if self.augment is not None:
            if transport != "native":
                raise ValueError(f"INPUT.TRANSFORMS run on the stored bytes: set --transport native (got {transport!r})")
            if getattr(dataset, "modality_type", None) == "oct_bscans_3d":
                raise ValueError("INPUT.TRANSFORMS: DATASET.MODALITY_TYPE oct_bscans_3d volumes are not augmented; choose "
                                 "another modality or drop the random transforms (--transforms normalize)")
            if dataset.resolution % 4:
                raise ValueError(augment_refusal(self.augment, dataset.resolution, [(1, 1)]))
        self.drop_last = train and len(dataset) >= batch_size
        self.gen = np.random.default_rng(seed)
        self.pin = torch.cuda.is_available() if pin_memory is None else pin_memory
        assert len(self) > 0

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _collate(self, idx: Sequence[int]) -> Dict[str, torch.Tensor]:
        native = self.transport == "native" and getattr(self.dataset, "modality_type", None) != "oct_bscans_3d"
        samples = [self.dataset.raw(int(i), native=True) if native else self.dataset.raw(int(i)) for i in idx]
        img = None
        if self.augment is not None:
            if not all(s[0].dtype == np.uint8 for s in samples):
                raise TypeError("INPUT.TRANSFORMS: a stored sample is not uint8 and cannot be augmented on the GPU; store uint8 "
                                "samples or drop the random transforms (--transforms normalize)")
            why = augment_refusal(self.augment, self.dataset.resolution, [s[0].shape[1:] for s in samples])
            if why:
                raise ValueError("INPUT.TRANSFORMS: " + why)
            img = NativeBatch.augmented([s[0] for s in samples], samples[0][1], self.dataset.resolution, idx, self.epoch,
                                        self.seed, self.augment)
        elif native and all(s[0].dtype == np.uint8 for s in samples):
            nb = NativeBatch.from_planes([s[0] for s in samples], samples[0][1], self.dataset.resolution)
            img = nb if nb.supported() else None
        if native and img is None:                                     # this batch takes the host resize
            samples = [self.dataset.raw(int(i)) for i in idx]
        if img is None:
            imgs = []
            for im, rep, _, _ in samples:
                if self.transport == "float32" or native or im.dtype != np.uint8:
                    im = im.astype(np.float32)
                    if rep > 1:
                        im = np.repeat(im, rep, axis=0)
                imgs.append(im)
            img = torch.from_numpy(np.stack(imgs))
        out = {"img": img, "label": torch.tensor([s[2] for s in samples], dtype=torch.int64),
               "attrs": torch.tensor([s[3] for s in samples], dtype=torch.int64).reshape(len(idx), -1)}
        if self.pin:
            out = {k: v.pin_memory() for k, v in out.items()}
        return out

    def __iter__(self):
        n = len(self.dataset)
        order = self.gen.permutation(n) if self.train else np.arange(n)
        for b in range(len(self)):
            yield self._collate(order[b * self.batch_size:(b + 1) * self.batch_size])
        self.epoch += 1


class FedData:
    """What ``GLP_OT_SVLoRA(cfg, data=...)`` needs from the reference's DataManager: per-client loaders, class names."""

    def __init__(self, cfg, transport: str = "float32"):
        from .config import augment_from_cfg
        augment = augment_from_cfg(cfg)               # INPUT.TRANSFORMS: the training loaders augment, the test loaders never
        name = cfg.DATASET.NAME
        if name not in DATASET_DIRS:
            raise NotImplementedError(name)
        root = os.path.join(os.path.abspath(os.path.expanduser(cfg.DATASET.ROOT)), DATASET_DIRS[name])
        cls = FairFedMedDataset if name == "FairFedMed" else FedChexMimicDataset
        kw = dict(attribute_type=cfg.DATASET.ATTRIBUTE_TYPE, attributes=list(cfg.DATASET.ATTRIBUTES),
                  modality_type=getattr(cfg.DATASET, "MODALITY_TYPE", None), resolution=cfg.INPUT.SIZE[0], depth=3)
        self.fed_train_loader_x_dict, self.fed_test_loader_x_dict = {}, {}
        seed = getattr(cfg, "SEED", 1)
        for net_id in range(cfg.DATASET.USERS):
            tr = cls(root, net_id + 1, train=True, **kw)
            te = cls(root, net_id + 1, train=False, **kw)
            self.fed_train_loader_x_dict[net_id] = FedLoader(tr, cfg.DATALOADER.TRAIN_X.BATCH_SIZE, True,
                                                             seed=seed * 1000 + net_id, transport=transport,
                                                             augment=augment)
            self.fed_test_loader_x_dict[net_id] = FedLoader(te, cfg.TEST.BATCH_SIZE, False, transport=transport)
        self.classnames = list(CLASSNAMES[name])
        self.dataset = NS(classnames=self.classnames)
        self.num_classes = len(self.classnames)
        self.lab2cname = {i: n for i, n in enumerate(self.classnames)}


# ------------------------------------------------------------------------------------------------ synthetic files --
def write_synthetic_fairfedmed(root: str, sites: int = 2, n_train: int = 12, n_test: int = 6, size: int = 224,
                               seed: int = 0, modality: str = "slo_fundus", attribute_type: str = "race",
                               unknown_every: int = 0, sizes: Optional[Sequence] = None) -> str:
    """A FairFedMed tree of random uint8 samples (tests, input-path benchmark).  Returns <root>/fairfedmed.
    sizes: stored sizes taken in turn, sample k gets sizes[k % len(sizes)], each an int or a pair (rows, columns) of the stored
    array; None writes every sample size x size."""
    g = np.random.Generator(np.random.Philox(key=[0xDA7A, seed & 0xFFFFFFFF]))
    base = os.path.join(root, DATASET_DIRS["FairFedMed"])
    os.makedirs(os.path.join(base, "all"), exist_ok=True)
    k = 0
    for site in range(1, sites + 1):
        for split, n in (("train", n_train), ("test", n_test)):
            names = []
            for _ in range(n):
                name = f"data_{k:05d}.npz"
                arrs = {"glaucoma": np.array(int(g.integers(0, 2))), "race": np.array(int(g.integers(0, 3))),
                        "gender": np.array(int(g.integers(0, 2))), "ethnicity": np.array(int(g.integers(0, 2))),
                        "language": np.array(int(g.integers(0, 3)))}
                if unknown_every and k % unknown_every == unknown_every - 1:
                    arrs[attribute_type] = np.array(-1)
                hw = sizes[k % len(sizes)] if sizes else size
                hw = (hw, hw) if np.isscalar(hw) else tuple(hw)
                if modality == "slo_fundus":
                    arrs["slo_fundus"] = g.integers(0, 256, size=hw, dtype=np.uint8)
                    arrs["oct_bscans"] = np.zeros((0,), np.uint8)
                else:
                    arrs["oct_bscans"] = g.integers(0, 256, size=(128,) + hw, dtype=np.uint8)
                    arrs["slo_fundus"] = np.zeros((0,), np.uint8)
                np.savez(os.path.join(base, "all", name), **arrs)
                names.append(name)
                k += 1
            with open(os.path.join(base, f"meta_site{site}_{attribute_type}_{split}.csv"), "w", newline="") as f:
                w = csv.writer(f)
                w.writerow(["filename"])
                w.writerows([[x] for x in names])
    return base


def write_synthetic_fedchexmimic(root: str, n_train: int = 12, n_test: int = 6, size: int = 224, seed: int = 0,
                                 attribute_type: str = "gender") -> str:
    """A FedChexMimic tree (utils/data_utils.py:729-753): site 1 "chexpert" with its images under the base path, site 2
    "mimic" under <base>/files_336p; csv columns filename, disease_label, gender_label, race_label.  The images alternate
    between 8-bit gray PNG, RGB JPEG and RGB PNG, so that the reader's ``convert('L')`` sees all three.  Returns
    <root>/fedchexmimic."""
    from PIL import Image
    g = np.random.Generator(np.random.Philox(key=[0xC4E5, seed & 0xFFFFFFFF]))
    base = os.path.join(root, DATASET_DIRS["FedChexMimic"])
    k = 0
    for name, sub in (("chexpert", "."), ("mimic", "files_336p")):
        for split, n in (("train", n_train), ("test", n_test)):
            rows = []
            for _ in range(n):
                kind = k % 3
                rel = os.path.join("imgs" if name == "chexpert" else "p10", f"view_{k:05d}." + ("jpg" if kind == 1 else "png"))
                path = os.path.join(base, sub, rel)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                if kind == 0:
                    Image.fromarray(g.integers(0, 256, size=(size, size), dtype=np.uint8), "L").save(path)
                else:
                    # smooth RGB content (a JPEG of white noise is all quantisation error)
                    low = g.integers(0, 256, size=(size // 4 + 1, size // 4 + 1, 3), dtype=np.uint8)
                    arr = np.kron(low, np.ones((4, 4, 1), np.uint8))[:size, :size]
                    Image.fromarray(arr, "RGB").save(path, **({"quality": 90} if kind == 1 else {}))
                rows.append([rel, int(g.integers(0, 2)), int(g.integers(0, 2)), int(g.integers(0, 3))])
                k += 1
            with open(os.path.join(base, f"meta_{name}_{attribute_type}_{split}.csv"), "w", newline="") as f:
                w = csv.writer(f)
                w.writerow(["filename", "disease_label", "gender_label", "race_label"])
                w.writerows(rows)
    return base
