"""get_loader(cfg, seed) -> (sup, unsup, val) or (sup, val) loaders
(reference: u2pl/dataset/builder.py:9-43, cityscapes.py, pascal_voc.py, base.py, augmentation.py)."""
import copy
import math
import os
import random

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

TOTAL_TRAIN = {"cityscapes": 2975, "pascal": 10582}   # cityscapes.py:116, pascal_voc.py:109


def parse_list(path):
    """base.py:12-35: naming scheme is picked from the LIST PATH."""
    lines = [l.strip() for l in open(path) if l.strip()]
    if "cityscapes" in path:
        return [(l, "gtFine/" + l[12:-15] + "gtFine_labelTrainIds.png") for l in lines], "cityscapes"
    if "pascal" in path or "VOC" in path:
        return [(f"JPEGImages/{l}.jpg", f"SegmentationClassAug/{l}.png") for l in lines], "pascal"
    raise ValueError("unknown dataset list: " + path)


def parse_pairs(path):
    """paired list (dataset.type `pairs` / `pairs_semi`): one sample per line, `image_path [label_path]`, whitespace
    separated, relative to data_root; a line with one field has no label (-> None: its label array is all ignore_label)"""
    out = []
    for l in open(path):
        f = l.split()
        if not f:
            continue
        if len(f) > 2:
            raise ValueError(f"{path}: expected `image_path [label_path]`, got {l.strip()!r}")
        out.append((f[0], f[1] if len(f) == 2 else None))
    return out


def label_tables(cfg_dataset, num_classes):
    """dataset.label_map -> (lut uint8[256], bad bool[256] or None).  lut: raw label byte -> class index or ignore_label
    (build_label_lut's rules).  bad marks the raw values that are neither mapped to a class (or listed in `table`) nor the
    ignore value -- what `other: error` refuses on the host; None with `other: ignore`."""
    from .. import hipops as H

    C = int(num_classes)
    H.check_num_classes(C)
    ignore = int(cfg_dataset.get("ignore_label", 255))
    if not C <= ignore <= 255:
        raise ValueError(f"ignore_label = {ignore}: expected a byte value >= num_classes = {C} (labels are 8-bit, class "
                         "indices are 0 .. num_classes - 1)")
    m = cfg_dataset.get("label_map") or {}
    unknown = set(m) - {"offset", "table", "other"}
    if unknown:
        raise ValueError(f"label_map: unknown keys {sorted(unknown)}")
    other = m.get("other", "error")
    if other not in ("error", "ignore"):
        raise ValueError(f"label_map.other = {other!r}: expected 'error' or 'ignore'")
    table, offset = m.get("table"), int(m.get("offset", 0))
    if table is not None:
        table = {int(k): int(v) for k, v in table.items()}
        if any(not 0 <= k <= 255 for k in table):
            raise ValueError("label_map.table: raw values are bytes (0 .. 255)")
    lut = np.full(256, ignore, np.uint8)
    bad = np.zeros(256, bool)
    for v in range(256):
        if table is not None and v in table:      # `table` wins over `offset`
            image, listed = table[v], True
        elif v == ignore:                         # the raw ignore value stays the ignore value
            continue
        elif table is not None:
            image, listed = None, False
        else:
            image, listed = v + offset, False
        if image is not None and 0 <= image < C:
            lut[v] = image
        elif not (listed and image == ignore):    # no image in [0, C): the entry is ignore_label, the value is `other`
            bad[v] = True
    assert ((lut < C) | (lut == ignore)).all()    # the invariant: nothing else can reach a loss kernel
    return lut, (bad if other == "error" else None)


def build_label_lut(cfg_dataset, num_classes):
    """-> np.uint8[256], raw label byte -> class index, from dataset.label_map = {offset, table, other}:
    `table` {raw: class} wins over `offset` (raw v -> v + offset); with neither the map is the identity.  The raw value equal
    to ignore_label maps to ignore_label unless `table` lists it, and every raw value whose image falls outside
    [0, num_classes) gets ignore_label.  Invariant (asserted): every entry is < num_classes or == ignore_label.  The
    table is applied where a label byte is first read -- at load, before any transform -- so the zero padding of the
    crop is class 0 and the rotated-out fill ignore_label, both in mapped space."""
    return label_tables(cfg_dataset, num_classes)[0]


def raw_id_lut(lut, ignore_label=255):
    """inverse of a label table for --raw_ids: class c -> the smallest raw value that maps to c; 255 (what predictions hold
    for dropped pixels) -> the raw ignore_label; classes nothing maps to -> ignore_label too.  np.uint8[256]."""
    inv = np.full(256, ignore_label, np.uint8)
    for v in range(255, -1, -1):
        if lut[v] != ignore_label:
            inv[lut[v]] = v
    inv[255] = ignore_label
    return inv


def read_label(path):
    """label file -> (h, w) uint8 index array.  Mode L and mode P (palette) PNGs hold the indices themselves -- a P image
    is never sent through convert("L"), which would give the luminance of its palette colours; anything else is refused."""
    with open(path, "rb") as f:
        im = Image.open(f)
        if im.mode not in ("L", "P"):
            what = "a 16-bit label file" if im.mode.startswith("I") else "not an index image"
            raise ValueError(f"{path}: mode {im.mode!r} is {what}; labels are 8-bit (mode L or P) throughout this project")
        return np.asarray(im).astype(np.uint8)


DEAD_OPTIONS_MESSAGE = ("dataset option '{}' cannot work upstream either: its transform returns a 5- or 3-tuple that the "
                        "reference's own __getitem__ cannot unpack (cityscapes.py:70-75); the strong augmentations of the "
                        "unlabeled branch are trainer.unsupervised.apply_aug")


def gaussian_blur_weights(radius=2):
    """float32 (5,5) weights of the reference's GaussianBlur(radius) (augmentation.py:325-346), i.e. of
    scipy.ndimage.gaussian_filter(delta, sigma=0.3*(radius-1)+0.8) restated in numpy: the 1-D kernel of radius
    int(4*sigma+0.5), exp(-x^2/2sigma^2) normalised, correlated with the delta row under `reflect` extension;
    the 2-D filter is separable, so the result is the outer product of that row with itself (float64, then cast)."""
    n, sigma = 2 * radius + 1, 0.3 * (radius - 1) + 0.8
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1)
    k = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    k = k / k.sum()
    delta = np.zeros(n)
    delta[radius] = 1.0
    ext = np.pad(delta, r, mode="symmetric")          # scipy's `reflect` (d c b a | a b c d | d c b a)
    row = np.array([np.dot(ext[i:i + 2 * r + 1], k) for i in range(n)])
    return np.outer(row, row).astype(np.float32)


def rotation_matrix(angle):
    """cv2.getRotationMatrix2D((0, 0), angle, 1) as float64 (2,3): OpenCV's formula, computed with `math`."""
    a = angle * math.pi / 180.0
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, s, 0.0], [-s, c, 0.0]])


class Pipeline:
    """ToTensor -> Normalize -> [Resize] -> [RandResize] -> [RandRotate] -> [RandomGaussianBlur] -> [Flip] -> [Crop]
    on (1,C,H,W) tensors; python `random` draws in the reference's order (augmentation.py:51-346,
    cityscapes.py:47-77, pascal_voc.py:48-71)."""

    def __init__(self, cfg):
        self.mean = torch.tensor(np.float32(cfg["mean"]))[None, :, None, None]
        self.std = torch.tensor(np.float32(cfg["std"]))[None, :, None, None]
        self.resize = cfg.get("resize", False)
        self.rand_resize = cfg.get("rand_resize", False)
        self.flip = bool(cfg.get("flip", False))
        self.crop = cfg.get("crop", False)
        self.rotation = cfg.get("rand_rotation", False)
        self.ignore_label = cfg.get("ignore_label", 255)
        self.blur = torch.from_numpy(gaussian_blur_weights())[None, None].repeat(3, 1, 1, 1) if cfg.get(
            "GaussianBlur", False) else None
        for k in ("cutout", "cutmix"):
            if cfg.get(k, False):
                raise NotImplementedError(DEAD_OPTIONS_MESSAGE.format(k))

    def __call__(self, image, label):
        image = torch.from_numpy(np.asarray(image).copy().transpose(2, 0, 1)[None]).float()
        label = torch.from_numpy(np.asarray(label).copy()[None, None]).float()
        image = (image - self.mean) / self.std
        if self.resize:
            image = F.interpolate(image, size=self.resize, mode="bilinear", align_corners=False)
            label = F.interpolate(label, size=self.resize, mode="nearest")
        if self.rand_resize:
            lo, hi = self.rand_resize
            s = lo + (1.0 - lo) * random.random() if random.random() < 0.5 else 1.0 + (hi - 1.0) * random.random()
            h, w = image.shape[-2:]
            size = (int(h * s), int(w * s))
            image = F.interpolate(image, size=size, mode="bilinear", align_corners=False)
            label = F.interpolate(label, size=size, mode="nearest")
        if self.rotation:   # RandRotate (augmentation.py:285-296): rotation about the origin of the NORMALISED grid
            lo, hi = self.rotation
            theta = torch.Tensor(rotation_matrix(lo + (hi - lo) * random.random())).unsqueeze(dim=0)
            grid = F.affine_grid(theta, image.size(), align_corners=False)
            image = F.grid_sample(image, grid, mode="bilinear", align_corners=False)
            label = F.grid_sample(label + 1, grid, mode="nearest", align_corners=False)
            label[label == 0.0] = self.ignore_label + 1     # what the zero padding of grid_sample left outside
            label = label - 1
        if self.blur is not None and random.random() < 0.5:   # RandomGaussianBlur (augmentation.py:315-346)
            image = F.conv2d(image, self.blur, stride=1, padding=2, groups=3)
        if self.flip and random.random() < 0.5:
            image, label = torch.flip(image, [3]), torch.flip(label, [3])
        if self.crop:
            ch, cw = self.crop["size"]
            h, w = image.shape[-2:]
            ph, pw = max(ch - h, 0), max(cw - w, 0)
            if ph or pw:  # labels are padded with 0, not ignore_label (augmentation.py:241-245)
                border = (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)
                image, label = F.pad(image, border, value=0.0), F.pad(label, border, value=0)
            h, w = image.shape[-2:]
            if self.crop["type"] == "rand":
                ho, wo = random.randint(0, h - ch), random.randint(0, w - cw)
            else:
                ho, wo = (h - ch) // 2, (w - cw) // 2
            image, label = image[:, :, ho:ho + ch, wo:wo + cw], label[:, :, ho:ho + ch, wo:wo + cw]
        return image[0].contiguous(), label[0, 0].long().contiguous()


class SegDataset(Dataset):
    """kind_hint "pairs": the paired-list format (parse_pairs) with label_map = label_tables(...) and ignore_label;
    otherwise the naming scheme comes from the list path (parse_list) and labels are read as they always were."""

    def __init__(self, data_root, data_list, transform, seed, n_sup, split, kind_hint=None, label_map=None, ignore_label=255):
        if kind_hint == "pairs":
            self.samples, self.kind = parse_pairs(data_list), "pairs"
            self.lut, self.bad = label_map
        else:
            self.samples, self.kind = parse_list(data_list)
            self.lut = self.bad = None
        self.ignore_label = ignore_label
        self.root, self.transform = data_root, transform
        random.seed(seed)
        if split == "train" and (self.kind == "cityscapes" or n_sup is not None):
            if len(self.samples) < n_sup:   # tile then sample (cityscapes.py:24-31)
                self.samples = self.samples * math.ceil(n_sup / len(self.samples))
            self.samples = random.sample(self.samples, n_sup)

    def __len__(self):
        return len(self.samples)

    def raw_label(self, lp, h, w):
        """paired lists: the label file's raw bytes (all ignore_label without a file), checked against `other: error`"""
        if lp is None:      # a raw value whose table image is ignore_label: ignore_label itself unless `table` lists it
            unmapped = np.flatnonzero(self.lut == self.ignore_label)
            if not unmapped.size:
                raise ValueError("a list line without a label file needs a raw value that dataset.label_map sends to ignore_label")
            raw = self.ignore_label if self.lut[self.ignore_label] == self.ignore_label else int(unmapped[0])
            return np.full((h, w), raw, np.uint8)
        path = os.path.join(self.root, lp)
        label = read_label(path)
        if self.bad is not None:
            present = np.flatnonzero(np.bincount(label.reshape(-1), minlength=256))
            offending = present[self.bad[present]]
            if offending.size:
                raise ValueError(f"{path}: label values {offending.tolist()} are neither mapped by dataset.label_map nor the "
                                 "ignore value (label_map.other: ignore would train on them as ignored pixels)")
        return label

    def __getitem__(self, i):
        ip, lp = self.samples[i]
        with open(os.path.join(self.root, ip), "rb") as f:
            image = Image.open(f).convert("RGB")
        if self.kind == "pairs":    # mapped at load, before any transform
            return self.transform(image, self.lut[self.raw_label(lp, image.size[1], image.size[0])])
        with open(os.path.join(self.root, lp), "rb") as f:
            label = Image.open(f).convert("L")
        return self.transform(image, label)


def _loader(dset, cfg, train):
    # the reference always samples through DistributedSampler (shuffle=True, re-seeded by set_epoch: cityscapes.py:143-163);
    # with explicit num_replicas / rank it needs no process group, so single-GPU runs shuffle per epoch too
    ddp = torch.distributed.is_available() and torch.distributed.is_initialized()
    world, rank = (torch.distributed.get_world_size(), torch.distributed.get_rank()) if ddp else (1, 0)
    sampler = DistributedSampler(dset, num_replicas=world, rank=rank, shuffle=train)
    # (RawSegDataset brings its own collate: batches of mixed image sizes are packed, not stacked)
    return DataLoader(dset, batch_size=cfg.get("batch_size", 1), num_workers=cfg.get("workers", 2), sampler=sampler,
                      shuffle=False, pin_memory=True, drop_last=train, collate_fn=getattr(dset, "collate_fn", None))


def get_loader(cfg, seed=0):
    d = cfg["dataset"]
    pairs = d["type"].startswith("pairs")
    kind = "pairs" if pairs else "cityscapes" if d["type"].startswith("cityscapes") else "pascal"
    semi = d["type"].endswith("_semi")

    def split_cfg(split):
        c = copy.deepcopy(d)
        c.update(c.get(split, {}))
        return c

    tc, vc = split_cfg("train"), split_cfg("val")
    # paired lists always carry a label table (the identity one included); the two reference types carry none
    tables = label_tables(d, cfg["net"]["num_classes"]) if pairs else None
    extra = dict(kind_hint="pairs", label_map=tables, ignore_label=d.get("ignore_label", 255)) if pairs else {}
    val = SegDataset(vc["data_root"], vc["data_list"], Pipeline(vc), seed, None, "val", **extra)
    plan = None
    if d.get("device_aug", False):
        # decoded uint8 samples + host-drawn geometry; the transform chain runs fused on the GPU (device_aug.py):
        # engine.run finishes the batches with augment_batch.  Val loaders stay on the host chain.
        from .device_aug import AugmentPlan, RawSegDataset
        plan = AugmentPlan(tc, lut=tables[0]) if pairs else AugmentPlan(tc)

    def train_loader(dset):
        if plan is None:
            return _loader(dset, tc, True)
        ld = _loader(RawSegDataset(dset, plan), tc, True)
        ld.device_plan = plan
        return ld

    if not semi:
        # (paired lists follow the VOC rule: resampled only when n_sup is given)
        n_sup = tc.get("n_sup", TOTAL_TRAIN[kind]) if kind == "cityscapes" else tc.get("n_sup") if pairs else None
        sup = SegDataset(tc["data_root"], tc["data_list"], Pipeline(tc), seed, n_sup, "train", **extra)
        return train_loader(sup), _loader(val, vc, False)
    unlabeled = tc.get("unlabeled_list") if pairs else None
    if unlabeled is None:
        unlabeled = tc["data_list"].replace("labeled.txt", "unlabeled.txt")
    # both sets are resampled to (total - n_sup) items (cityscapes.py:116-141, pascal_voc.py:109-134; Q12); for the reference's
    # own splits that is the length of the unlabeled list, which is what paired lists are resampled to
    n = len(parse_pairs(unlabeled)) if pairs else TOTAL_TRAIN[kind] - tc.get("n_sup", TOTAL_TRAIN[kind])
    sup = SegDataset(tc["data_root"], tc["data_list"], Pipeline(tc), seed, n, "train", **extra)
    unsup = SegDataset(tc["data_root"], unlabeled, Pipeline(tc), seed, n, "train", **extra)
    return train_loader(sup), train_loader(unsup), _loader(val, vc, False)
