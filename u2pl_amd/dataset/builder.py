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
    def __init__(self, data_root, data_list, transform, seed, n_sup, split, kind_hint=None):
        self.samples, self.kind = parse_list(data_list)
        self.root, self.transform = data_root, transform
        random.seed(seed)
        if split == "train" and (self.kind == "cityscapes" or n_sup is not None):
            if len(self.samples) < n_sup:   # tile then sample (cityscapes.py:24-31)
                self.samples = self.samples * math.ceil(n_sup / len(self.samples))
            self.samples = random.sample(self.samples, n_sup)

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        ip, lp = self.samples[i]
        with open(os.path.join(self.root, ip), "rb") as f:
            image = Image.open(f).convert("RGB")
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
    kind = "cityscapes" if d["type"].startswith("cityscapes") else "pascal"
    semi = d["type"].endswith("_semi")

    def split_cfg(split):
        c = copy.deepcopy(d)
        c.update(c.get(split, {}))
        return c

    tc, vc = split_cfg("train"), split_cfg("val")
    val = SegDataset(vc["data_root"], vc["data_list"], Pipeline(vc), seed, None, "val")
    plan = None
    if d.get("device_aug", False):
        # decoded uint8 samples + host-drawn geometry; the transform chain runs fused on the GPU (device_aug.py):
        # engine.run finishes the batches with augment_batch.  Val loaders stay on the host chain.
        from .device_aug import AugmentPlan, RawSegDataset
        plan = AugmentPlan(tc)

    def train_loader(dset):
        if plan is None:
            return _loader(dset, tc, True)
        ld = _loader(RawSegDataset(dset, plan), tc, True)
        ld.device_plan = plan
        return ld

    if not semi:
        n_sup = tc.get("n_sup", TOTAL_TRAIN[kind]) if kind == "cityscapes" else None
        sup = SegDataset(tc["data_root"], tc["data_list"], Pipeline(tc), seed, n_sup, "train")
        return train_loader(sup), _loader(val, vc, False)
    # both sets are resampled to (total - n_sup) items (cityscapes.py:116-141, pascal_voc.py:109-134; Q12)
    n = TOTAL_TRAIN[kind] - tc.get("n_sup", TOTAL_TRAIN[kind])
    sup = SegDataset(tc["data_root"], tc["data_list"], Pipeline(tc), seed, n, "train")
    unsup = SegDataset(tc["data_root"], tc["data_list"].replace("labeled.txt", "unlabeled.txt"), Pipeline(tc), seed, n,
                       "train")
    return train_loader(sup), train_loader(unsup), _loader(val, vc, False)
