"""Device-side training data pipeline.  The decoded uint8 sample goes to the GPU as it is; the
reference's per-sample CPU transform chain (augmentation.py:51-346, composed in cityscapes.py:47-77 and
pascal_voc.py:48-71: ToTensor -> Normalize -> RandResize -> RandRotate -> RandomGaussianBlur ->
RandomHorizontalFlip -> Crop) runs fused on the GPU: equal-sized batches of a config without rotation / blur as ONE
gather (`u2pl_augment_u8_f32`), everything else -- the two options, batches of mixed image sizes (Pascal VOC) --
through `u2pl_augment_ex_u8_f32`.  A plan with a label table (`dataset.label_map`, the paired-list dataset types) takes
`u2pl_augment_lut_u8_f32` for every batch: the same kernels with the table fused into the one read of a source label
byte, so the device only ever sees table outputs.  The random numbers are still drawn on the host with python `random` in the
reference's order, so a seeded run consumes the RNG stream exactly like `builder.Pipeline` does."""
import random

import numpy as np
import torch

from .._lib import call, query
from .builder import DEAD_OPTIONS_MESSAGE, gaussian_blur_weights, rotation_matrix

REC = 16                    # U2PL_AUG_REC: int32 words of a wide record (layout: include/u2pl_hip.h)
ROTATE, BLUR = 1, 2         # U2PL_AUG_ROTATE / U2PL_AUG_BLUR


class AugmentPlan:
    """Draws the per-sample geometry of builder.Pipeline.__call__ without touching pixels."""

    def __init__(self, cfg, lut=None):
        # lut: np.uint8[256] of builder.build_label_lut (raw label byte -> class index), or None: labels are used as read
        self.lut = None if lut is None else np.ascontiguousarray(lut, np.uint8).reshape(256).copy()
        self._dev_lut = {}      # device -> the table
        self.mean = np.asarray(cfg["mean"], np.float32).copy()
        self.std = np.asarray(cfg["std"], np.float32).copy()
        self.rand_resize = cfg.get("rand_resize", False)
        self.rotation = cfg.get("rand_rotation", False)
        self.blur = bool(cfg.get("GaussianBlur", False))
        self.ignore_label = cfg.get("ignore_label", 255)
        self.flip = bool(cfg.get("flip", False))
        self.crop = cfg.get("crop", False)
        self.mode = (ROTATE if self.rotation else 0) | (BLUR if self.blur else 0)
        self.blur_weights = gaussian_blur_weights() if self.blur else None
        self._dev = {}          # device -> (blur weights, scratch) of the two-pass blur
        if cfg.get("resize", False):
            raise NotImplementedError("fixed `resize` is only used by val pipelines; the device pipeline is train-only")
        for k in ("cutout", "cutmix"):
            if cfg.get(k, False):
                raise NotImplementedError(DEAD_OPTIONS_MESSAGE.format(k))
        if not self.crop:
            raise NotImplementedError("the device pipeline emits fixed-size crops (every train config crops)")

    def out_size(self):
        return tuple(self.crop["size"])

    def draw(self, h, w):
        """Same `random` calls in the same order as builder.Pipeline: resize (2), angle (1), blur coin (1), flip (1),
        crop (2).  Without rand_rotation / GaussianBlur in the config
        -> int32[8] = {rh, rw, flip, pad_top, pad_left, crop_y, crop_x, 0}; with one of them the wide record
        -> int32[16] = {rh, rw, flip, pad_top, pad_left, crop_y, crop_x, flags, h, w, m00, m01, m10, m11, 0, 0}:
        flags = ROTATE | BLUR as they apply to THIS sample, m** the bit patterns of the float32 rotation matrix."""
        rh, rw = h, w
        if self.rand_resize:
            lo, hi = self.rand_resize
            s = lo + (1.0 - lo) * random.random() if random.random() < 0.5 else 1.0 + (hi - 1.0) * random.random()
            rh, rw = int(h * s), int(w * s)
        flags, m = 0, np.zeros(4, np.float32)
        if self.rotation:
            lo, hi = self.rotation
            m = rotation_matrix(lo + (hi - lo) * random.random())[:, :2].astype(np.float32).reshape(4)
            flags |= ROTATE
        if self.blur and random.random() < 0.5:
            flags |= BLUR
        flip = int(self.flip and random.random() < 0.5)
        ch, cw = self.crop["size"]
        ph, pw = max(ch - rh, 0), max(cw - rw, 0)
        H2, W2 = rh + ph, rw + pw
        if self.crop["type"] == "rand":
            ho, wo = random.randint(0, H2 - ch), random.randint(0, W2 - cw)
        else:
            ho, wo = (H2 - ch) // 2, (W2 - cw) // 2
        if not self.mode:
            return np.array([rh, rw, flip, ph // 2, pw // 2, ho, wo, 0], np.int32)
        return np.array([rh, rw, flip, ph // 2, pw // 2, ho, wo, flags, h, w, *m.view(np.int32), 0, 0], np.int32)

    def _device_buffers(self, dev, B):
        """blur weights on the device and the caller-owned scratch of the two-pass blur (grown on demand, reused)"""
        Sh, Sw = self.out_size()
        need = query("u2pl_augment_ex_scratch_bytes", B, Sh, Sw, self.mode) // 4
        wts, scratch = self._dev.get(dev, (None, None))
        if wts is None:
            from ..hipops import h2d
            wts = h2d(torch.from_numpy(self.blur_weights.reshape(25)), dev)
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty(need, dtype=torch.float32, device=dev)
        self._dev[dev] = (wts, scratch)
        return wts, scratch

    def _device_lut(self, dev):
        """the label table on the device, copied once per device"""
        t = self._dev_lut.get(dev)
        if t is None:
            from ..hipops import h2d
            t = self._dev_lut[dev] = h2d(torch.from_numpy(self.lut), dev)
        return t


def widen(params, h, w):
    """(B,8) option-free records -> (B,16) wide records of samples that are all h x w (or per-sample sizes)"""
    B = params.shape[0]
    wide = torch.zeros((B, REC), dtype=torch.int32)
    wide[:, :7] = params[:, :7]
    wide[:, 8] = torch.as_tensor(h, dtype=torch.int32)
    wide[:, 9] = torch.as_tensor(w, dtype=torch.int32)
    return wide


def augment_batch(plan, images_u8, labels_u8, params, offsets=None, device=None):
    """Stacked form: images_u8 (B,H,W,3) uint8, labels_u8 (B,H,W) uint8, params (B,8) or (B,16) int32.
    Packed form (RawSegDataset.collate_fn, samples of different sizes): images_u8 / labels_u8 flat uint8 buffers,
    params (B,16) int32 with each sample's size, offsets (B,) int64 = first PIXEL of each sample.
    Tensors still on the host (pinned by the DataLoader) are copied to `device` without blocking.
    With plan.lut every batch, option-free dense ones included, takes u2pl_augment_lut_u8_f32: labels_u8 are the RAW bytes of
    the label files and the output labels their table images; without it the calls are the ones made before the table existed.
    -> (B,3,Sh,Sw) float32 normalised crops, (B,Sh,Sw) int64 labels."""
    from ..hipops import h2d

    dev = images_u8.device if images_u8.is_cuda else torch.device(device)
    packed = offsets is not None
    if packed:
        B = params.shape[0]
        if params.shape[1] != REC:
            raise ValueError("a packed batch carries wide records (each sample's size travels in its record)")
        if not offsets.is_cuda:      # the kernel trusts the table: check it against the buffers while it is on the host
            px = params[:, 8].long() * params[:, 9].long()
            if int(offsets.min()) < 0 or int((offsets + px).max()) > labels_u8.numel() or \
                    images_u8.numel() != 3 * labels_u8.numel():
                raise ValueError("packed batch: offsets / sizes do not fit the buffers")
        H = W = 0
    else:
        B, H, W, _ = images_u8.shape
    Sh, Sw = plan.out_size()
    old_entry = not packed and not plan.mode and params.shape[1] == 8 and plan.lut is None
    if not old_entry and params.shape[1] == 8:
        params = widen(params.cpu(), H, W)
    images_u8, labels_u8 = (t if t.is_cuda else t.to(dev, non_blocking=True) for t in (images_u8, labels_u8))
    if not params.is_cuda:
        params = h2d(params.contiguous(), dev)
    if packed and not offsets.is_cuda:
        offsets = h2d(offsets.contiguous(), dev)
    out = torch.empty((B, 3, Sh, Sw), dtype=torch.float32, device=dev)
    lab = torch.empty((B, Sh, Sw), dtype=torch.int64, device=dev)
    if old_entry:
        call("u2pl_augment_u8_f32", images_u8.contiguous(), labels_u8.contiguous(), params, B, H, W, Sh, Sw,
             plan.mean.ctypes.data, plan.std.ctypes.data, out, lab)
        return out, lab
    wts, scratch = plan._device_buffers(dev, B) if plan.mode & BLUR else (None, None)
    if plan.lut is not None:
        call("u2pl_augment_lut_u8_f32", images_u8.contiguous(), labels_u8.contiguous(), offsets, params, B, H, W, Sh, Sw,
             plan.ignore_label, plan.mode, plan._device_lut(dev), plan.mean.ctypes.data, plan.std.ctypes.data, wts, scratch,
             out, lab)
        return out, lab
    call("u2pl_augment_ex_u8_f32", images_u8.contiguous(), labels_u8.contiguous(), offsets, params, B, H, W, Sh, Sw,
         plan.ignore_label, plan.mode, plan.mean.ctypes.data, plan.std.ctypes.data, wts, scratch, out, lab)
    return out, lab


class RawSegDataset(torch.utils.data.Dataset):
    """Same sample list / resampling as builder.SegDataset, but __getitem__ returns the decoded uint8 sample
    plus the drawn geometry; `augment_batch` finishes the job on the GPU.  Batches are built by `collate_fn`:
    samples of one size (Cityscapes: 1024 x 2048) are stacked, samples of different sizes (Pascal VOC) are packed."""

    def __init__(self, base, plan):
        self.base, self.plan = base, plan

    def __len__(self):
        return len(self.base)

    def __getitem__(self, i):
        import os

        from PIL import Image

        ip, lp = self.base.samples[i]
        with open(os.path.join(self.base.root, ip), "rb") as f:
            image = np.asarray(Image.open(f).convert("RGB")).copy()
        if self.base.kind == "pairs":   # raw bytes (checked against `other: error`): the table is applied on the GPU
            label = self.base.raw_label(lp, image.shape[0], image.shape[1]).copy()
        else:
            with open(os.path.join(self.base.root, lp), "rb") as f:
                label = np.asarray(Image.open(f).convert("L")).copy()
        params = self.plan.draw(image.shape[0], image.shape[1])
        return torch.from_numpy(image), torch.from_numpy(label), torch.from_numpy(params)

    @staticmethod
    def collate_fn(samples):
        """[(image (H,W,3), label (H,W), record)] -> the stacked batch [images (B,H,W,3), labels (B,H,W), records] when all
        sizes agree (what the default collate gives), else the packed batch [images flat, labels flat, records (B,16),
        offsets (B,) int64]: sample b occupies pixels offsets[b] .. offsets[b] + H_b * W_b of both buffers (3 bytes per
        pixel in the image buffer), and its H_b, W_b travel in words 8 and 9 of its record."""
        images, labels, recs = zip(*samples)
        if len({tuple(l.shape) for l in labels}) == 1:
            return [torch.stack(images), torch.stack(labels), torch.stack(recs)]
        sizes = [tuple(l.shape) for l in labels]
        px = torch.tensor([h * w for h, w in sizes], dtype=torch.int64)
        offsets = torch.cumsum(px, 0) - px
        recs = torch.stack(recs)
        if recs.shape[1] == 8:
            recs = widen(recs, [h for h, _ in sizes], [w for _, w in sizes])
        return [torch.cat([i.reshape(-1) for i in images]), torch.cat([l.reshape(-1) for l in labels]), recs, offsets]
