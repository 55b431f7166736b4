"""torch (CPU) restatement of test-time flip / probability fusion: the block the reference leaves commented out in
eval.py:166-180 (softmax per view, a mirrored view flipped back, the mean over views) inside its live
scale_crop_process / validate_city control flow (eval.py:184-224, 264-284).  Shared by tests/test_tta_cpu.py and
tests/test_gpu_tta.py; every function follows the dtype of what it is given (float32 or float64)."""
import math

import torch
import torch.nn.functional as F


def window_fuse_ref(pred, count, logits, origin, size, flip, softmax, weight, bump):
    """what u2pl_window_fuse_f32 does, in place: pred (C,H,W), count (H,W) or None, logits (C,h,w)"""
    (h0, w0), (hc, wc) = origin, size
    v = F.interpolate(logits.unsqueeze(0), size=(hc, wc), mode="bilinear", align_corners=True)[0]
    if flip:
        v = v.flip(2)
    if softmax:
        v = F.softmax(v, dim=0)
    pred[:, h0:h0 + hc, w0:w0 + wc] += weight * v
    if bump:
        count[h0:h0 + hc, w0:w0 + wc] += 1


def fused_window_ref(net, crop, flip, prob):
    """net: (1,3,h,w) -> low-resolution logits (1,C,h',w').  -> (C,h,w): the mean over the views of one window"""
    def view(x):
        v = F.interpolate(net(x), size=crop.shape[2:], mode="bilinear", align_corners=True)
        return F.softmax(v, dim=1) if prob else v
    out = view(crop)
    if flip:
        out = 0.5 * out + 0.5 * view(crop.flip(3)).flip(3)
    return out[0]


def scale_crop_ref(net, image, classes, crop_h, crop_w, h, w, flip, prob, stride_rate=2 / 3):
    ori_h, ori_w = image.shape[2:]
    pad_h, pad_w = max(crop_h - ori_h, 0), max(crop_w - ori_w, 0)
    ph, pw = int(pad_h / 2), int(pad_w / 2)
    if pad_h > 0 or pad_w > 0:
        image = F.pad(image, (pw, pad_w - pw, ph, pad_h - ph), mode="constant", value=0.0)
    new_h, new_w = image.shape[2:]
    stride_h, stride_w = int(math.ceil(crop_h * stride_rate)), int(math.ceil(crop_w * stride_rate))
    grid_h = int(math.ceil(float(new_h - crop_h) / stride_h) + 1)
    grid_w = int(math.ceil(float(new_w - crop_w) / stride_w) + 1)
    pred = torch.zeros((classes, new_h, new_w), dtype=image.dtype)
    cnt = torch.zeros((new_h, new_w), dtype=image.dtype)
    for ih in range(grid_h):
        for iw in range(grid_w):
            e_h, e_w = min(ih * stride_h + crop_h, new_h), min(iw * stride_w + crop_w, new_w)
            s_h, s_w = e_h - crop_h, e_w - crop_w
            cnt[s_h:e_h, s_w:e_w] += 1
            pred[:, s_h:e_h, s_w:e_w] += fused_window_ref(net, image[:, :, s_h:e_h, s_w:e_w].contiguous(), flip, prob)
    pred = (pred / cnt)[:, ph:ph + ori_h, pw:pw + ori_w]
    return F.interpolate(pred.unsqueeze(0), size=(h, w), mode="bilinear", align_corners=True)[0]


def scaled_size(h, w, base_size, scale):
    long_size = round(scale * base_size)
    new_h = new_w = long_size
    if h > w:
        new_w = round(long_size / float(h) * w)
    else:
        new_h = round(long_size / float(w) * h)
    return new_h, new_w


def predict_image_ref(net, image, classes, base_size, crop, scales, use_crop, flip, prob):
    """image (1,3,h,w) -> (classes,h,w): the sum over scales (validate_city's inner loop)"""
    h, w = image.shape[2:]
    total = torch.zeros((classes, h, w), dtype=image.dtype)
    for scale in scales:
        size = scaled_size(h, w, base_size, scale)
        scaled = image if size == (h, w) else F.interpolate(image, size=size, mode="bilinear", align_corners=True)
        if use_crop:
            total += scale_crop_ref(net, scaled, classes, crop[0], crop[1], h, w, flip, prob)
        else:
            fused = fused_window_ref(net, scaled, flip, prob)
            total += F.interpolate(fused.unsqueeze(0), size=(h, w), mode="bilinear", align_corners=True)[0]
    return total
