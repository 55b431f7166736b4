"""Sliding-window / whole-image evaluation (reference eval.py:158-320) on the HIP forward path.

  net_process          eval.py:158-181   model(x)["pred"] -> bilinear(align_corners=True) to the input size
  fuse_window          eval.py:166-180   (commented out upstream) softmax per view, a mirrored view flipped back, the mean
                                         over views: one u2pl_window_fuse_f32 launch per view (flip= / prob=)
  scale_crop_process   eval.py:184-224   zero-pad to the crop size, windows at stride ceil(crop * 2/3) (the last
                                         window is pulled back inside the image), sum of window logits / window
                                         count, un-pad, bilinear to the label size
  validate_city        eval.py:235-306   per image: sum over scales, argmax, intersection / union histograms
  mIoU                 eval.py:302-305   mean(I / (U + 1e-10))
Host side = the reference's control flow; every tensor op is a libu2pl_hip kernel (forward stack, bilinear,
window accumulate / normalise, confusion histogram).
"""
import math

import numpy as np
import torch

from . import hipops as H
from ._lib import call


@torch.no_grad()
def view_logits(model, image, half=None):
    """image (1,3,h,w) on the GPU -> one view's low-resolution logits (1,C,h',w'), as the decoder leaves them.  half: a
    u2pl_amd.half.HalfPredictor of `model`: the forward runs on the fp16 path; a pass that saturated (its count is nonzero)
    is recomputed on the fp32 path."""
    out = None
    if half is not None:
        out, saturated = half(image)
        if saturated:
            out = None
    if out is None:
        out = model(image, need_aux=False, need_rep=False)["pred"]
    return out


@torch.no_grad()
def fuse_window(model, crop, pred, count, origin, half=None, flip=False, prob=False, first=None):
    """test-time fusion of one window (the block eval.py:166-180 leaves commented out), in place: the window's views --
    `crop`, and with flip its mirror image, whose result is mirrored back -- are interpolated to the crop's size, turned
    into class probabilities when prob, and their mean is added into pred at origin; count (None: not kept) gains 1.  One
    u2pl_window_fuse_f32 launch per view; a view's full-resolution logits are never written.  first: view_logits of
    `crop` when the caller has them already."""
    size = crop.shape[2:]
    weight = 0.5 if flip else 1.0
    if first is None:
        first = view_logits(model, crop, half)
    H.window_fuse(pred, count, first, origin, size, False, prob, weight, count is not None)
    if flip:
        H.window_fuse(pred, count, view_logits(model, crop.flip(3), half), origin, size, True, prob, weight, False)


@torch.no_grad()
def net_process(model, image, half=None, flip=False, prob=False):
    """image (1,3,h,w) on the GPU -> logits (1,C,h,w), planar.  half: see view_logits.  flip / prob: the mean over the
    image and its mirror image / of class probabilities instead of logits (fuse_window with one window = the image)."""
    out = view_logits(model, image, half)
    if not (flip or prob):
        return H.bilinear_up(out, image.shape[2:])
    fused = torch.zeros((1, out.shape[1]) + tuple(image.shape[2:]), dtype=torch.float32, device=image.device)
    fuse_window(model, image, fused, None, (0, 0), half, flip, prob, first=out)
    return fused


def window_grid(new_h, new_w, crop_h, crop_w, stride_rate=2 / 3):
    """[(s_h, s_w)] window origins in the reference's visiting order."""
    stride_h, stride_w = int(math.ceil(crop_h * stride_rate)), int(math.ceil(crop_w * stride_rate))
    grid_h = int(math.ceil(float(new_h - crop_h) / stride_h) + 1)
    grid_w = int(math.ceil(float(new_w - crop_w) / stride_w) + 1)
    wins = []
    for ih in range(grid_h):
        for iw in range(grid_w):
            e_h = min(ih * stride_h + crop_h, new_h)
            e_w = min(iw * stride_w + crop_w, new_w)
            wins.append((e_h - crop_h, e_w - crop_w))
    return wins


@torch.no_grad()
def scale_crop_process(model, image, classes, crop_h, crop_w, h, w, stride_rate=2 / 3, half=None, flip=False, prob=False):
    """image (1,3,H,W) GPU tensor -> logits (classes, h, w); with flip / prob every window is fused by fuse_window."""
    ori_h, ori_w = image.shape[2:]
    pad_h, pad_w = max(crop_h - ori_h, 0), max(crop_w - ori_w, 0)
    ph, pw = int(pad_h / 2), int(pad_w / 2)
    if pad_h > 0 or pad_w > 0:
        padded = torch.zeros((1, image.shape[1], ori_h + pad_h, ori_w + pad_w), dtype=torch.float32, device=image.device)
        padded[:, :, ph:ph + ori_h, pw:pw + ori_w] = image
        image = padded
    new_h, new_w = image.shape[2:]
    pred = torch.zeros((1, classes, new_h, new_w), dtype=torch.float32, device=image.device)
    count = torch.zeros((new_h, new_w), dtype=torch.float32, device=image.device)
    for s_h, s_w in window_grid(new_h, new_w, crop_h, crop_w, stride_rate):
        crop = image[:, :, s_h:s_h + crop_h, s_w:s_w + crop_w].contiguous()
        if flip or prob:
            fuse_window(model, crop, pred, count, (s_h, s_w), half, flip, prob)
            continue
        logits = net_process(model, crop, half).contiguous()
        call("u2pl_window_accumulate_f32", pred, count, classes, new_h, new_w, logits, s_h, s_w, crop_h, crop_w)
    call("u2pl_window_normalize_f32", pred, count, classes, new_h, new_w)
    pred = pred[:, :, ph:ph + ori_h, pw:pw + ori_w]
    return H.bilinear_up(pred.contiguous(), (h, w))[0]


@torch.no_grad()
def scale_whole_process(model, image, h, w, half=None, flip=False, prob=False):
    """with flip / prob: one fused window that covers the scaled image (its count would be 1 everywhere: not kept)"""
    return H.bilinear_up(net_process(model, image, half, flip, prob), (h, w))[0]


@torch.no_grad()
def predict_image(model, image, classes, base_size, crop, scales=(1.0,), use_crop=True, half=None, flip=False, prob=False):
    """image (1,3,h,w) normalised GPU tensor -> summed logits (classes, h, w) (validate_city's inner loop).  flip / prob:
    per window, the mean over the window and its mirror image / of class probabilities instead of logits; scales are
    still summed."""
    h, w = image.shape[2:]
    total = torch.zeros((classes, h, w), dtype=torch.float32, device=image.device)
    for scale in scales:
        long_size = round(scale * base_size)
        new_h = new_w = long_size
        if h > w:
            new_w = round(long_size / float(h) * w)
        else:
            new_h = round(long_size / float(w) * h)
        scaled = image if (new_h, new_w) == (h, w) else H.bilinear_up(image.contiguous(), (new_h, new_w))
        if use_crop:
            total += scale_crop_process(model, scaled, classes, crop[0], crop[1], h, w, half=half, flip=flip, prob=prob)
        else:
            total += scale_whole_process(model, scaled, h, w, half, flip, prob)
    return total


def _iou(hist3c):
    """(3, C) intersection / output / target counts -> (mIoU, per-class IoU), eval.py:302-305"""
    hh = np.asarray(hist3c, dtype=np.float64)
    iou = hh[0] / (hh[1] + hh[2] - hh[0] + 1e-10)
    return float(np.mean(iou)), iou


@torch.no_grad()
def evaluate(model, samples, classes, base_size, crop, scales=(1.0,), use_crop=True, ignore=255, on_prediction=None,
             palette=None, half=None, flip=False, prob=False, drop_percent=None, entropy=False, raw_lut=None):
    """samples: iterable of (image (3,h,w) float tensor already mean/std normalised, label (h,w) integer array).
    Returns (mIoU, per-class IoU).  on_prediction(i, uint8 map) receives every argmax map (gray dumps); with a
    palette ((256,3) uint8, array or tensor) it is called as on_prediction(i, gray, color): both maps come from one
    u2pl_predict_map_f32 launch on the summed logits (lowest class index wins a tie) and one uint8 copy each.
    half: a u2pl_amd.half.HalfPredictor of `model`: every forward call runs on the fp16 path (view_logits).
    flip / prob: test-time fusion of every window (fuse_window); with flip a window costs two forward passes.
    drop_percent / entropy (reliability maps): per image, on the summed scores (class weights when prob), the
    entropy map and with drop_percent = P the labels filtered at np.percentile(entropy, P) (H.predict_reliable).  With
    either set on_prediction receives the filtered maps and one more trailing argument, the entropy heat map (uint8, None
    without entropy=True).  With drop_percent the return value is (mIoU, IoU, rel): mIoU / IoU are those of the unfiltered
    arg-max as before, and rel = dict(miou_reliable, iou_reliable, miou_unreliable, iou_unreliable, coverage = kept pixels
    over non-ignored pixels, hist_reliable, hist_unreliable = the (3, classes) integer counts) from a second confusion
    histogram on the target with the unreliable pixels set to `ignore`; unreliable = total - reliable.
    raw_lut (--raw_ids): (256,) uint8 table class -> raw id (builder.raw_id_lut); the gray map handed to on_prediction goes
    through it on the device (H.lut_u8, in place).  Colours and every IoU stay in class space."""
    H.check_drop_percent(drop_percent)
    model.eval()
    dev = next(model.parameters()).device
    hist = torch.zeros(3 * classes, dtype=torch.int64, device=dev)
    hist_rel = torch.zeros(3 * classes, dtype=torch.int64, device=dev) if drop_percent is not None else None
    if palette is not None:
        palette = torch.as_tensor(palette).to(dev)
    if raw_lut is not None:
        raw_lut = torch.as_tensor(raw_lut).to(dev)
    for i, (image, label) in enumerate(samples):
        image = torch.as_tensor(image, dtype=torch.float32).unsqueeze(0).to(dev)
        logits = predict_image(model, image, classes, base_size, crop, scales, use_crop, half, flip, prob)
        lab = torch.as_tensor(np.asarray(label)).to(dev).long().contiguous().unsqueeze(0)
        h, w = lab.shape[1:]
        call("u2pl_confusion_hist_f32", logits.contiguous(), lab, ignore, 1, classes, h, w, hist)
        if drop_percent is not None or (entropy and on_prediction is not None):
            dump = on_prediction is not None
            gray, color, rel = H.predict_reliable(logits.unsqueeze(0), (h, w), prob, palette if dump else None, drop_percent,
                                                  entropy and dump)
            if drop_percent is not None:
                kept = lab.clone()
                H.drop_high_entropy_(kept, rel["entropy"], rel["threshold"], ignore)
                call("u2pl_confusion_hist_f32", logits.contiguous(), kept, ignore, 1, classes, h, w, hist_rel)
            if on_prediction is not None:
                if raw_lut is not None:
                    H.lut_u8(gray, raw_lut)
                maps = [gray[0].cpu().numpy()] + ([] if color is None else [color[0].cpu().numpy()])
                on_prediction(i, *maps, None if rel["heat"] is None else rel["heat"].cpu().numpy())
        elif on_prediction is not None and palette is not None:
            gray, color = H.predict_map(logits.unsqueeze(0), (h, w), palette)
            if raw_lut is not None:
                H.lut_u8(gray, raw_lut)
            on_prediction(i, gray[0].cpu().numpy(), color[0].cpu().numpy())
        elif on_prediction is not None:
            gray = logits.argmax(0).to(torch.uint8)
            on_prediction(i, (gray if raw_lut is None else H.lut_u8(gray.contiguous(), raw_lut)).cpu().numpy())
    hh = hist.cpu().double().reshape(3, classes)
    inter, union = hh[0], hh[1] + hh[2] - hh[0]
    iou = (inter / (union + 1e-10)).numpy()
    if hist_rel is None:
        return float(np.mean(iou)), iou
    total, reliable = hist.cpu().numpy().reshape(3, classes), hist_rel.cpu().numpy().reshape(3, classes)
    unreliable = total - reliable
    (mr, ir), (mu, iu) = _iou(reliable), _iou(unreliable)
    rel = dict(miou_reliable=mr, iou_reliable=ir, miou_unreliable=mu, iou_unreliable=iu,
               coverage=float(reliable[1].sum()) / max(float(total[1].sum()), 1.0), hist_reliable=reliable,
               hist_unreliable=unreliable)
    return float(np.mean(iou)), iou, rel
