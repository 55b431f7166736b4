"""Single-image inference (reference infer.py:111-134) and the colour maps of the gray / colour dumps
(utils.py:526-531, 639-700) on the HIP path.

  normalise_lut   infer.py:119-121   (image - mean) / std as a per-channel table over the 256 byte values
  infer_image     infer.py:118-130   table gather + bilinear to the input scale (one kernel), forward, then bilinear to
                                     the image size + argmax + colour lookup (one kernel): neither the resized float
                                     image on the host nor the full-resolution logits exist; half=: the forward on the
                                     fp16 path (u2pl_amd.half), redone in fp32 when it saturated; flip= / prob=: the
                                     views fused at the image size (eval.py:166-180, commented out upstream);
                                     drop_percent= / entropy=: entropy map and labels filtered by it (loss_helper.py:35-43)
  colormap        utils.py:639-700   Pascal VOC / Cityscapes label colours as (256, 3) uint8 tables; "generic": the VOC
                                     rule over all 256 rows, 256 distinct colours for any class count
  dataset_colormap                   the table a config asks for (dataset.colormap) or gets by default
"""
import numpy as np
import torch

from . import hipops as H

# the 19 Cityscapes train ids (road ... bicycle) in the colours of the official cityscapesScripts label table
_CITYSCAPES = [(128, 64, 128), (244, 35, 232), (70, 70, 70), (102, 102, 156), (190, 153, 153), (153, 153, 153), (250, 170, 30),
               (220, 220, 0), (107, 142, 35), (152, 251, 152), (70, 130, 180), (220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70),
               (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32)]


def colormap(name):
    """(256, 3) uint8 table of `name` ("pascal" | "cityscapes" | "generic").  Pascal: the VOC devkit's rule for classes 0..20 (bit
    3j + k of the class index becomes bit 7 - j of channel k), every other row 255; Cityscapes: the 19 train-id colours,
    every other row 0 -- the rows the reference's tables leave at their fill value.  Generic: the devkit's rule for all 256
    rows; it spreads the 8 bits of the index over 3 channels one to one, so the rows are distinct, and rows 0..20 are Pascal's."""
    if name == "generic":
        i = np.arange(256)[:, None, None]
        j, k = np.arange(3)[None, :, None], np.arange(3)[None, None, :]
        return ((((i >> (3 * j + k)) & 1) << (7 - j)).sum(1)).astype(np.uint8)
    if name == "pascal":
        cm = np.full((256, 3), 255, np.uint8)
        for i in range(21):
            cm[i] = [sum(((i >> (3 * j + k)) & 1) << (7 - j) for j in range(3)) for k in range(3)]
        return cm
    if name == "cityscapes":
        cm = np.zeros((256, 3), np.uint8)
        cm[:len(_CITYSCAPES)] = _CITYSCAPES
        return cm
    raise ValueError(f"unknown colour map {name!r}")


def dataset_colormap(ds, default):
    """dataset.colormap ("pascal" | "cityscapes" | "generic") -> table; without the key "generic" for the paired-list
    types and `default` -- what the script has always used -- for the two reference types"""
    return colormap(ds.get("colormap", "generic" if ds["type"].startswith("pairs") else default))


def normalise_lut(mean, std):
    """(3, 256) float32: [c][v] = (v - mean[c]) / std[c].  As in the reference the byte value is a float32 and mean / std
    are Python lists, so numpy evaluates the expression in float64; the result is rounded to float32 once."""
    v = np.arange(256, dtype=np.float32)[:, None]
    return np.ascontiguousarray(((v - list(mean)) / list(std)).astype(np.float32).T)


@torch.no_grad()
def infer_image(model, img_u8, lut, input_scale, palette=None, half=None, flip=False, prob=False, drop_percent=None,
                entropy=False, raw_lut=None):
    """img_u8 (h,w,3) uint8, lut (3,256) float32, palette (256,3) uint8 or None: GPU tensors.
    -> (label (h,w) uint8, rgb (h,w,3) uint8 or None, pred = the decoder's low-resolution logits).
    half: a u2pl_amd.half.HalfPredictor of `model` -- the forward pass runs with fp16 activations and weights, and the
    result gains a fourth element, fell_back: True when that pass saturated (a stored activation beyond +-65504) and the
    image was therefore run again on the fp32 path, whose result is then what is returned.
    flip / prob (test-time fusion, evaluate.fuse_window's rule): the views -- the input and, with flip, its mirror image,
    whose result is mirrored back -- are fused straight to the image size, as class probabilities when prob, into a
    (C,h,w) accumulator (one u2pl_window_fuse_f32 launch per view), which predict_map reads at identity size; pred is then
    that accumulator, and fell_back tells whether any view was run again.
    drop_percent / entropy (reliability maps): when either is set the final scores go through
    H.predict_reliable instead of predict_map and the result gains one last element, dict(entropy (h,w) float32, heat uint8
    (h,w) or None, threshold, ndropped: one-element device tensors or None).  drop_percent = P in [0, 100] has the meaning
    of trainer.unsupervised.drop_percent, the share kept: the pixels whose entropy reaches np.percentile(entropy, P) become
    255 in label and take palette[255] in rgb.  entropy=True adds the heat map (255 = log C) and leaves label / rgb as they
    are without it.
    raw_lut (--raw_ids): (256,) uint8 device table class -> raw id (builder.raw_id_lut); label is rewritten through it in
    place (H.lut_u8) after the colours were looked up, so rgb stays in class space."""
    H.check_drop_percent(drop_percent)
    h, w = img_u8.shape[:2]
    x = H.infer_input(img_u8, lut, input_scale)
    fell_back = False

    def forward(x):
        nonlocal fell_back
        if half is not None:
            pred, saturated = half(x)
            if not saturated > 0:
                return pred
            fell_back = True
        return model(x, need_aux=False, need_rep=False)["pred"]

    pred = forward(x)
    if flip or prob:
        fused = torch.zeros((pred.shape[1], h, w), dtype=torch.float32, device=pred.device)
        weight = 0.5 if flip else 1.0
        H.window_fuse(fused, None, pred, (0, 0), (h, w), False, prob, weight, False)
        if flip:
            H.window_fuse(fused, None, forward(x.flip(3)), (0, 0), (h, w), True, prob, weight, False)
        pred = fused.unsqueeze(0)
    rel = None
    if drop_percent is not None or entropy:
        label, rgb, rel = H.predict_reliable(pred, (h, w), prob, palette, drop_percent, entropy)
    else:
        label, rgb = H.predict_map(pred, (h, w), palette)     # straight to the image size, not through the input scale
    if raw_lut is not None:
        H.lut_u8(label, raw_lut)
    out = (label[0], None if rgb is None else rgb[0], pred)
    if half is not None:
        out += (fell_back,)
    return out if rel is None else out + (rel,)
