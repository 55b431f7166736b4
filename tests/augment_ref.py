"""Yardstick of the rotation / blur options of the data pipeline: a float64 numpy restatement of RandRotate and
RandomGaussianBlur (reference augmentation.py:269-346) behind the float32 stages the pipeline already has.

`reference(cfg, img, lab, seed)` replays one sample:
  * ToTensor, Normalize and RandResize run in float32 torch exactly as builder.Pipeline runs them (that part is pinned
    bit for bit by tests/test_dataset_cpu.py); their output, cast to float64, is the input of the restatement;
  * the remaining draws (angle, blur coin, flip, crop origin) are taken from python `random` in the reference's order;
  * rotation: F.affine_grid + F.grid_sample(align_corners=False) written out in float64 with the float32 matrix the
    pipeline hands to torch; blur: the 5x5 zero-padded correlation in float64 with the float32 weights.

Besides image and label it returns, per output pixel,
  near   the float64 rotate coordinate lies within NEAR of a rounding boundary (|frac - 0.5| < NEAR in x or y): there
         a float32 evaluation may legitimately pick the neighbouring label;
  absum  sum_k |w_k| |x_k| of the blur, the scale of the a-priori error bound of a 25-term float32 sum.
"""
import math
import random

import numpy as np

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
BASE = dict(mean=MEAN, std=STD, ignore_label=255, crop=dict(type="rand", size=[49, 57]))
# the four configs of tests/golden/augment_rot_blur.npz (tools/gen_augment_golden.py)
CONFIGS = dict(
    rot=dict(BASE, rand_rotation=[-10.0, 10.0]),
    blur=dict(BASE, GaussianBlur=True),
    rot_blur=dict(BASE, rand_rotation=[-10.0, 10.0], GaussianBlur=True),
    all=dict(BASE, rand_rotation=[-10.0, 10.0], GaussianBlur=True, rand_resize=[0.5, 2.0], flip=True),
)
NEAR = 1e-3
NEAR_CAP = 0.01          # at most 1 % of the pixels may be that close to a boundary


def blur_weights_f64():
    """the float32 weights of GaussianBlur(2) as exact float64 numbers, from the golden (the reference's own tensor)"""
    from conftest import golden

    return golden("augment_rot_blur")["blur_weight"][0, 0].astype(np.float64)


def rotate_f64(image, label, m32, ignore_label):
    """image (C,h,w) float64, label (h,w) int, m32 (2,2) float32 -> rotated image, label, near mask"""
    _, h, w = image.shape
    m = np.asarray(m32, np.float32).astype(np.float64)
    xn = ((2.0 * np.arange(w) + 1.0) / w - 1.0)[None, :]
    yn = ((2.0 * np.arange(h) + 1.0) / h - 1.0)[:, None]
    ix = ((m[0, 0] * xn + m[0, 1] * yn + 1.0) * w - 1.0) / 2.0
    iy = ((m[1, 0] * xn + m[1, 1] * yn + 1.0) * h - 1.0) / 2.0
    x0, y0 = np.floor(ix), np.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    out = np.zeros_like(image)
    for dy, wy in ((0, 1.0 - wy1), (1, wy1)):
        for dx, wx in ((0, 1.0 - wx1), (1, wx1)):
            yy, xx = (y0 + dy).astype(np.int64), (x0 + dx).astype(np.int64)
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            tap = image[:, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
            out += np.where(ok, wy * wx, 0.0)[None] * tap
    ny, nx = np.rint(iy).astype(np.int64), np.rint(ix).astype(np.int64)     # nearbyint: half to even
    ok = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
    lab = np.where(ok, label[np.clip(ny, 0, h - 1), np.clip(nx, 0, w - 1)], ignore_label)
    near = (np.abs(wx1 - 0.5) < NEAR) | (np.abs(wy1 - 0.5) < NEAR)
    return out, lab, near


def blur_f64(image, wts):
    """(C,h,w) float64 -> 5x5 correlation with zero padding 2, and the same of |image| with |weights|"""
    _, h, w = image.shape
    pad = np.pad(image, ((0, 0), (2, 2), (2, 2)))
    out, absum = np.zeros_like(image), np.zeros_like(image)
    for ky in range(5):
        for kx in range(5):
            win = pad[:, ky:ky + h, kx:kx + w]
            out += wts[ky, kx] * win
            absum += abs(wts[ky, kx]) * np.abs(win)
    return out, absum


def reference(cfg, img, lab, seed):
    """-> dict(image (3,Sh,Sw) float64, label (Sh,Sw) int64, near, absum, blurred, padding (bool, the crop's zero
    padding), h, w (frame size after RandResize)); consumes python `random` like the pipeline, seeded with `seed`"""
    from PIL import Image

    from u2pl_amd.dataset.builder import Pipeline

    random.seed(seed)
    front = Pipeline(dict(mean=cfg["mean"], std=cfg["std"], rand_resize=cfg.get("rand_resize", False)))
    image, label = front(Image.fromarray(img), Image.fromarray(lab))
    image, label = image.numpy().astype(np.float64), label.numpy()
    _, h, w = image.shape
    near = np.zeros((h, w), bool)
    if cfg.get("rand_rotation", False):
        lo, hi = cfg["rand_rotation"]
        a = (lo + (hi - lo) * random.random()) * math.pi / 180.0
        m32 = np.array([[math.cos(a), math.sin(a)], [-math.sin(a), math.cos(a)]]).astype(np.float32)
        image, label, near = rotate_f64(image, label, m32, cfg.get("ignore_label", 255))
    absum, blurred = np.abs(image), False
    if cfg.get("GaussianBlur", False) and random.random() < 0.5:
        image, absum = blur_f64(image, blur_weights_f64())
        blurred = True
    if cfg.get("flip", False) and random.random() < 0.5:
        image, label, near, absum = (np.flip(a, -1) for a in (image, label, near, absum))
    ch, cw = cfg["crop"]["size"]
    ph, pw = max(ch - h, 0), max(cw - w, 0)
    border = ((ph // 2, ph - ph // 2), (pw // 2, pw - pw // 2))
    image, absum = (np.pad(a, ((0, 0),) + border) for a in (image, absum))
    label, near = np.pad(label, border), np.pad(near, border)
    padding = np.pad(np.zeros((h, w), bool), border, constant_values=True)
    H2, W2 = label.shape
    if cfg["crop"]["type"] == "rand":
        ho, wo = random.randint(0, H2 - ch), random.randint(0, W2 - cw)
    else:
        ho, wo = (H2 - ch) // 2, (W2 - cw) // 2
    sl = (slice(ho, ho + ch), slice(wo, wo + cw))
    return dict(image=image[(slice(None),) + sl], label=label[sl].astype(np.int64), near=near[sl], absum=absum[(slice(None),) + sl],
                blurred=blurred, padding=padding[sl], h=h, w=w)


def host_pipeline(cfg, img, lab, seed):
    """builder.Pipeline on the same sample and seed -> (image (3,Sh,Sw) float32, label (Sh,Sw) int64, next random())"""
    from PIL import Image

    from u2pl_amd.dataset.builder import Pipeline

    random.seed(seed)
    oi, ol = Pipeline(cfg)(Image.fromarray(img), Image.fromarray(lab))
    return oi.numpy(), ol.numpy(), random.random()


def make_mixed_voc(root, sizes=((96, 120), (80, 132), (110, 90), (72, 100)), n=8, C=21, seed=0):
    """synthetic VOC layout (tools/make_synth_dataset.py) whose images all differ in size like the real set; writes
    labeled.txt, unlabeled.txt and val.txt -> (data_root, split dir)"""
    import os

    import make_synth_dataset as M
    from PIL import Image

    rng = np.random.default_rng(seed)
    droot = os.path.join(root, "data", "VOC2012")
    sroot = os.path.join(root, "data", "splits", "pascal", str(n))
    for d in ("JPEGImages", "SegmentationClassAug"):
        os.makedirs(os.path.join(droot, d), exist_ok=True)
    os.makedirs(sroot, exist_ok=True)
    names = []
    for i in range(n):
        H, W = sizes[i % len(sizes)]
        img, lab = M.scene(rng, H + 2 * (i // len(sizes)), W, C)
        Image.fromarray(img).save(os.path.join(droot, "JPEGImages", f"s{i:04d}.jpg"), quality=95)
        Image.fromarray(lab).save(os.path.join(droot, "SegmentationClassAug", f"s{i:04d}.png"))
        names.append(f"s{i:04d}")
    for k in ("labeled", "unlabeled", "val"):
        path = os.path.join(sroot if k != "val" else os.path.dirname(sroot), k + ".txt")
        open(path, "w").write("\n".join(names) + "\n")
    return droot, sroot


def voc_dataset_cfg(droot, sroot, semi, crop=65, batch_size=4, **train_options):
    """the `dataset` section of a VOC experiment on make_mixed_voc's files"""
    import os

    n = sum(1 for _ in open(os.path.join(sroot, "labeled.txt")))
    d = dict(type="pascal_semi" if semi else "pascal", batch_size=batch_size, workers=0, mean=MEAN, std=STD, ignore_label=255,
             train=dict(data_root=droot, data_list=os.path.join(sroot, "labeled.txt"), flip=True,
                        rand_resize=[0.5, 2.0], crop=dict(type="rand", size=[crop, crop]), **train_options),
             val=dict(data_root=droot, data_list=os.path.join(os.path.dirname(sroot), "val.txt"),
                      crop=dict(type="center", size=[crop, crop])))
    if semi:
        d["n_sup"] = 10582 - n          # both train sets are resampled to 10582 - n_sup items (pascal_voc.py:109-134)
    return d
