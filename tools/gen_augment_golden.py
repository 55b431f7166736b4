"""Writes tests/golden/augment_rot_blur.npz: the reference's own transform classes, as its
pascal_voc.build_transfrom composes them (pascal_voc.py:48-71), with `rand_rotation` and `GaussianBlur` switched on.
Needs the reference tree (oracle/ref_shim.py) and scipy (the reference's GaussianBlur imports it); the tests only read
the stored arrays.  Re-run:  python tools/gen_augment_golden.py

Two things the reference cannot do by itself here:
  * OpenCV is not installed, so the shim's empty `cv2` module gets a getRotationMatrix2D for the one call RandRotate makes
    (centre (0, 0), scale 1): OpenCV's documented formula computed with `math`.  It has not been compared with a real cv2.
  * augmentation.Compose.__call__ (augmentation.py:31-47) unpacks two values only from its first five transforms; from the
    sixth on it expects the 5- / 3-tuples of the dead cutout / cutmix options and raises.  The largest config below has
    seven transforms, so every case applies `compose.segtransforms` one after the other; for the configs of at most five
    transforms the script asserts that this gives what Compose.__call__ gives, bit for bit.
"""
import importlib
import math
import os
import random
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from augment_ref import CONFIGS  # noqa: E402  (the four configs; the tests read the same table)

SEEDS = [0, 1, 2, 3, 4, 5]


def rotation_matrix_2d(center, angle, scale):
    assert tuple(center) == (0, 0) and scale == 1
    a = angle * math.pi / 180.0
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, s, 0.0], [-s, c, 0.0]])


def apply(tf, img, lab):
    image, label = Image.fromarray(img), Image.fromarray(lab)
    for t in tf.segtransforms:
        image, label = t(image, label)
    return image, label


def main():
    ref_shim.install(init_dist=False)
    sys.modules["cv2"].getRotationMatrix2D = rotation_matrix_2d
    voc = importlib.import_module("u2pl.dataset.pascal_voc")
    aug = importlib.import_module("u2pl.dataset.augmentation")
    rng = np.random.default_rng(7)          # the sample of oracle/gen_golden.py:gen_augment
    img = rng.integers(0, 256, (60, 84, 3), dtype=np.uint8)
    lab = rng.integers(0, 19, (60, 84), dtype=np.uint8)
    lab[:4] = 255
    fx = dict(img=img, lab=lab, seeds=np.array(SEEDS), configs=np.array(list(CONFIGS)),
              blur_weight=aug.GaussianBlur(2).kernel.weight.detach().numpy())
    for name, cfg in CONFIGS.items():
        coins = set()
        for sd in SEEDS:
            random.seed(sd)
            tf = voc.build_transfrom(cfg)
            oi, ol = apply(tf, img, lab)
            nxt = random.random()
            if len(tf.segtransforms) <= 5:
                random.seed(sd)
                ci, cl = voc.build_transfrom(cfg)(Image.fromarray(img), Image.fromarray(lab))
                assert torch.equal(ci, oi) and torch.equal(cl, ol) and random.random() == nxt
            fx[f"{name}_img_{sd}"] = oi[0].numpy()
            fx[f"{name}_lab_{sd}"] = ol[0, 0].long().to(torch.uint8).numpy()
            fx[f"{name}_next_{sd}"] = np.float64(nxt)
            # which way the blur / flip coins fell, replayed from the same stream (resize 2 draws, angle 1, blur 1, flip 1)
            random.seed(sd)
            if cfg.get("rand_resize"):
                random.random() < 0.5
                random.random()
            if cfg.get("rand_rotation"):
                random.random()
            if cfg.get("GaussianBlur"):
                coins.add(("blur", random.random() < 0.5))
            if cfg.get("flip"):
                coins.add(("flip", random.random() < 0.5))
        for k in ("GaussianBlur", "flip"):
            if cfg.get(k):
                tag = "blur" if k == "GaussianBlur" else "flip"
                assert {(tag, True), (tag, False)} <= coins, (name, coins)      # both outcomes occur among the seeds
    path = os.path.join(ROOT, "tests", "golden", "augment_rot_blur.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
