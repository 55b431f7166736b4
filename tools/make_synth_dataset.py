"""Deterministic synthetic datasets in the reference's on-disk layouts (SURVEY hard part 11):
Cityscapes (leftImg8bit/<split>/<city>/*_leftImg8bit.png + gtFine/..._gtFine_labelTrainIds.png, list lines as in
data/splits/cityscapes/*/labeled.txt, list path contains "cityscapes") and VOC (JPEGImages / SegmentationClassAug);
and a paired-list dataset (dataset.type pairs / pairs_semi) that stores its labels ADE20K-style: class + 1, 0 = unlabeled."""
import os
import sys

import numpy as np
import yaml
from PIL import Image


def scene(rng, H, W, C, cell=16):
    g = rng.integers(0, C, ((H + cell - 1) // cell, (W + cell - 1) // cell))
    lab = np.kron(g, np.ones((cell, cell), dtype=np.int64))[:H, :W].astype(np.uint8)
    lab[:4] = 255
    pal = (np.arange(C)[:, None] * np.array([37, 91, 151]) % 256).astype(np.uint8)
    img = pal[np.where(lab == 255, 0, lab)] + rng.integers(0, 40, (H, W, 3), dtype=np.uint8)
    return img.astype(np.uint8), lab


def make_cityscapes(root, n_l=4, n_u=4, n_val=4, H=140, W=200, C=19, seed=0):
    rng = np.random.default_rng(seed)
    droot = os.path.join(root, "data", "cityscapes")
    sroot = os.path.join(root, "data", "splits", "cityscapes", str(n_l))
    os.makedirs(sroot, exist_ok=True)
    lists = {"labeled": [], "unlabeled": [], "val": []}
    for split, name, n in (("train", "labeled", n_l), ("train", "unlabeled", n_u), ("val", "val", n_val)):
        for i in range(n):
            city = "synth"
            stem = f"{city}_{name}_{i:06d}_000019"
            ip = f"leftImg8bit/{split}/{city}/{stem}_leftImg8bit.png"
            lp = f"gtFine/{split}/{city}/{stem}_gtFine_labelTrainIds.png"
            img, lab = scene(rng, H, W, C)
            for p, a in ((ip, img), (lp, lab)):
                os.makedirs(os.path.dirname(os.path.join(droot, p)), exist_ok=True)
                Image.fromarray(a).save(os.path.join(droot, p))
            lists[name].append(ip)
    for k, v in lists.items():
        path = os.path.join(sroot if k != "val" else os.path.dirname(sroot), k + ".txt")
        open(path, "w").write("\n".join(v) + "\n")
    return droot, sroot


def make_voc(root, n=8, H=96, W=120, C=21, seed=0):
    rng = np.random.default_rng(seed)
    droot = os.path.join(root, "data", "VOC2012")
    sroot = os.path.join(root, "data", "splits", "pascal", str(n))
    for d in ("JPEGImages", "SegmentationClassAug"):
        os.makedirs(os.path.join(droot, d), exist_ok=True)
    os.makedirs(sroot, exist_ok=True)
    names = []
    for i in range(n):
        img, lab = scene(rng, H, W, C)
        Image.fromarray(img).save(os.path.join(droot, "JPEGImages", f"s{i:04d}.jpg"), quality=95)
        Image.fromarray(lab).save(os.path.join(droot, "SegmentationClassAug", f"s{i:04d}.png"))
        names.append(f"s{i:04d}")
    for k in ("labeled", "val"):
        open(os.path.join(sroot if k != "val" else os.path.dirname(sroot), k + ".txt"), "w").write("\n".join(names) + "\n")
    return droot, sroot


def make_pairs(root, n_l=4, n_u=4, n_val=4, H=110, W=150, C=40, raw_offset=1, palette_png=True, mixed_sizes=False, seed=0):
    """paired-list dataset: images/<name>.jpg + labels/<name>.png, lists of `image_path label_path` lines (labeled.txt,
    val.txt) and of single-field lines (unlabeled.txt, which has label files on disk but does not name them).  Labels are
    stored as class + raw_offset with 0 for "unlabeled" (scene()'s 255 rows); mode P files with a palette whose luminance
    differs from the index when palette_png, mode L otherwise.  mixed_sizes: every image a little different in size.
    -> (data_root, list dir)"""
    rng = np.random.default_rng(seed)
    droot, sroot = os.path.join(root, "data", "pairs"), os.path.join(root, "data", "pairs", "lists")
    for d in ("images", "labels", "lists"):
        os.makedirs(os.path.join(droot, d), exist_ok=True)
    pal = (np.arange(256)[:, None] * np.array([151, 37, 91]) % 256).astype(np.uint8)
    lists = {}
    for name, n in (("labeled", n_l), ("unlabeled", n_u), ("val", n_val)):
        lines = []
        for i in range(n):
            h, w = (H - 6 * (i % 3), W + 4 * (i % 4)) if mixed_sizes else (H, W)
            img, lab = scene(rng, h, w, C)
            raw = np.where(lab == 255, 0, lab.astype(np.int64) + raw_offset).astype(np.uint8)
            ip, lp = f"images/{name}_{i:04d}.jpg", f"labels/{name}_{i:04d}.png"
            Image.fromarray(img).save(os.path.join(droot, ip), quality=95)
            lim = Image.fromarray(raw)
            if palette_png:      # putpalette turns the L image into a P image over the same index bytes
                lim.putpalette(pal.reshape(-1).tolist())
            lim.save(os.path.join(droot, lp))
            lines.append(ip if name == "unlabeled" else ip + " " + lp)
        lists[name] = os.path.join(sroot, name + ".txt")
        open(lists[name], "w").write("\n".join(lines) + "\n")
    return droot, sroot


def write_pairs_config(root, droot, sroot, C=40, crop=97, arch="resnet50", epochs=1, semi=True, device_aug=False, raw_offset=1):
    """the experiment config of make_pairs' files: the Cityscapes template with dataset.type pairs_semi (pairs when not
    semi: no representation head, no unsupervised / contrastive sections), label_map {offset: -raw_offset, other: ignore}
    (raw 0, "unlabeled", has no class) and net.num_classes = C"""
    exp = os.path.join(root, "experiments", "pairs", "ours")
    os.makedirs(exp, exist_ok=True)
    ref = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "city_semi_template.yaml")))
    ds = ref["dataset"]
    ds["type"] = "pairs_semi" if semi else "pairs"
    ds["label_map"] = dict(offset=-raw_offset, other="ignore")
    ds["train"].update(data_root=droot, data_list=os.path.join(sroot, "labeled.txt"), crop=dict(type="rand", size=[crop, crop]))
    ds["val"].update(data_root=droot, data_list=os.path.join(sroot, "val.txt"), crop=dict(type="center", size=[crop, crop]))
    ds.pop("n_sup")
    ds["workers"] = 0
    ds["device_aug"] = bool(device_aug)
    ref["trainer"]["epochs"] = epochs
    ref["criterion"]["kwargs"]["min_kept"] = 3000
    ref["net"].update(sync_bn=False, num_classes=C)
    ref["net"]["encoder"]["type"] = f"u2pl.models.resnet.{arch}"
    ref["net"]["encoder"]["kwargs"]["pretrained"] = False
    if not semi:
        ref["net"]["decoder"]["kwargs"]["rep_head"] = False
        for k in ("unsupervised", "contrastive"):
            ref["trainer"].pop(k)
    path = os.path.join(exp, "config.yaml")
    yaml.safe_dump(ref, open(path, "w"))
    return path


def write_city_config(root, droot, sroot, crop=97, arch="resnet50", epochs=1, n_sup=4, total_hack=None):
    exp = os.path.join(root, "experiments", "cityscapes", str(n_sup), "ours")
    os.makedirs(exp, exist_ok=True)
    ref = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "city_semi_template.yaml")))
    ref["dataset"]["train"].update(data_root=droot, data_list=os.path.join(sroot, "labeled.txt"),
                                   crop=dict(type="rand", size=[crop, crop]))
    ref["dataset"]["val"].update(data_root=droot, data_list=os.path.join(os.path.dirname(sroot), "val.txt"),
                                 crop=dict(type="center", size=[crop, crop]))
    ref["dataset"]["n_sup"] = 2975 - 4          # both loaders are resampled to 2975 - n_sup = 4 items (Q12)
    ref["dataset"]["workers"] = 0
    ref["trainer"]["epochs"] = epochs
    ref["criterion"]["kwargs"]["min_kept"] = 3000
    ref["net"]["sync_bn"] = False
    ref["net"]["encoder"]["type"] = f"u2pl.models.resnet.{arch}"
    ref["net"]["encoder"]["kwargs"]["pretrained"] = False
    path = os.path.join(exp, "config.yaml")
    yaml.safe_dump(ref, open(path, "w"))
    return path


if __name__ == "__main__":
    r = sys.argv[1]
    d, s = make_cityscapes(r)
    print(write_city_config(r, d, s))
