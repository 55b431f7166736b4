#!/usr/bin/env python
"""Evaluation CLI with the reference's surface (eval.py:26-156): --config --model_path --base_size --scales
--save_folder --crop; Cityscapes lists -> sliding-window evaluation, VOC lists -> whole-image evaluation.  Every
prediction is written to <save_folder>/gray/<name>.png and, in the dataset's colours, <save_folder>/color/<name>.png.
This project's options: --half, the forward passes on the fp16 path; --flip / --prob, test-time fusion of every
window (a mirrored view, class probabilities instead of logits) -- with --scales this is "ms+flip";
--entropy, the softmax entropy of the summed scores as an 8-bit heat map in <save_folder>/entropy/<name>.png; --drop_percent P,
gray/ and color/ keep the P per cent lowest-entropy pixels of each image (the rest 255) and the mIoU on the reliable and on the
unreliable pixels is printed next to the usual one.  dataset.type pairs / pairs_semi: the list holds
`image_path [label_path]` lines, the ground truth goes through dataset.label_map, colours are dataset.colormap (default
generic), and --raw_ids writes gray/ in the dataset's raw ids; the mIoU is always computed in class space."""
import argparse
import os
import sys

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def get_parser():
    p = argparse.ArgumentParser(description="U2PL evaluation (MI355X HIP path)")
    p.add_argument("--base_size", type=int, default=2048)
    p.add_argument("--scales", type=float, default=[1.0], nargs="+")
    p.add_argument("--config", type=str, default="config.yaml")
    p.add_argument("--model_path", type=str, default="checkpoints/ckpt_best.pth")
    p.add_argument("--save_folder", type=str, default="checkpoints/results/")
    p.add_argument("--names_path", type=str, default="")
    p.add_argument("--crop", action="store_true", default=False)
    return p


def get_cli_parser(fusion=False, reliability=False, raw_ids=False):
    """get_parser() keeps the reference's surface; the options only this project has are added here: --half, with
    fusion=True the test-time fusion options --flip and --prob, and with reliability=True as well (what main() parses)
    --drop_percent and --entropy, and with raw_ids=True as well (main() too) --raw_ids"""
    p = get_parser()
    p.add_argument("--half", action="store_true", default=False,
                   help="forward passes with fp16 activations and weights (u2pl_amd.half); a pass that saturates is "
                        "recomputed in fp32")
    if not fusion:
        return p
    p.add_argument("--flip", action="store_true", default=False,
                   help="test-time flip: every window also runs mirrored, the result is mirrored back and the two are averaged")
    p.add_argument("--prob", action="store_true", default=False,
                   help="fuse class probabilities (softmax per view) instead of raw logits, per window and scale")
    if reliability:
        p.add_argument("--drop_percent", type=float, default=None, metavar="P",
                       help="keep the P per cent lowest-entropy pixels of every image, write 255 for the rest, and report "
                            "the mIoU on reliable and unreliable pixels (trainer.unsupervised.drop_percent's meaning)")
        p.add_argument("--entropy", action="store_true", default=False,
                       help="write the per-pixel softmax entropy as an 8-bit heat map to <save_folder>/entropy/<name>.png")
    if reliability and raw_ids:
        p.add_argument("--raw_ids", action="store_true", default=False,
                       help="write gray/ in the dataset's raw label ids (the inverse of dataset.label_map; dropped pixels get "
                            "the raw ignore value) -- paired-list dataset types only")
    return p


def raw_id_table(cfg, raw_ids):
    """--raw_ids -> the (256,) uint8 table class -> raw id of the config's label_map, or None without the option"""
    if not raw_ids:
        return None
    ds = cfg["dataset"]
    if not ds["type"].startswith("pairs"):
        raise SystemExit(f"--raw_ids needs a dataset.label_map, which dataset.type {ds['type']} does not have (types pairs / "
                         "pairs_semi do)")
    from u2pl_amd.dataset.builder import build_label_lut, raw_id_lut

    return raw_id_lut(build_label_lut(ds, cfg["net"]["num_classes"]), ds.get("ignore_label", 255))


def data_list(cfg):
    d = cfg["dataset"]["val"]
    root, out = d["data_root"], []
    if cfg["dataset"]["type"].startswith("pairs"):     # `image_path [label_path]` (no label: None)
        from u2pl_amd.dataset.builder import parse_pairs

        return [[os.path.join(root, ip), None if lp is None else os.path.join(root, lp)] for ip, lp in parse_pairs(d["data_list"])]
    for line in open(d["data_list"]):
        line = line.strip()
        if not line:
            continue
        if "cityscapes" in root:
            arr = [line, "gtFine/" + line[12:-15] + "gtFine_labelTrainIds.png"]
        else:
            arr = [f"JPEGImages/{line}.jpg", f"SegmentationClassAug/{line}.png"]
        out.append([os.path.join(root, a) for a in arr])
    return out


def main():
    from PIL import Image

    from u2pl_amd import evaluate as E
    from u2pl_amd.engine import load_state
    from u2pl_amd.infer import dataset_colormap
    from u2pl_amd.models.model_helper import ModelBuilder

    args = get_cli_parser(fusion=True, reliability=True, raw_ids=True).parse_args()
    cfg = yaml.load(open(args.config), Loader=yaml.Loader)
    ds = cfg["dataset"]
    mean, std = np.asarray(ds["mean"], np.float32), np.asarray(ds["std"], np.float32)
    classes = cfg["net"]["num_classes"]
    crop = ds["val"]["crop"]["size"]
    gray, color = os.path.join(args.save_folder, "gray"), os.path.join(args.save_folder, "color")
    os.makedirs(gray, exist_ok=True)
    os.makedirs(color, exist_ok=True)
    items = data_list(cfg)
    pairs = ds["type"].startswith("pairs")
    raw_lut = raw_id_table(cfg, args.raw_ids)
    label_lut = None
    if pairs:
        from u2pl_amd.dataset.builder import build_label_lut, read_label

        label_lut = build_label_lut(ds, classes)
        missing = [ip for ip, lp in items if lp is None]
        if missing:
            raise SystemExit(f"evaluation needs a label for every image: {missing[0]} has none (infer.py takes such lists)")
    cfg["net"]["sync_bn"] = False
    model = ModelBuilder(cfg["net"])
    ck = torch.load(args.model_path, map_location="cpu")
    load_state(args.model_path, model, key="teacher_state" if "teacher_state" in ck else "model_state")
    model = model.cuda()
    half = None
    if args.half:
        from u2pl_amd.half import HalfPredictor
        half = HalfPredictor(model.eval())

    def samples():
        for ip, lp in items:
            img = (np.asarray(Image.open(ip).convert("RGB")).astype(np.float32) - mean) / std
            if pairs:      # ground truth in class space, like the val loader's
                yield torch.from_numpy(img).permute(2, 0, 1).contiguous(), label_lut[read_label(lp)]
                continue
            yield torch.from_numpy(img).permute(2, 0, 1).contiguous(), np.asarray(Image.open(lp).convert("L")).astype(np.uint8)

    if not 0.0 <= (100.0 if args.drop_percent is None else args.drop_percent) <= 100.0:
        raise SystemExit("--drop_percent is a percentile in [0, 100]")
    heat_dir = os.path.join(args.save_folder, "entropy")
    if args.entropy:
        os.makedirs(heat_dir, exist_ok=True)

    def dump(i, pred, rgb, heat=None):
        name = os.path.basename(items[i][0]).split(".")[0] + ".png"
        Image.fromarray(pred).save(os.path.join(gray, name))
        Image.fromarray(rgb).save(os.path.join(color, name))
        if heat is not None:
            Image.fromarray(heat).save(os.path.join(heat_dir, name))

    city = "cityscapes" in ds["type"]
    kw = {}
    if args.drop_percent is not None or args.entropy:
        kw = dict(drop_percent=args.drop_percent, entropy=args.entropy)
    if raw_lut is not None:
        kw["raw_lut"] = raw_lut
    miou, iou, *rel = E.evaluate(model, samples(), classes, args.base_size, crop, args.scales, use_crop=city or args.crop,
                                 ignore=ds.get("ignore_label", 255), on_prediction=dump,
                                 palette=dataset_colormap(ds, "cityscapes" if city else "pascal"), half=half, flip=args.flip,
                                 prob=args.prob, **kw)
    for c, v in enumerate(iou):
        print(f" * class [{c}] IoU {v * 100:.2f}")
    print(f" * mIoU {miou * 100:.2f}")
    if rel:
        print(f" * mIoU reliable ({args.drop_percent:g}) {rel[0]['miou_reliable'] * 100:.2f}")
        print(f" * mIoU unreliable {rel[0]['miou_unreliable'] * 100:.2f}")
        print(f" * coverage {rel[0]['coverage'] * 100:.2f}")
    if half is not None:
        print(half.log_line())


if __name__ == "__main__":
    main()
