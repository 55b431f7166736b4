#!/usr/bin/env python
"""Inference CLI with the reference's surface (infer.py:27-134): --config --model_path --save_folder; every image of the
validation list is resized to the input scale (769 x 769 for Cityscapes, 513 x 513 otherwise, or --input_scale H W),
run through the network once, and its prediction written to <save_folder>/gray/<file name> (class indices) and
<save_folder>/color/<file name> (Pascal colours for every dataset, as upstream: DESIGN Q14).  This project's options: --half,
the forward pass on the fp16 path; --flip / --prob, test-time fusion of the image with its mirror image / of
class probabilities instead of logits; --entropy, the softmax entropy of every pixel as an 8-bit heat map in
<save_folder>/entropy/<stem>.png (255 = log C); --drop_percent P, gray/ and color/ hold the labels as the method's own
pseudo-label rule would keep them: the P per cent lowest-entropy pixels of each image, the rest 255.
dataset.type pairs / pairs_semi: `image_path [label_path]` lines (labels are not read), input scale dataset.val.crop.size,
colours dataset.colormap (default generic), --raw_ids: gray/ in the dataset's raw label ids."""
import argparse
import os
import sys

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def get_parser():
    p = argparse.ArgumentParser(description="U2PL inference (MI355X HIP path)")
    p.add_argument("--config", type=str, default="config.yaml")
    p.add_argument("--model_path", type=str, default="checkpoints/psp_best.pth", help="evaluation model path")
    p.add_argument("--save_folder", type=str, default="viewer", help="results save folder")
    p.add_argument("--input_scale", type=int, nargs=2, default=None, metavar=("H", "W"),
                   help="network input size (default: 769 769 for Cityscapes, else 513 513)")
    return p


def get_cli_parser(fusion=False, reliability=False, raw_ids=False):
    """get_parser() keeps the reference's surface; the options only this project has are added here: --half, with
    fusion=True the test-time fusion options --flip and --prob, and with reliability=True as well (what main() parses)
    --drop_percent and --entropy, and with raw_ids=True as well (main() too) --raw_ids"""
    p = get_parser()
    p.add_argument("--half", action="store_true", default=False,
                   help="forward pass with fp16 activations and weights (u2pl_amd.half); an image whose pass saturates is "
                        "run again in fp32")
    if not fusion:
        return p
    p.add_argument("--flip", action="store_true", default=False,
                   help="test-time flip: every image also runs mirrored, the result is mirrored back and the two are averaged")
    p.add_argument("--prob", action="store_true", default=False,
                   help="fuse class probabilities (softmax per view) instead of raw logits")
    if reliability:
        p.add_argument("--drop_percent", type=float, default=None, metavar="P",
                       help="keep the P per cent lowest-entropy pixels of every image, write 255 for the rest "
                            "(trainer.unsupervised.drop_percent's meaning; P in [0, 100])")
        p.add_argument("--entropy", action="store_true", default=False,
                       help="write the per-pixel softmax entropy as an 8-bit heat map to <save_folder>/entropy/<stem>.png")
    if reliability and raw_ids:
        p.add_argument("--raw_ids", action="store_true", default=False,
                       help="write gray/ in the dataset's raw label ids (the inverse of dataset.label_map; dropped pixels get "
                            "the raw ignore value) -- paired-list dataset types only")
    return p


def main():
    from PIL import Image
    from tqdm import tqdm

    from eval import data_list, raw_id_table
    from u2pl_amd import infer as I
    from u2pl_amd.engine import load_state
    from u2pl_amd.models.model_helper import ModelBuilder

    args = get_cli_parser(fusion=True, reliability=True, raw_ids=True).parse_args()
    cfg = yaml.load(open(args.config), Loader=yaml.Loader)
    ds = cfg["dataset"]
    gray, color = os.path.join(args.save_folder, "gray"), os.path.join(args.save_folder, "color")
    os.makedirs(gray, exist_ok=True)
    os.makedirs(color, exist_ok=True)
    items = data_list(cfg)
    raw_lut = raw_id_table(cfg, args.raw_ids)
    if raw_lut is not None:
        raw_lut = torch.from_numpy(raw_lut).cuda()
    cfg["net"]["sync_bn"] = False
    model = ModelBuilder(cfg["net"])
    ck = torch.load(args.model_path, map_location="cpu")
    load_state(args.model_path, model, key="teacher_state" if "teacher_state" in ck else "model_state")
    model = model.cuda().eval()
    if ds["type"].startswith("pairs"):
        input_scale = args.input_scale or list(ds["val"]["crop"]["size"])
    else:
        input_scale = args.input_scale or ([769, 769] if "cityscapes" in ds["val"]["data_root"] else [513, 513])
    lut = torch.from_numpy(I.normalise_lut(ds["mean"], ds["std"])).cuda()
    palette = torch.from_numpy(I.dataset_colormap(ds, "pascal")).cuda()
    half = None
    if args.half:
        from u2pl_amd.half import HalfPredictor
        half = HalfPredictor(model)
    reliability = args.drop_percent is not None or args.entropy
    if not 0.0 <= (100.0 if args.drop_percent is None else args.drop_percent) <= 100.0:
        raise SystemExit("--drop_percent is a percentile in [0, 100]")
    heat_dir = os.path.join(args.save_folder, "entropy")
    if args.entropy:
        os.makedirs(heat_dir, exist_ok=True)
    dropped = []       # (ndropped device tensor, pixels) per image: read once, after the loop
    for image_path, _ in tqdm(items):
        name = image_path.split("/")[-1]
        if ds["type"].startswith("pairs"):      # any image format: index maps go to a lossless file
            name = os.path.splitext(name)[0] + ".png"
        img = torch.from_numpy(np.array(Image.open(image_path).convert("RGB"))).cuda()
        kw = dict(drop_percent=args.drop_percent, entropy=args.entropy) if reliability else {}
        if raw_lut is not None:
            kw["raw_lut"] = raw_lut
        out = I.infer_image(model, img, lut, input_scale, palette, half=half, flip=args.flip, prob=args.prob, **kw)
        label, rgb = out[:2]
        Image.fromarray(rgb.cpu().numpy()).save(os.path.join(color, name))
        Image.fromarray(label.cpu().numpy()).save(os.path.join(gray, name))
        if args.entropy:
            Image.fromarray(out[-1]["heat"].cpu().numpy()).save(os.path.join(heat_dir, os.path.splitext(name)[0] + ".png"))
        if args.drop_percent is not None:
            dropped.append((out[-1]["ndropped"], label.numel()))
    if dropped:
        counts = torch.cat([d for d, _ in dropped]).cpu().numpy()
        share = float(np.mean(counts / np.array([n for _, n in dropped], dtype=np.float64)))
        print(f" * dropped pixels (drop_percent {args.drop_percent:g}): mean share {share * 100:.2f} % over {len(dropped)} images")
    if half is not None:
        print(half.log_line())


if __name__ == "__main__":
    main()
