"""Writes tests/golden/colormaps.npz and tests/golden/infer_r50_97.npz from the reference's own code.
Needs the reference tree (oracle/ref_shim.py, which makes `.cuda()` the identity); the tests only read the stored
arrays.  Re-run:  python tools/gen_infer_golden.py

  colormaps.npz      pascal / cityscapes = what utils.create_pascal_label_colormap() / create_cityscapes_label_colormap()
                     return
  infer_r50_97.npz   two synthetic uint8 images (110 x 150 and, portrait, 140 x 96) through the reference's per-image
                     statements (infer.py:118-130) with its ModelBuilder (ResNet-50, 19 classes, aux head), the closed-form
                     weights of oracle/gen_golden.py, input_scale (97, 97) and the mean / std of
                     tools/city_semi_template.yaml.  Per image k: img_k, input_k (normalised + resized), pred_k (the
                     decoder's low-resolution logits), pred64_k (the same from a float64 copy of the model, fed input_k),
                     mask_k, color_k = colorful(mask_k, pascal map).
"""
import copy
import importlib
import importlib.util
import os
import sys
import textwrap

import numpy as np
import torch
import torch.nn.functional as F
import yaml
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402
from oracle.gen_golden import formula_state_dict  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_synth_dataset import scene  # noqa: E402

SIZES = [(110, 150), (140, 96)]
INPUT_SCALE = [97, 97]
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ref_shim.install(init_dist=False)
    utils = importlib.import_module("u2pl.utils.utils")
    model_helper = importlib.import_module("u2pl.models.model_helper")
    spec = importlib.util.spec_from_file_location("reference_infer", os.path.join(ref_shim.REFERENCE_ROOT, "infer.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    path = os.path.join(GOLDEN, "colormaps.npz")
    np.savez_compressed(path, pascal=utils.create_pascal_label_colormap(), cityscapes=utils.create_cityscapes_label_colormap())
    print(path, os.path.getsize(path), "bytes")

    tpl = yaml.safe_load(open(os.path.join(ROOT, "tools", "city_semi_template.yaml")))
    mean, std = tpl["dataset"]["mean"], tpl["dataset"]["std"]
    net = dict(
        num_classes=19, sync_bn=False, ema_decay=0.99,
        encoder=dict(type="u2pl.models.resnet.resnet50",
                     kwargs=dict(multi_grid=True, zero_init_residual=True, fpn=True,
                                 replace_stride_with_dilation=[False, True, True], pretrained=False)),
        decoder=dict(type="u2pl.models.decoder.dec_deeplabv3_plus", kwargs=dict(inner_planes=256, dilations=[12, 24, 36])),
        aux_loss=dict(aux_plane=1024, loss_weight=0.4),
    )
    model = model_helper.ModelBuilder(copy.deepcopy(net))
    model.load_state_dict(formula_state_dict(model))
    model.eval()
    m64 = model_helper.ModelBuilder(copy.deepcopy(net))
    m64.load_state_dict(formula_state_dict(m64))
    m64 = m64.double().eval()
    colormap = ref.create_pascal_label_colormap()
    STATEMENTS = open(os.path.join(ref_shim.REFERENCE_ROOT, "infer.py")).readlines()[118:130]     # infer.py:119-130
    assert "np.asarray(image)" in STATEMENTS[0] and "colorful(mask, colormap)" in STATEMENTS[-1], STATEMENTS
    rng = np.random.default_rng(11)
    fx = dict(mean=np.array(mean), std=np.array(std), input_scale=np.array(INPUT_SCALE))
    for k, (H, W) in enumerate(SIZES):
        img = scene(rng, H, W, 19)[0]
        # the reference's own per-image statements, read from its infer.py and run as they stand (the image file is
        # replaced by the array: `image` enters as what Image.open(...).convert("RGB") would return)
        seen = []
        ns = dict(np=np, torch=torch, F=F, mean=mean, std=std, input_scale=INPUT_SCALE, model=model, colormap=colormap,
                  colorful=ref.colorful, Image=Image, image=Image.fromarray(img),
                  net_process=lambda m, x: seen.append(ref.net_process(m, x)) or seen[-1])
        exec(textwrap.dedent("".join(STATEMENTS)), ns)
        image, pred, mask, color = ns["image"], seen[0], ns["mask"], np.asarray(ns["color_mask"])
        assert image.shape == (1, 3, *INPUT_SCALE) and mask.shape == (H, W) and color.shape == (H, W, 3)
        with torch.no_grad():
            pred64 = m64(image.double())["pred"]
        print(k, (H, W), "pred", tuple(pred.shape), "|pred32 - pred64| max", float((pred.double() - pred64).abs().max()),
              "scale", float(pred64.abs().max()), "classes", np.unique(mask).size)
        fx.update({f"img_{k}": img, f"input_{k}": image.numpy(), f"pred_{k}": pred.numpy(), f"pred64_{k}": pred64.numpy(),
                   f"mask_{k}": mask.astype(np.uint8), f"color_{k}": color})
    path = os.path.join(GOLDEN, "infer_r50_97.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
