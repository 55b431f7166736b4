"""CPU tests of the `rand_rotation` / `GaussianBlur` options of the data pipeline and of batches of mixed image sizes:
builder.Pipeline against the reference's own transforms (tests/golden/augment_rot_blur.npz, written by
tools/gen_augment_golden.py), device_aug.AugmentPlan's draws against the Pipeline's, the float64 yardstick of
tests/augment_ref.py against the golden, and the loaders on a synthetic VOC set whose images differ in size."""
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_ref as A  # noqa: E402
from conftest import golden  # noqa: E402


@pytest.mark.parametrize("name", list(A.CONFIGS))
def test_pipeline_pinned_to_reference_rotation_and_blur(name):
    """builder.Pipeline == the reference's pascal_voc.build_transfrom chain with RandRotate / RandomGaussianBlur: the same
    torch calls in the same container, so image and label agree bit for bit, and so does the next random.random()"""
    from PIL import Image

    from u2pl_amd.dataset.builder import Pipeline

    g = golden("augment_rot_blur")
    assert len(g["seeds"]) >= 6
    for sd in g["seeds"]:
        random.seed(int(sd))
        oi, ol = Pipeline(A.CONFIGS[name])(Image.fromarray(g["img"]), Image.fromarray(g["lab"]))
        assert random.random() == float(g[f"{name}_next_{sd}"]), sd
        assert np.array_equal(oi.numpy(), g[f"{name}_img_{sd}"]), sd
        assert np.array_equal(ol.numpy().astype(np.uint8), g[f"{name}_lab_{sd}"]), sd


def test_blur_weights_restated_without_scipy():
    """numpy restatement of scipy.ndimage.gaussian_filter(delta5x5, sigma=1.1) == the reference's GaussianBlur(2) weight
    tensor, bit for bit; the product module does not import scipy"""
    import subprocess

    from u2pl_amd.dataset.builder import gaussian_blur_weights

    w = gaussian_blur_weights()
    ref = golden("augment_rot_blur")["blur_weight"]
    assert ref.shape == (3, 1, 5, 5) and w.dtype == np.float32
    for c in range(3):
        assert np.array_equal(w, ref[c, 0])
    code = ("import sys; sys.modules['scipy'] = None; sys.modules['scipy.ndimage'] = None\n"
            "from u2pl_amd.dataset.builder import gaussian_blur_weights as g\n"
            "print(repr(float(g()[2, 2])))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    assert float(r.stdout.strip()) == float(w[2, 2])


@pytest.mark.parametrize("name", list(A.CONFIGS) + ["none"])
def test_plan_draws_like_the_pipeline_with_options(name):
    """AugmentPlan.draw consumes python `random` exactly like the extended Pipeline and its record reproduces the
    Pipeline's output size / padding / crop origin; without an option the record is still int32[8]"""
    from PIL import Image

    from u2pl_amd.dataset.builder import Pipeline
    from u2pl_amd.dataset.device_aug import AugmentPlan

    cfg = dict(A.CONFIGS[name] if name != "none" else dict(A.BASE, rand_resize=[0.5, 2.0], flip=True),
               crop=dict(type="rand", size=[97, 113]))
    img = np.zeros((96, 150, 3), np.uint8)
    lab = np.full((96, 150), 7, np.uint8)
    blur_coins = set()
    for seed in range(12):
        random.seed(seed)
        out_img, out_lab = Pipeline(cfg)(Image.fromarray(img), Image.fromarray(lab))
        after_cpu = random.random()
        random.seed(seed)
        p = AugmentPlan(cfg).draw(96, 150)
        assert random.random() == after_cpu
        assert p.dtype == np.int32 and p.shape == ((8,) if name == "none" else (16,))
        rh, rw, flip, pt, pl, ho, wo, flags = [int(v) for v in p[:8]]
        assert tuple(out_lab.shape) == (97, 113)
        ys, xs = np.arange(97) + ho - pt, np.arange(113) + wo - pl
        inside = ((ys >= 0) & (ys < rh))[:, None] & ((xs >= 0) & (xs < rw))[None, :]
        # the crop's padding carries label 0; inside the frame the label is 7 or, where the rotation left it, 255
        assert np.array_equal(out_lab.numpy() != 0, inside), (seed, p)
        if name == "none":
            assert flags == 0
            continue
        assert (int(p[8]), int(p[9])) == (96, 150) and not p[14] and not p[15]
        assert bool(flags & 1) == ("rand_rotation" in cfg)
        blur_coins.add(bool(flags & 2))
        if flags & 1:
            m = p[10:14].view(np.float32)
            assert abs(float(m[0]) ** 2 + float(m[1]) ** 2 - 1.0) < 1e-6 and m[0] == m[3] and m[1] == -m[2]
            assert abs(np.degrees(np.arctan2(float(m[1]), float(m[0])))) <= 10.0 + 1e-4
    assert blur_coins == ({True, False} if "GaussianBlur" in cfg else ({False} if name != "none" else set()))


@pytest.mark.parametrize("name", list(A.CONFIGS))
def test_float64_yardstick_against_the_golden(name, capsys):
    """tests/augment_ref.reference (float64 rotate + blur) against the reference's float32 output: labels equal
    everywhere outside the near-boundary set, that set holds at most 1 % of the pixels, and the image differs by the
    float32 grid coordinate's error only.  e_host is printed in units of 2^-24 * max(h, w) * max|pixel|."""
    g = golden("augment_rot_blur")
    for sd in g["seeds"]:
        r = A.reference(A.CONFIGS[name], g["img"], g["lab"], int(sd))
        assert random.random() == float(g[f"{name}_next_{sd}"]), sd       # the yardstick draws like the pipeline too
        lab = g[f"{name}_lab_{sd}"].astype(np.int64)
        assert r["near"].mean() <= A.NEAR_CAP, (sd, r["near"].mean())
        assert np.array_equal(lab[~r["near"]], r["label"][~r["near"]]), sd
        if "rand_rotation" not in A.CONFIGS[name]:
            assert not r["near"].any() and np.array_equal(lab, r["label"])
        e_host = float(np.abs(g[f"{name}_img_{sd}"].astype(np.float64) - r["image"]).max())
        unit = 2.0 ** -24 * max(r["h"], r["w"]) * float(np.abs(r["image"]).max())
        with capsys.disabled():
            print(f"\n  {name} seed {sd}: e_host {e_host:.3g} = {e_host / unit:.2f} units, near {r['near'].mean() * 100:.2f} %, "
                  f"label mismatches inside the near set {int((lab != r['label']).sum())}", end="")
        # float32 grid coordinate: a few units (measured 2-3); without rotation only the 25-term float32 sum is left
        assert e_host <= (8.0 * unit if "rand_rotation" in A.CONFIGS[name] else 27 * 2.0 ** -24 * float(r["absum"].max()))


def test_ragged_collate_round_trip():
    """RawSegDataset.collate_fn packs three sizes into flat buffers: the offsets index the right bytes, every record
    carries its sample's size; equal sizes keep the stacked form"""
    from u2pl_amd.dataset.device_aug import AugmentPlan, RawSegDataset

    rng = np.random.default_rng(3)
    plan = AugmentPlan(dict(A.BASE, rand_resize=[0.5, 2.0], flip=True))
    sizes = [(40, 64), (52, 48), (33, 71)]
    samples = []
    for h, w in sizes:
        img, lab = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 21, (h, w), dtype=np.uint8)
        samples.append((torch.from_numpy(img), torch.from_numpy(lab), torch.from_numpy(plan.draw(h, w))))
    images, labels, recs, offsets = RawSegDataset.collate_fn(samples)
    assert images.dtype == labels.dtype == torch.uint8 and images.dim() == labels.dim() == 1
    assert offsets.dtype == torch.int64 and offsets.tolist() == [0, 40 * 64, 40 * 64 + 52 * 48]
    assert labels.numel() == sum(h * w for h, w in sizes) and images.numel() == 3 * labels.numel()
    assert recs.shape == (3, 16) and recs.dtype == torch.int32
    for b, (h, w) in enumerate(sizes):
        o = int(offsets[b])
        assert torch.equal(images[3 * o:3 * (o + h * w)].reshape(h, w, 3), samples[b][0])
        assert torch.equal(labels[o:o + h * w].reshape(h, w), samples[b][1])
        assert recs[b, 8:10].tolist() == [h, w] and torch.equal(recs[b, :7], samples[b][2][:7])
    stacked = RawSegDataset.collate_fn([samples[0], samples[0]])
    assert len(stacked) == 3 and stacked[0].shape == (2, 40, 64, 3) and stacked[2].shape == (2, 8)


def test_voc_loaders_with_device_aug_yield_packed_batches(tmp_path):
    """get_loader on a VOC set of mixed image sizes with dataset.device_aug: semi AND supervised branch set
    `device_plan`, train batches arrive packed (or stacked when the sizes happen to agree), val stays on the host"""
    from u2pl_amd.dataset import get_loader

    d, s = A.make_mixed_voc(str(tmp_path))
    for semi in (True, False):
        for opts in (dict(), dict(rand_rotation=[-10.0, 10.0], GaussianBlur=True)):
            cfg = dict(dataset=dict(A.voc_dataset_cfg(d, s, semi, **opts), device_aug=True))
            loaders = get_loader(cfg, seed=0)
            assert len(loaders) == (3 if semi else 2)
            for ld in loaders[:-1]:
                assert ld.device_plan.mode == (3 if opts else 0)
                packed = 0
                for batch in ld:
                    if len(batch) == 4:
                        images, labels, recs, offsets = batch
                        packed += 1
                        assert recs.shape == (4, 16) and offsets.shape == (4,) and images.numel() == 3 * labels.numel()
                        assert int(offsets[-1]) + int(recs[-1, 8]) * int(recs[-1, 9]) == labels.numel()
                    else:
                        assert batch[0].dim() == 4 and batch[2].shape[1] == (16 if opts else 8)
                assert packed > 0
            assert not hasattr(loaders[-1], "device_plan")
            img_v, lab_v = next(iter(loaders[-1]))
            assert img_v.shape[1:] == (3, 65, 65) and img_v.dtype == torch.float32


def test_host_voc_loader_with_rotation_and_blur(tmp_path):
    """the host chain serves the same options (train_sup.py / train_semi.py without device_aug)"""
    from u2pl_amd.dataset import get_loader

    d, s = A.make_mixed_voc(str(tmp_path))
    cfg = dict(dataset=A.voc_dataset_cfg(d, s, False, rand_rotation=[-10.0, 10.0], GaussianBlur=True))
    sup, _ = get_loader(cfg, seed=0)
    assert not hasattr(sup, "device_plan")
    img, lab = next(iter(sup))
    assert img.shape == (4, 3, 65, 65) and lab.dtype == torch.int64 and set(np.unique(lab.numpy())) <= set(range(21)) | {255}


@pytest.mark.parametrize("key", ["cutout", "cutmix"])
def test_dead_dataset_options_still_raise(key):
    from u2pl_amd.dataset.builder import Pipeline
    from u2pl_amd.dataset.device_aug import AugmentPlan

    cfg = dict(A.BASE, **{key: dict(n_holes=1, length=8)})
    for cls in (Pipeline, AugmentPlan):
        with pytest.raises(NotImplementedError, match="cannot unpack"):
            cls(cfg)
