"""-m gpu: `rand_rotation` / `GaussianBlur` and batches of mixed image sizes through the device-side data pipeline
(u2pl_augment_ex_u8_f32) against the host chain (builder.Pipeline) and the float64 yardstick (tests/augment_ref.py)
under the same python-`random` seed.  Every test prints its figures before it asserts."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_ref as A  # noqa: E402

CROP = dict(type="rand", size=[97, 113])
BASE = dict(mean=A.MEAN, std=A.STD, ignore_label=255, crop=CROP)
ROT = dict(rand_rotation=[-10.0, 10.0])
CONFIGS = dict(
    rot=dict(BASE, **ROT),
    rot_blur=dict(BASE, GaussianBlur=True, **ROT),
    all=dict(BASE, GaussianBlur=True, rand_resize=[0.5, 2.0], flip=True, **ROT),
    blur=dict(BASE, GaussianBlur=True),
    blur_resize_flip=dict(BASE, GaussianBlur=True, rand_resize=[0.5, 2.0], flip=True),
)


def sample(seed, labels_to=19):
    """sizes that force padding in some cases: a third of the seeds is lower than the 97-row crop"""
    rng = np.random.default_rng(seed)
    H, W = 96 + 8 * (seed % 3), 150
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lab = rng.integers(0, labels_to, (H, W), dtype=np.uint8)
    return img, lab


def device_pipeline(cfg, samples, seed, packed=False):
    """the device chain on a list of (img, lab) under `seed` -> image (B,3,Sh,Sw), label (B,Sh,Sw) numpy, records"""
    from u2pl_amd.dataset.device_aug import AugmentPlan, RawSegDataset, augment_batch

    plan = AugmentPlan(cfg)
    random.seed(seed)
    items = [(torch.from_numpy(i), torch.from_numpy(l), torch.from_numpy(plan.draw(*l.shape))) for i, l in samples]
    batch = RawSegDataset.collate_fn(items)
    assert len(batch) == (4 if packed else 3)
    out, lab = augment_batch(plan, *batch, device=DEV)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lab.cpu().numpy(), batch[2].numpy()


@pytest.mark.parametrize("name", ["rot", "rot_blur", "all"])
@pytest.mark.parametrize("seed", range(8))
def test_rotation_against_host_and_float64(name, seed):
    cfg = CONFIGS[name]
    img, lab = sample(seed)
    host_img, host_lab, nxt = A.host_pipeline(cfg, img, lab, 100 + seed)
    ref = A.reference(cfg, img, lab, 100 + seed)
    out, ol, rec = device_pipeline(cfg, [(img, lab)], 100 + seed)
    assert random.random() == nxt                      # both consume the RNG stream identically
    near = ref["near"]
    e_host = float(np.abs(host_img.astype(np.float64) - ref["image"]).max())
    e_dev = float(np.abs(out[0].astype(np.float64) - ref["image"]).max())
    print(f"{name} seed {seed}: record {rec[0, :10].tolist()} blurred {ref['blurred']} padding {int(ref['padding'].sum())} px, "
          f"near {near.mean() * 100:.2f} %, label mismatches outside near {int((ol[0] != host_lab)[~near].sum())} "
          f"inside {int((ol[0] != host_lab)[near].sum())}, e_host {e_host:.3g} e_dev {e_dev:.3g}")
    assert near.mean() <= A.NEAR_CAP
    assert np.array_equal(ol[0][~near], host_lab[~near])
    assert e_dev <= 2 * e_host + 1e-6


@pytest.mark.parametrize("name", ["blur", "blur_resize_flip"])
@pytest.mark.parametrize("seed", range(8))
def test_blur_against_host_and_float64(name, seed):
    cfg = CONFIGS[name]
    img, lab = sample(seed)
    host_img, host_lab, nxt = A.host_pipeline(cfg, img, lab, 200 + seed)
    ref = A.reference(cfg, img, lab, 200 + seed)
    out, ol, rec = device_pipeline(cfg, [(img, lab)], 200 + seed)
    assert random.random() == nxt
    err = np.abs(out[0].astype(np.float64) - ref["image"])
    bound = 2e-6 + 27 * 2.0 ** -24 * ref["absum"]       # pre-blur tolerance + a 25-term float32 sum in any order
    print(f"{name} seed {seed}: record {rec[0, :10].tolist()} blurred {ref['blurred']}, label mismatches "
          f"{int((ol[0] != host_lab).sum())}, max err {err.max():.3g}, max err / bound {(err / bound).max():.3f}, "
          f"host err {np.abs(host_img - ref['image']).max():.3g}")
    assert bool(rec[0, 7] & 2) == ref["blurred"]
    assert np.array_equal(ol[0], host_lab)
    assert (err <= bound).all()


def test_padding_stays_zero_under_blur_and_rotated_out_corners():
    # blur + rotation on an image lower AND narrower than the crop: the crop's padding is exact zeros / label 0
    cfg = dict(CONFIGS["rot_blur"], crop=dict(type="center", size=[97, 113]))
    rng = np.random.default_rng(5)
    img, lab = rng.integers(1, 256, (80, 100, 3), dtype=np.uint8), rng.integers(1, 19, (80, 100), dtype=np.uint8)
    blurred = 0
    for seed in range(6):
        ref = A.reference(cfg, img, lab, seed)
        out, ol, _ = device_pipeline(cfg, [(img, lab)], seed)
        pad = ref["padding"]
        print(f"seed {seed}: blurred {ref['blurred']}, padding {int(pad.sum())} px, max |image| there "
              f"{np.abs(out[0][:, pad]).max()}, labels there {np.unique(ol[0][pad]).tolist()}")
        assert pad.sum() == 97 * 113 - 80 * 100
        assert (out[0][:, pad] == 0.0).all() and (ol[0][pad] == 0).all()
        assert (ol[0][~pad] != 0).all()                 # source labels are 1..18, rotated-out pixels 255
        blurred += ref["blurred"]
    assert 0 < blurred < 6
    # rotation alone, 8 to 10 degrees: where all four bilinear taps leave the frame the image is exactly 0.0 and the
    # label is ignore_label (the crop is the whole 104 x 150 frame, so the four corners are in it)
    cfg = dict(BASE, rand_rotation=[8.0, 10.0], crop=dict(type="center", size=[104, 150]))
    img, lab = sample(1, labels_to=19)
    ref = A.reference(cfg, img, lab, 3)
    out, ol, _ = device_pipeline(cfg, [(img, lab)], 3)
    gone = (ref["image"] == 0.0).all(0) & (ref["label"] == 255) & ~ref["near"] & ~ref["padding"]
    print(f"rotated-out pixels in the crop: {int(gone.sum())}")
    assert gone.sum() > 100
    assert (out[0][:, gone] == 0.0).all() and (ol[0][gone] == 255).all()


def test_ragged_batch_options_off_and_dense_bit_identity():
    from u2pl_amd._lib import call
    from u2pl_amd.dataset.device_aug import AugmentPlan, augment_batch, widen

    cfg = dict(BASE, rand_resize=[0.5, 2.0], flip=True)
    rng = np.random.default_rng(11)
    samples = []
    for h, w in ((96, 150), (120, 131), (77, 201)):
        samples.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 21, (h, w), dtype=np.uint8)))
    out, ol, rec = device_pipeline(cfg, samples, 7, packed=True)
    after = random.random()
    random.seed(7)
    from PIL import Image

    from u2pl_amd.dataset.builder import Pipeline
    for b, (img, lab) in enumerate(samples):
        hi, hl = Pipeline(cfg)(Image.fromarray(img), Image.fromarray(lab))
        err = float(np.abs(out[b] - hi.numpy()).max())
        print(f"ragged sample {b}: record {rec[b, :10].tolist()} label mismatches {int((ol[b] != hl.numpy()).sum())} max err {err:.3g}")
        assert np.array_equal(ol[b], hl.numpy())
        assert err < 2e-6
    assert random.random() == after
    # a dense equal-size batch: the new entry point (dense AND with an offset table) gives the bits of u2pl_augment_u8_f32
    plan = AugmentPlan(cfg)
    imgs = torch.from_numpy(rng.integers(0, 256, (3, 104, 150, 3), dtype=np.uint8)).to(DEV)
    labs = torch.from_numpy(rng.integers(0, 21, (3, 104, 150), dtype=np.uint8)).to(DEV)
    random.seed(21)
    params = torch.stack([torch.from_numpy(plan.draw(104, 150)) for _ in range(3)])
    old_img, old_lab = augment_batch(plan, imgs, labs, params)
    wide = widen(params, 104, 150).to(DEV)
    offsets = (torch.arange(3, dtype=torch.int64) * 104 * 150).to(DEV)
    for off, H, W in ((None, 104, 150), (offsets, 0, 0)):
        new_img = torch.full_like(old_img, float("nan"))
        new_lab = torch.full_like(old_lab, -1)
        call("u2pl_augment_ex_u8_f32", imgs, labs, off, wide, 3, H, W, 97, 113, 255, 0, plan.mean.ctypes.data,
             plan.std.ctypes.data, None, None, new_img, new_lab)
        torch.cuda.synchronize()
        print("dense batch, offsets", off is not None, ": image bits equal", torch.equal(new_img, old_img), "labels equal",
              torch.equal(new_lab, old_lab))
        assert torch.equal(new_img.view(torch.int32), old_img.view(torch.int32)) and torch.equal(new_lab, old_lab)


def _run(script, cfg):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--config", cfg, "--seed", "2"], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def _voc_config(tmp_path, semi, **options):
    import make_synth_dataset as M

    d, s = A.make_mixed_voc(str(tmp_path))
    cfgp = M.write_city_config(str(tmp_path), d, s, crop=97, epochs=1)
    cfg = yaml.load(open(cfgp), Loader=yaml.Loader)
    cfg["dataset"] = dict(A.voc_dataset_cfg(d, s, semi, crop=97, batch_size=2, **options), device_aug=True)
    cfg["net"]["num_classes"] = 21
    if not semi:
        cfg["net"]["decoder"]["kwargs"]["rep_head"] = False
        for k in ("unsupervised", "contrastive"):
            cfg["trainer"].pop(k)
    yaml.safe_dump(cfg, open(cfgp, "w"))
    return cfgp


def test_train_semi_cli_on_mixed_size_voc_with_rotation_and_blur(tmp_path):
    out = _run("train_semi.py", _voc_config(tmp_path, True, rand_rotation=[-10.0, 10.0], GaussianBlur=True))
    assert "mIoU" in out


def test_train_sup_cli_with_device_side_data_pipeline(tmp_path):
    out = _run("train_sup.py", _voc_config(tmp_path, False))
    assert "mIoU" in out
