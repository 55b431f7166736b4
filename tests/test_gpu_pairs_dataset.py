"""-m gpu: dataset.label_map on the device data pipeline (u2pl_augment_lut_u8_f32: the label table fused into the one read of
a source label byte), the byte-table kernel behind --raw_ids (u2pl_lut_u8), and the command lines on a paired-list
dataset with 40 classes, palette label files and mixed image sizes.  The oracle is the host chain -- builder.Pipeline on
the label array mapped with numpy first -- and, for rotation and blur, the float64 yardstick tests/augment_ref.py with
the bounds of tests/test_gpu_augment_options.py.  Every test prints its figures before it asserts."""
import os
import random
import re
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

C_ADE = 150
ADE = dict(ignore_label=255, label_map=dict(offset=-1))
CROP = dict(type="rand", size=[97, 113])
BASE = dict(mean=A.MEAN, std=A.STD, ignore_label=255, crop=CROP)
ROT = dict(rand_rotation=[-10.0, 10.0])
CONFIGS = dict(
    plain=dict(BASE, rand_resize=[0.5, 2.0], flip=True),
    rot=dict(BASE, **ROT),
    rot_blur=dict(BASE, GaussianBlur=True, **ROT),
    all=dict(BASE, GaussianBlur=True, rand_resize=[0.5, 2.0], flip=True, **ROT),
    blur_resize_flip=dict(BASE, GaussianBlur=True, rand_resize=[0.5, 2.0], flip=True),
)
RAGGED = ((96, 150), (120, 131), (77, 201))


def ade_lut():
    from u2pl_amd.dataset.builder import build_label_lut

    return build_label_lut(ADE, C_ADE)


def sample(seed, lo=0, hi=256, size=None):
    """the sizes of tests/test_gpu_augment_options.py (a third of the seeds is lower than the 97-row crop); RAW labels from
    the whole byte range"""
    rng = np.random.default_rng(seed)
    H, W = size or (96 + 8 * (seed % 3), 150)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(lo, hi, (H, W), dtype=np.uint8)


def device_pipeline(cfg, samples, seed, lut):
    """the device chain with a label table on a list of (img, RAW lab) under `seed` -> image, label (numpy), records"""
    from u2pl_amd.dataset.device_aug import AugmentPlan, RawSegDataset, augment_batch

    plan = AugmentPlan(cfg, lut=lut)
    random.seed(seed)
    items = [(torch.from_numpy(i), torch.from_numpy(l), torch.from_numpy(plan.draw(*l.shape))) for i, l in samples]
    batch = RawSegDataset.collate_fn(items)
    out, lab = augment_batch(plan, *batch, device=DEV)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lab.cpu().numpy(), batch[2].numpy()


def invariant(lab, C=C_ADE):
    return bool(((lab < C) | (lab == 255)).all()) and bool((lab >= 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# identity table: the new entry point gives the bits of the old ones
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense_plain", "dense_rot", "dense_rot_blur", "packed_plain", "packed_all"])
def test_identity_table_gives_the_bits_of_the_old_entry_points(layout):
    from u2pl_amd._lib import HipError, call
    from u2pl_amd.dataset.device_aug import AugmentPlan, RawSegDataset, widen

    kind, name = layout.split("_", 1)
    cfg = CONFIGS[name]
    plan = AugmentPlan(cfg)
    sizes = RAGGED if kind == "packed" else ((104, 150),) * 3
    random.seed(21)
    items = []
    for b, (h, w) in enumerate(sizes):
        img, lab = sample(40 + b, size=(h, w))
        items.append((torch.from_numpy(img), torch.from_numpy(lab), torch.from_numpy(plan.draw(h, w))))
    batch = RawSegDataset.collate_fn(items)
    imgs, labs, rec = batch[0].to(DEV), batch[1].to(DEV), batch[2]
    off = batch[3].to(DEV) if kind == "packed" else None
    H, W = (0, 0) if kind == "packed" else sizes[0]
    wide = (widen(rec, H, W) if rec.shape[1] == 8 else rec).to(DEV)
    B, (Sh, Sw) = len(sizes), plan.out_size()
    wts, scratch = plan._device_buffers(torch.device(DEV, 0), B) if plan.mode & 2 else (None, None)
    ident = torch.arange(256, dtype=torch.uint8, device=DEV)
    ade = torch.from_numpy(ade_lut()).to(DEV)

    def run(entry, *table):
        oi = torch.full((B, 3, Sh, Sw), float("nan"), dtype=torch.float32, device=DEV)
        ol = torch.full((B, Sh, Sw), -1, dtype=torch.int64, device=DEV)
        call(entry, imgs, labs, off, wide, B, H, W, Sh, Sw, 255, plan.mode, *table, plan.mean.ctypes.data,
             plan.std.ctypes.data, wts, scratch, oi, ol)
        torch.cuda.synchronize()
        return oi, ol

    old_img, old_lab = run("u2pl_augment_ex_u8_f32")
    new_img, new_lab = run("u2pl_augment_lut_u8_f32", ident)
    ade_img, ade_lab = run("u2pl_augment_lut_u8_f32", ade)
    print(f"{layout}: mode {plan.mode}, image bits equal {torch.equal(new_img.view(torch.int32), old_img.view(torch.int32))}, "
          f"labels equal {torch.equal(new_lab, old_lab)}, distinct labels {old_lab.unique().numel()}")
    assert not torch.isnan(old_img).any() and old_lab.min() >= 0
    assert torch.equal(new_img.view(torch.int32), old_img.view(torch.int32)) and torch.equal(new_lab, old_lab)
    assert torch.equal(ade_img.view(torch.int32), old_img.view(torch.int32))     # the table never touches the image
    assert invariant(ade_lab.cpu().numpy())
    if layout == "dense_plain":
        o8 = torch.full_like(old_img, float("nan"))
        l8 = torch.full_like(old_lab, -1)
        call("u2pl_augment_u8_f32", imgs, labs, rec.to(DEV), B, H, W, Sh, Sw, plan.mean.ctypes.data, plan.std.ctypes.data, o8, l8)
        torch.cuda.synchronize()
        assert torch.equal(new_img.view(torch.int32), o8.view(torch.int32)) and torch.equal(new_lab, l8)
        with pytest.raises(HipError, match="1001"):
            run("u2pl_augment_lut_u8_f32", None)


# ---------------------------------------------------------------------------------------------------------------------
# ADE-style table (offset -1, 150 classes), raw labels from the whole byte range, against the host chain
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_ade_table_without_options_equals_the_host_chain(seed):
    lut = ade_lut()
    cfg = CONFIGS["plain"]
    img, raw = sample(seed)
    host_img, host_lab, nxt = A.host_pipeline(cfg, img, lut[raw], 100 + seed)
    out, ol, rec = device_pipeline(cfg, [(img, raw)], 100 + seed, lut)
    assert random.random() == nxt                       # both consume the RNG stream identically
    err = float(np.abs(out[0] - host_img).max())
    print(f"plain seed {seed}: record {rec[0, :8].tolist()} label mismatches {int((ol[0] != host_lab).sum())} max err {err:.3g}")
    assert np.array_equal(ol[0], host_lab)
    assert err < 2e-6
    assert invariant(ol[0])


@pytest.mark.parametrize("name", ["rot", "all"])
@pytest.mark.parametrize("seed", range(8))
def test_ade_table_with_rotation_equals_the_host_chain(name, seed):
    lut = ade_lut()
    cfg = CONFIGS[name]
    img, raw = sample(seed)
    host_img, host_lab, nxt = A.host_pipeline(cfg, img, lut[raw], 100 + seed)
    ref = A.reference(cfg, img, lut[raw], 100 + seed)
    out, ol, rec = device_pipeline(cfg, [(img, raw)], 100 + seed, lut)
    assert random.random() == nxt
    near = ref["near"]
    e_host = float(np.abs(host_img.astype(np.float64) - ref["image"]).max())
    e_dev = float(np.abs(out[0].astype(np.float64) - ref["image"]).max())
    print(f"{name} seed {seed}: record {rec[0, :10].tolist()} blurred {ref['blurred']} near {near.mean() * 100:.2f} %, label "
          f"mismatches vs host outside near {int((ol[0] != host_lab)[~near].sum())} inside {int((ol[0] != host_lab)[near].sum())}, "
          f"vs float64 {int((ol[0] != ref['label']).sum())}, e_host {e_host:.3g} e_dev {e_dev:.3g}")
    assert near.mean() <= A.NEAR_CAP
    assert np.array_equal(ol[0], host_lab)
    assert e_dev <= 2 * e_host + 1e-6
    assert invariant(ol[0])


@pytest.mark.parametrize("seed", range(8))
def test_ade_table_with_blur_equals_the_host_chain(seed):
    lut = ade_lut()
    cfg = CONFIGS["blur_resize_flip"]
    img, raw = sample(seed)
    host_img, host_lab, nxt = A.host_pipeline(cfg, img, lut[raw], 200 + seed)
    ref = A.reference(cfg, img, lut[raw], 200 + seed)
    out, ol, rec = device_pipeline(cfg, [(img, raw)], 200 + seed, lut)
    assert random.random() == nxt
    err = np.abs(out[0].astype(np.float64) - ref["image"])
    bound = 2e-6 + 27 * 2.0 ** -24 * ref["absum"]       # pre-blur tolerance + a 25-term float32 sum in any order
    print(f"blur seed {seed}: record {rec[0, :10].tolist()} blurred {ref['blurred']}, label mismatches "
          f"{int((ol[0] != host_lab).sum())}, max err {err.max():.3g}, max err / bound {(err / bound).max():.3f}")
    assert np.array_equal(ol[0], host_lab)
    assert (err <= bound).all()
    assert invariant(ol[0])


def test_ade_table_on_a_packed_batch_equals_the_host_chain():
    from PIL import Image

    from u2pl_amd.dataset.builder import Pipeline

    lut = ade_lut()
    cfg = CONFIGS["plain"]
    samples = [sample(60 + b, size=s) for b, s in enumerate(RAGGED)]
    out, ol, rec = device_pipeline(cfg, samples, 7, lut)
    assert rec.shape == (3, 16)
    after = random.random()
    random.seed(7)
    for b, (img, raw) in enumerate(samples):
        hi, hl = Pipeline(cfg)(Image.fromarray(img), Image.fromarray(lut[raw]))
        err = float(np.abs(out[b] - hi.numpy()).max())
        print(f"packed sample {b}: record {rec[b, :10].tolist()} label mismatches {int((ol[b] != hl.numpy()).sum())} max err {err:.3g}")
        assert np.array_equal(ol[b], hl.numpy())
        assert err < 2e-6
    assert random.random() == after
    assert invariant(ol)


def test_padding_is_class_0_and_rotated_out_pixels_are_ignore_label():
    lut = ade_lut()
    assert lut[0] == 255
    # an image lower AND narrower than the crop, blur + rotation: the border is label 0 (not lut[0] = 255), image 0.0
    cfg = dict(CONFIGS["rot_blur"], crop=dict(type="center", size=[80, 120]))
    img, raw = sample(5, lo=2, hi=256, size=(64, 100))          # raw 1 (class 0) does not occur inside the frame
    for seed in range(3):
        ref = A.reference(cfg, img, lut[raw], seed)
        out, ol, _ = device_pipeline(cfg, [(img, raw)], seed, lut)
        pad = ref["padding"]
        print(f"seed {seed}: blurred {ref['blurred']}, padding {int(pad.sum())} px, labels there {np.unique(ol[0][pad]).tolist()}")
        assert pad.sum() == 80 * 120 - 64 * 100
        assert (out[0][:, pad] == 0.0).all() and (ol[0][pad] == 0).all()
        assert (ol[0][~pad] != 0).all() and invariant(ol[0])
    # the same without options, through the table entry's option-free kernel (a dense batch of 3)
    cfg = dict(BASE, crop=dict(type="center", size=[80, 120]))
    samples = [sample(70 + b, lo=2, hi=256, size=(64, 100)) for b in range(3)]
    out, ol, _ = device_pipeline(cfg, samples, 0, lut)
    pad = np.ones((80, 120), bool)
    pad[8:72, 10:110] = False
    for b, (img, raw) in enumerate(samples):
        assert (ol[b][pad] == 0).all() and (out[b][:, pad] == 0.0).all()
        assert np.array_equal(ol[b][8:72, 10:110], lut[raw].astype(np.int64))
    # rotation alone, 8 to 10 degrees, the crop is the whole frame: out-of-frame pixels are ignore_label
    cfg = dict(BASE, rand_rotation=[8.0, 10.0], crop=dict(type="center", size=[104, 150]))
    img, raw = sample(1, lo=1, hi=151)                           # every source label has a class: 255 only from rotation
    ref = A.reference(cfg, img, lut[raw], 3)
    out, ol, _ = device_pipeline(cfg, [(img, raw)], 3, lut)
    gone = (ref["image"] == 0.0).all(0) & (ref["label"] == 255) & ~ref["near"] & ~ref["padding"]
    print(f"rotated-out pixels in the crop: {int(gone.sum())}, 255 elsewhere {int(((ol[0] == 255) & ~gone & ~ref['near']).sum())}")
    assert gone.sum() > 100
    assert (out[0][:, gone] == 0.0).all() and (ol[0][gone] == 255).all()
    assert invariant(ol[0])


# ---------------------------------------------------------------------------------------------------------------------
# u2pl_lut_u8
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4097, 97 * 113])
@pytest.mark.parametrize("src_off", [0, 1, 3])
def test_lut_u8_any_length_any_alignment_and_in_place(n, src_off):
    from u2pl_amd import hipops as H

    rng = np.random.default_rng(n + src_off)
    lut = rng.permutation(256).astype(np.uint8)
    host = rng.integers(0, 256, n + 64, dtype=np.uint8)
    want = lut[host[src_off:src_off + n]]
    lut_d = torch.from_numpy(lut).to(DEV)
    for dst_off in (0, 2, 4, src_off):                   # 16-byte, byte and dword stores; aligned like the source
        src = torch.from_numpy(host).to(DEV)
        dst = torch.full((n + 64,), 7, dtype=torch.uint8, device=DEV)
        H.lut_u8(src[src_off:src_off + n], lut_d, out=dst[dst_off:dst_off + n])
        got = dst.cpu().numpy()
        assert np.array_equal(got[dst_off:dst_off + n], want), (n, src_off, dst_off)
        assert (got[:dst_off] == 7).all() and (got[dst_off + n:] == 7).all()      # nothing written outside
        assert np.array_equal(src.cpu().numpy(), host)
    buf = torch.from_numpy(host).to(DEV)
    out = H.lut_u8(buf[src_off:src_off + n], lut_d)      # in place
    got = buf.cpu().numpy()
    assert out.data_ptr() == buf.data_ptr() + src_off
    assert np.array_equal(got[src_off:src_off + n], want)
    assert np.array_equal(got[:src_off], host[:src_off]) and np.array_equal(got[src_off + n:], host[src_off + n:])


def test_lut_u8_rejects_bad_arguments():
    from u2pl_amd import _lib
    from u2pl_amd import hipops as H

    x = torch.zeros(16, dtype=torch.uint8, device=DEV)
    lut = torch.arange(256, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.HipError):
        H.lut_u8(x, lut[:255])
    with pytest.raises(_lib.HipError):
        H.lut_u8(x.cpu(), lut)
    with pytest.raises(_lib.HipError, match="1001"):
        _lib.call("u2pl_lut_u8", x, x, 16, None)


# ---------------------------------------------------------------------------------------------------------------------
# command lines: 40 classes (the wide loss route, from real files), palette label files stored as class + 1, mixed sizes
# ---------------------------------------------------------------------------------------------------------------------
C_CLI = 40


def _run(script, cfg, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--config", cfg, *extra], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def _pairs(root, **kw):
    import make_synth_dataset as M

    d, s = M.make_pairs(str(root), H=110, W=150, C=C_CLI, raw_offset=1, palette_png=True, mixed_sizes=True)
    return d, s, M.write_pairs_config(str(root), d, s, C=C_CLI, crop=97, arch="resnet50", epochs=1, **kw)


def _finite_losses(text):
    m = re.findall(r"Sup (\S+) Uns (\S+) Con (\S+) LR", text)
    assert m, text[-2000:]
    vals = np.array(m, dtype=np.float64)
    print("losses", vals.tolist())
    assert np.isfinite(vals).all()


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """train_semi.py for one epoch with the device-side data pipeline -> (data root, list dir, config, output, ckpt)"""
    root = tmp_path_factory.mktemp("pairs_semi")
    d, s, cfgp = _pairs(root, device_aug=True)
    from PIL import Image
    assert Image.open(os.path.join(d, "labels", "labeled_0000.png")).mode == "P"
    assert len({Image.open(os.path.join(d, "images", f"labeled_{i:04d}.jpg")).size for i in range(4)}) > 1
    text = _run("train_semi.py", cfgp, "--seed", "2")
    return d, s, cfgp, text, os.path.join(os.path.dirname(cfgp), "checkpoints", "ckpt.pth")


def test_train_semi_cli_on_pairs_with_the_device_pipeline(trained):
    _, _, _, text, ckpt = trained
    assert "mIoU" in text
    _finite_losses(text)
    ck = torch.load(ckpt, map_location="cpu")
    assert ck["epoch"] == 1 and set(ck) >= {"model_state", "teacher_state", "best_miou"}


def test_train_semi_cli_on_pairs_with_the_host_chain(tmp_path):
    _, _, cfgp = _pairs(tmp_path, device_aug=False)
    text = _run("train_semi.py", cfgp, "--seed", "2")
    assert "mIoU" in text
    _finite_losses(text)
    assert os.path.exists(os.path.join(os.path.dirname(cfgp), "checkpoints", "ckpt.pth"))


def test_train_sup_cli_on_pairs(tmp_path):
    _, _, cfgp = _pairs(tmp_path, semi=False, device_aug=True)
    assert yaml.safe_load(open(cfgp))["dataset"]["type"] == "pairs"
    assert "mIoU" in _run("train_sup.py", cfgp, "--seed", "2")


def test_eval_cli_on_pairs_class_ids_and_raw_ids(trained, tmp_path):
    from PIL import Image

    from u2pl_amd.infer import colormap

    d, s, cfgp, _, ckpt = trained
    out, raw = str(tmp_path / "results"), str(tmp_path / "results_raw")
    text = _run("eval.py", cfgp, "--model_path", ckpt, "--save_folder", out, "--crop", "--base_size", "160")
    ious = re.findall(r"\* class \[(\d+)\] IoU", text)
    assert [int(c) for c in ious] == list(range(C_CLI)) and "* mIoU" in text
    text_raw = _run("eval.py", cfgp, "--model_path", ckpt, "--save_folder", raw, "--crop", "--base_size", "160", "--raw_ids")
    assert re.findall(r"\* mIoU (\S+)", text_raw) == re.findall(r"\* mIoU (\S+)", text)      # mIoU stays in class space
    generic = colormap("generic")
    names = sorted(os.listdir(os.path.join(out, "gray")))
    assert len(names) == 4
    for name in names:
        gray = np.array(Image.open(os.path.join(out, "gray", name)))
        assert gray.dtype == np.uint8 and gray.max() < C_CLI
        assert np.array_equal(np.array(Image.open(os.path.join(raw, "gray", name))), gray + 1)
        for folder in (out, raw):                        # colours are looked up in class space either way
            assert np.array_equal(np.array(Image.open(os.path.join(folder, "color", name))), generic[gray])


def test_infer_cli_on_a_list_of_single_field_lines(trained, tmp_path):
    from PIL import Image

    from u2pl_amd.infer import colormap

    d, s, cfgp, _, ckpt = trained
    cfg = yaml.safe_load(open(cfgp))
    cfg["dataset"]["val"]["data_list"] = os.path.join(s, "unlabeled.txt")        # `image_path` alone on every line
    assert all(len(ln.split()) == 1 for ln in open(cfg["dataset"]["val"]["data_list"]))
    cfg2 = str(tmp_path / "config.yaml")
    yaml.safe_dump(cfg, open(cfg2, "w"))
    out = str(tmp_path / "viewer")
    _run("infer.py", cfg2, "--model_path", ckpt, "--save_folder", out)           # input scale: dataset.val.crop.size
    generic = colormap("generic")
    names = sorted(os.listdir(os.path.join(out, "gray")))
    assert len(names) == 4
    for name in names:
        gray = np.array(Image.open(os.path.join(out, "gray", name)))
        assert name.endswith(".png")                     # index maps are never written as JPEG
        size = Image.open(os.path.join(d, "images", name[:-4] + ".jpg")).size
        assert gray.shape == size[::-1] and gray.max() < C_CLI
        assert np.array_equal(np.array(Image.open(os.path.join(out, "color", name))), generic[gray])
