"""-m gpu: the prediction epilogue / prologue kernels (csrc/infer.hip), u2pl_amd.infer.infer_image against the reference
fixture tests/golden/infer_r50_97.npz (tools/gen_infer_golden.py), evaluate(palette=...) and the infer.py / eval.py
command lines."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from model_utils import formula_state_dict, net_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLASSES = [2, 19, 21]
SIZES = [((25, 25), (110, 150)), ((9, 13), (37, 50)), ((40, 40), (64, 64)), ((33, 33), (33, 33)), ((17, 25), (70, 101)),
         ((5, 7), (3, 5))]
BATCH = [1, 2]


def _palette(name):
    from u2pl_amd.infer import colormap
    return colormap(name)


@functools.lru_cache(maxsize=None)
def _case(C, lo, hi, N):
    """(random-normal logits, the copy with exact ties) as CPU tensors; seeded by the case."""
    g = torch.Generator().manual_seed(1000 * C + 100 * lo[0] + 10 * hi[1] + N)
    x = torch.randn(N, C, lo[0], lo[1], generator=g) * 3
    tied = x.clone()
    # planes 7 and C - 1 := plane 3 (C = 2 has neither a plane 3 nor a plane 7: there plane 1 := plane 0)
    src = 3 if C > 3 else 0
    for c in {7, C - 1}:
        if src < c < C:
            tied[:, c] = x[:, src]
    return x, tied


def _strided(x):
    """the same values as a view with sn, sc, sh, sw all different from a contiguous tensor's"""
    N, C, h, w = x.shape
    wide = torch.full((N, 2 * C + 1, h + 1, 2 * w + 2), float("nan"), device=x.device)
    view = wide[:, 1::2, 1:, 2::2]
    view.copy_(x)
    assert view.shape == x.shape and view.stride(1) != h * w and view.stride(3) == 2
    return view


@pytest.mark.parametrize("N", BATCH)
@pytest.mark.parametrize("lo,hi", SIZES)
@pytest.mark.parametrize("C", CLASSES)
def test_predict_map_equals_bilinear_up_then_lowest_index_argmax(C, lo, hi, N):
    from u2pl_amd import hipops as H
    pal_np = _palette("pascal" if C == 21 else "cityscapes")
    pal = torch.from_numpy(pal_np).to(DEV)
    for kind, x in zip(("normal", "ties"), _case(C, lo, hi, N)):
        xd = x.to(DEV)
        up = H.bilinear_up(xd, hi).cpu().numpy()
        want = up.argmax(1).astype(np.uint8)                     # numpy: lowest index among equals
        if kind == "ties":
            top = np.sort(up, axis=1)[:, -1]
            src = 3 if C > 3 else 0
            print("pixels whose maximum is a duplicated plane:", int((up[:, src] == top).sum()), "of", top.size)
        for tag, inp in (("contiguous", xd), ("strided", _strided(xd))):
            label, rgb = H.predict_map(inp, hi, pal)
            assert label.dtype == torch.uint8 and tuple(label.shape) == (N, *hi)
            assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (N, *hi, 3)
            label, rgb = label.cpu().numpy(), rgb.cpu().numpy()
            assert np.array_equal(label, want), (kind, tag, int((label != want).sum()))
            assert np.array_equal(rgb, pal_np[label]), (kind, tag)
            only, none = H.predict_map(inp, hi)
            assert none is None and np.array_equal(only.cpu().numpy(), want), (kind, tag)


@pytest.mark.parametrize("N", BATCH)
@pytest.mark.parametrize("lo,hi", SIZES)
@pytest.mark.parametrize("C", CLASSES)
def test_predict_map_against_torch_cpu(C, lo, hi, N):
    """torch's CPU bilinear differs from the three-FMA form in the last bit at some size pairs, so pixels whose
    reference top-two margin is below 2^-20 * max|reference logits| are left out (at most 0.1 % of a case); every other
    pixel must agree."""
    from u2pl_amd import hipops as H
    x = _case(C, lo, hi, N)[0]
    ref = F.interpolate(x, hi, mode="bilinear", align_corners=True)
    top2 = ref.topk(2, dim=1).values
    near = (top2[:, 0] - top2[:, 1]) < 2.0 ** -20 * ref.abs().max()
    label = H.predict_map(x.to(DEV), hi)[0].cpu()
    bad = (label.long() != ref.argmax(1)) & ~near
    share = near.double().mean().item()
    print(f"excluded {int(near.sum())} of {near.numel()} pixels, disagreements outside {int(bad.sum())}")
    assert share <= 1e-3
    assert not bad.any()


def test_predict_map_rejects_more_than_256_classes_and_cpu_tensors():
    from u2pl_amd import hipops as H
    from u2pl_amd._lib import HipError
    with pytest.raises(HipError):
        H.predict_map(torch.zeros(1, 257, 3, 3, device=DEV), (4, 4))
    with pytest.raises(HipError):
        H.predict_map(torch.zeros(1, 4, 3, 3), (4, 4))
    with pytest.raises(HipError):
        H.infer_input(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(3, 256), (4, 4))
    label, _ = H.predict_map(torch.zeros(1, 256, 3, 3, device=DEV), (4, 4))
    assert int(label.max()) == 0


def _lut():
    from u2pl_amd.infer import normalise_lut
    g = golden("infer_r50_97")
    return normalise_lut(g["mean"].tolist(), g["std"].tolist())


def _images():
    g = golden("infer_r50_97")
    rng = np.random.default_rng(5)
    return [(g["img_0"], (97, 97), g["input_0"]), (g["img_1"], (97, 97), g["input_1"]),
            (rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), (65, 65), None),
            (rng.integers(0, 256, (64, 48, 3), dtype=np.uint8), (64, 48), None)]


@pytest.mark.parametrize("k", range(4))
def test_infer_input_equals_table_then_bilinear_up(k):
    from u2pl_amd import hipops as H
    img, size, ref = _images()[k]
    lut = _lut()
    out = H.infer_input(torch.from_numpy(img).to(DEV), torch.from_numpy(lut).to(DEV), size)
    assert tuple(out.shape) == (1, 3, *size) and out.is_contiguous(memory_format=torch.channels_last)
    planar = np.stack([lut[c][img[:, :, c]] for c in range(3)])[None]                # (1,3,h,w) normalised
    want = H.bilinear_up(torch.from_numpy(planar).to(DEV), size).contiguous(memory_format=torch.channels_last)
    assert out.stride() == want.stride()
    assert torch.equal(out, want)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))    # the bits, signed zeros too
    if ref is not None:
        # the reference normalises with the same table values and interpolates the same fp32 operands with the same
        # three roundings per axis pair; only contraction can differ: <= 4 ulp of the tensor's maximum
        ulp = float(np.spacing(np.float32(np.abs(ref).max())))
        diff = float(np.abs(out.cpu().numpy().astype(np.float64) - ref.astype(np.float64)).max())
        print(f"max |hip - reference input| = {diff:.3e} = {diff / ulp:.2f} ulp of the maximum {np.abs(ref).max():.4f}")
        assert diff <= 4 * ulp


def _model():
    from u2pl_amd.models.model_helper import ModelBuilder
    m = ModelBuilder(net_cfg("resnet50", 19, True))
    m.load_state_dict(formula_state_dict(m))
    return m.to(DEV).eval()


@pytest.mark.parametrize("k", [0, 1])
def test_infer_image_matches_the_reference_fixture(k):
    """the error model of tests/test_gpu_eval.py for this network and these ill-conditioned weights"""
    from u2pl_amd import infer as I
    g = golden("infer_r50_97")
    pascal = _palette("pascal")
    img = g[f"img_{k}"]
    label, rgb, pred = I.infer_image(_model(), torch.from_numpy(img).to(DEV), torch.from_numpy(_lut()).to(DEV),
                                     tuple(int(v) for v in g["input_scale"]), torch.from_numpy(pascal).to(DEV))
    ref32, ref64 = torch.from_numpy(g[f"pred_{k}"]).double(), torch.from_numpy(g[f"pred64_{k}"]).double()
    assert tuple(pred.shape) == tuple(ref32.shape)
    e_ref = (ref32 - ref64).abs().max().item()
    err = (pred.cpu().double() - ref64).abs()
    scale = ref64.abs().max().item()
    share = (err > 32.0 * e_ref + 1e-6 * scale).double().mean().item()
    label, rgb = label.cpu().numpy(), rgb.cpu().numpy()
    agree = float((label == g[f"mask_{k}"]).mean())
    print(f"|hip-f64| {err.max().item():.3e}  |ref32-f64| {e_ref:.3e}  scale {scale:.3e}  share over {share:.4f}  "
          f"label agreement {agree:.4f}")
    assert share <= 0.01
    assert label.shape == img.shape[:2] and label.dtype == np.uint8
    assert agree > 0.97
    assert np.array_equal(rgb, pascal[label])
    assert float((rgb == g[f"color_{k}"]).all(-1).mean()) > 0.97      # the reference's colour image, where labels agree


def test_evaluate_with_palette_hands_out_gray_and_colour():
    from u2pl_amd import evaluate as E
    from u2pl_amd.models.model_helper import ModelBuilder
    torch.manual_seed(3)
    m = ModelBuilder(net_cfg("resnet50", 19, True)).to(DEV).eval()
    g = torch.Generator().manual_seed(4)
    samples = []
    for (h, w) in [(70, 100), (60, 66)]:
        img = torch.randn(3, h, w, generator=g)
        lab = torch.randint(0, 19, (h, w), generator=g).numpy().astype(np.uint8)
        lab[:3] = 255
        samples.append((img, lab))
    city = _palette("cityscapes")
    kw = dict(base_size=100, crop=(65, 65), scales=(1.0,), use_crop=True)
    plain, coloured = {}, {}
    miou0, iou0 = E.evaluate(m, samples, 19, on_prediction=lambda i, gray: plain.__setitem__(i, gray), **kw)
    miou1, iou1 = E.evaluate(m, samples, 19, on_prediction=lambda i, gray, color: coloured.__setitem__(i, (gray, color)),
                             palette=city, **kw)
    assert miou1 == miou0 and np.array_equal(iou0, iou1)
    assert sorted(plain) == sorted(coloured) == [0, 1]
    for i, (img, lab) in enumerate(samples):
        gray, color = coloured[i]
        assert gray.dtype == np.uint8 and gray.shape == lab.shape and color.dtype == np.uint8 and color.shape == (*lab.shape, 3)
        logits = E.predict_image(m, img.unsqueeze(0).to(DEV), 19, kw["base_size"], kw["crop"], kw["scales"], True)
        top2 = logits.topk(2, dim=0).values
        clear = ((top2[0] - top2[1]) != 0).cpu().numpy()
        assert np.array_equal(gray[clear], plain[i][clear])
        assert np.array_equal(color, city[gray])


def test_infer_and_eval_command_lines(tmp_path):
    import make_synth_dataset as M
    import yaml
    from PIL import Image
    from u2pl_amd import infer as I
    from u2pl_amd.models.model_helper import ModelBuilder

    d, s = M.make_cityscapes(str(tmp_path), H=110, W=150)
    cfgp = M.write_city_config(str(tmp_path), d, s, crop=97, epochs=1)
    cfg = yaml.load(open(cfgp), Loader=yaml.Loader)
    model = ModelBuilder(cfg["net"])
    sd = formula_state_dict(model)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"teacher_state": {"module." + k: v for k, v in sd.items()}}, ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(script, out, *extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--config", cfgp, "--model_path", ckpt,
                            "--save_folder", out, *extra], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout + r.stderr

    names = [ln.strip() for ln in open(cfg["dataset"]["val"]["data_list"]) if ln.strip()]
    assert len(names) == 4
    pascal, city = _palette("pascal"), _palette("cityscapes")
    lut = torch.from_numpy(I.normalise_lut(cfg["dataset"]["mean"], cfg["dataset"]["std"])).to(DEV)
    out = str(tmp_path / "viewer")
    run("infer.py", out, "--input_scale", "97", "97")
    for rel in names:
        name = os.path.basename(rel)
        img = np.array(Image.open(os.path.join(d, rel)).convert("RGB"))
        gray = Image.open(os.path.join(out, "gray", name))
        assert gray.mode == "L"
        gray, color = np.array(gray), np.array(Image.open(os.path.join(out, "color", name)))
        assert gray.dtype == np.uint8 and gray.shape == img.shape[:2] and gray.max() < 19
        assert np.array_equal(color, pascal[gray])
        label, _, _ = I.infer_image(model, torch.from_numpy(img).to(DEV), lut, (97, 97))
        assert np.array_equal(gray, label.cpu().numpy())
    # (--base_size: the images are 110 x 150; eval.py's default of 2048 would slide the 97 x 97 window over 1502 x 2048)
    out = str(tmp_path / "results")
    text = run("eval.py", out, "--crop", "--base_size", "150")
    assert "mIoU" in text
    for rel in names:
        name = os.path.basename(rel).split(".")[0] + ".png"
        gray, color = np.array(Image.open(os.path.join(out, "gray", name))), np.array(Image.open(os.path.join(out, "color", name)))
        assert gray.shape == (110, 150) and np.array_equal(color, city[gray])
