"""-m gpu: the reliability maps of the prediction side -- u2pl_predict_entropy_f32 and u2pl_reliable_map_u8 (csrc/infer.hip)
against the kernels they restate and the float64 / numpy references of tests/reliability_ref.py, then infer_image,
evaluate and the two command lines with drop_percent / entropy.

Shapes: the smallest at which these kernels can go wrong -- W % 4 != 0 (byte stores), aligned quads, identity size (what the
fused accumulators use), one source pixel, down-sampling, and 4 (h - 1) = H - 1, where u2pl_entropy_up_f32 (the kernel the
entropy is held to, bit for bit) takes its cell kernels for 19 and 21 classes."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import reliability_ref as R
from conftest import golden
from model_utils import formula_state_dict, net_cfg
from test_gpu_infer import _case, _lut, _model, _palette, _strided

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLASSES = [2, 19, 21, 5]
SIZES = [((5, 7), (17, 23)), ((9, 13), (37, 52)), ((13, 16), (13, 16)), ((1, 1), (4, 5)), ((5, 7), (3, 5)), ((5, 7), (17, 25))]
BATCH = [1, 2]
TOL = 2e-6          # the project's entropy tolerance (tests/test_gpu_loss_path.py, header of csrc/reliability.hip)


def _views(x):
    xd = x.to(DEV)
    return (("contiguous", xd), ("strided", _strided(xd)))


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _logf(C):
    """the device's logf((float)C) from a kernel that was there before: the entropy of C equal logits is logf(s) - t / s with
    s = C and t = 0 exactly (u2pl_entropy_up_f32)"""
    from u2pl_amd import hipops as H
    v = H.entropy_map_up(torch.zeros(1, C, 1, 1, device=DEV), (1, 1), None, H.new_select_ws(DEV, 1)).cpu().numpy()[0, 0, 0]
    assert abs(float(v) - np.log(float(C))) <= TOL
    return v


def _is_logf(v, C):
    return isinstance(v, np.float32) and v.view(np.uint32) == _logf(C).view(np.uint32)


# ------------------------------------------------------------------ 1. labels
@pytest.mark.parametrize("lo,hi", SIZES)
@pytest.mark.parametrize("C", CLASSES)
def test_labels_are_predict_maps(C, lo, hi):
    from u2pl_amd import hipops as H
    for N in BATCH:
        for kind, x in zip(("normal", "ties"), _case(C, lo, hi, N)):
            for tag, inp in _views(x):
                want = H.predict_map(inp, hi)[0]
                for prob in (False, True):       # the arg-max does not depend on what the scores mean
                    label, ent = H.predict_entropy(inp, hi, prob)
                    assert label.dtype == torch.uint8 and tuple(label.shape) == (N, *hi)
                    assert ent.dtype == torch.float32 and tuple(ent.shape) == (N, *hi)
                    assert torch.equal(label, want), (N, kind, tag, prob, int((label != want).sum()))
        flat = torch.full((N, C, *lo), 0.37, device=DEV)
        label, ent = H.predict_entropy(flat, hi)
        err = float((ent.double() - np.log(C)).abs().max())
        print(f"all-equal logits: max |entropy - log C| = {err:.3e}")
        assert int(label.max()) == 0 and err <= TOL


# ------------------------------------------------------------------ 2. entropy of logits
@pytest.mark.parametrize("lo,hi", SIZES)
@pytest.mark.parametrize("C", CLASSES)
def test_entropy_of_logits_has_entropy_ups_bits_and_the_float64_bound(C, lo, hi):
    from u2pl_amd import hipops as H
    worst = 0.0
    for N in BATCH:
        for scale in (0.1, 3.0, 80.0):
            x = _case(C, lo, hi, N)[0] * (scale / 3.0)
            ref = R.entropy_ref64(H.bilinear_up(x.to(DEV), hi).cpu().numpy())       # the interpolated bits, then float64
            for tag, inp in _views(x):
                ws = H.new_select_ws(DEV, N * hi[0] * hi[1])
                want = H.entropy_map_up(inp, hi, None, ws)
                ent = H.predict_entropy(inp, hi)[1]
                assert torch.equal(_bits(ent), _bits(want)), (N, scale, tag, int((_bits(ent) != _bits(want)).sum()))
                err = float(np.abs(ent.cpu().numpy().astype(np.float64) - ref).max())
                worst = max(worst, err)
                assert err <= TOL, (N, scale, tag, err)
    print(f"C {C} {lo}->{hi}: max |entropy - float64 reference| = {worst:.3e}")


# ------------------------------------------------------------------ 3. entropy of class weights
@functools.lru_cache(maxsize=None)
def _weights(C, lo, N, S):
    """means of two float64 softmaxes times S, rounded to fp32, entries below 1e-30 zeroed; plane 1 all zeros (C > 2: the
    pixel sums stay positive); the pixel (0, 0, 0) all zeros"""
    rng = np.random.default_rng(100 * C + 10 * lo[1] + N)

    def softmax(scale):
        z = rng.standard_normal((N, C, *lo)) * scale
        e = np.exp(z - z.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)

    a = (S * 0.5 * (softmax(3.0) + softmax(40.0))).astype(np.float32)
    a[a < 1e-30] = 0
    if C > 2:
        a[:, 1] = 0
    a[0, :, 0, 0] = 0
    return torch.from_numpy(a)


@pytest.mark.parametrize("lo,hi", SIZES)
@pytest.mark.parametrize("C", CLASSES)
def test_entropy_of_class_weights_against_float64(C, lo, hi):
    from u2pl_amd import hipops as H
    worst = worst32 = 0.0
    for N in BATCH:
        for S in (1.0, 3.0):
            a = _weights(C, lo, N, S)
            up = H.bilinear_up(a.to(DEV), hi).cpu().numpy()
            ref, ref32 = R.entropy_prob_f64(up), R.entropy_prob_f32(up)
            worst32 = max(worst32, float(np.abs(ref32.astype(np.float64) - ref).max()))
            for tag, inp in _views(a):
                ent = H.predict_entropy(inp, hi, prob=True)[1].cpu().numpy()
                assert not np.isnan(ent).any(), (N, S, tag)
                assert _is_logf(ent[0, 0, 0], C), (N, S, tag, ent[0, 0, 0])                  # the pixel that knows nothing
                err = float(np.abs(ent.astype(np.float64) - ref).max())
                worst = max(worst, err)
                assert err <= TOL, (N, S, tag, err)
    print(f"C {C} {lo}->{hi}: max |entropy - float64| = {worst:.3e} (float32 numpy restatement: {worst32:.3e})")


def test_class_weights_that_are_all_zero_or_negative_give_no_nan():
    from u2pl_amd import hipops as H
    a = torch.zeros(1, 5, 6, 7, device=DEV)
    ent = H.predict_entropy(a, (6, 7), prob=True)[1].cpu().numpy()
    assert all(_is_logf(v, 5) for v in ent.ravel())
    a[:, 2] = -1.0
    a[:, 3, :3] = 2.0            # rows 0-2: S = 1 with one negative weight, which contributes nothing; rows 3-5: S = -1
    ent = H.predict_entropy(a, (6, 7), prob=True)[1].cpu().numpy()
    assert not np.isnan(ent).any() and all(_is_logf(v, 5) for v in ent[0, 3:].ravel())
    assert np.abs(ent[0, :3].astype(np.float64) + 2 * np.log(2.0)).max() <= 4 * np.spacing(np.float32(1.0))


# ------------------------------------------------------------------ 4. the epilogue, exactly
@functools.lru_cache(maxsize=None)
def _maps(C, lo, hi, N):
    from u2pl_amd import hipops as H
    label, ent = H.predict_entropy(_case(C, lo, hi, N)[0].to(DEV), hi)
    return label, ent


@pytest.mark.parametrize("P", [0, 20, 80, 99.5, 100])
@pytest.mark.parametrize("C,lo,hi,N", [(19, (9, 13), (37, 52), 1), (21, (5, 7), (17, 23), 2), (5, (1, 1), (4, 5), 1)])
def test_epilogue_is_exact(C, lo, hi, N, P):
    from u2pl_amd import hipops as H
    label0, ent = _maps(C, lo, hi, N)
    l_np, e_np = label0.cpu().numpy(), ent.cpu().numpy()
    thr = H.entropy_threshold(ent, P)
    want_thr = np.asarray(np.percentile(e_np.ravel(), P)).astype(np.float32)
    assert thr.dtype == torch.float32 and thr.numel() == 1
    assert thr.cpu().numpy().view(np.uint32)[0] == want_thr.view(np.uint32), (float(thr), float(want_thr))
    runs = []
    for name in ("pascal", "cityscapes"):
        pal_np = _palette(name)
        for _ in range(2):
            label = label0.clone()
            rgb, heat, nd = H.reliable_map(label, ent, thr, torch.from_numpy(pal_np).to(DEV), C)
            want, want_rgb, want_heat, count = R.reliable_map_np(l_np, e_np, want_thr, pal_np, C)
            assert np.array_equal(label.cpu().numpy(), want)
            assert np.array_equal(rgb.cpu().numpy(), want_rgb) and tuple(rgb.shape) == (N, *hi, 3)
            assert np.array_equal(heat.cpu().numpy(), want_heat)
            assert nd.dtype == torch.int32 and int(nd) == count
            runs.append((name, label, rgb, heat, nd))
        assert all(torch.equal(a, b) for a, b in zip(runs[-1][1:], runs[-2][1:]))           # two runs, the same bytes
    print(f"P {P}: threshold {float(thr):.6f}, dropped {int(runs[0][4])} of {l_np.size}")
    # no threshold: nothing is dropped, nothing is counted; every output is optional
    label = label0.clone()
    rgb, heat, nd = H.reliable_map(label, ent, None, torch.from_numpy(_palette("pascal")).to(DEV), C)
    assert nd is None and torch.equal(label, label0) and np.array_equal(rgb.cpu().numpy(), _palette("pascal")[l_np])
    assert np.array_equal(heat.cpu().numpy(), R.heat_bytes(e_np, C))
    label = label0.clone()
    assert H.reliable_map(label, ent, thr)[:2] == (None, None) and np.array_equal(label.cpu().numpy(), want)


def test_epilogue_on_addresses_that_allow_no_wide_access():
    """pixel runs that start 1 byte / 4 bytes into an allocation and end inside a quad: every byte path"""
    from u2pl_amd import hipops as H
    label0, ent0 = _maps(19, (9, 13), (37, 52), 1)
    n = 37 * 52 - 2
    lbuf = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
    ebuf = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
    label, ent = lbuf[1:1 + n], ebuf[1:1 + n]
    label.copy_(label0.reshape(-1)[:n])
    ent.copy_(ent0.reshape(-1)[:n])
    assert label.data_ptr() % 4 == 1 and ent.data_ptr() % 16 == 4
    l_np, e_np, pal_np = label.cpu().numpy(), ent.cpu().numpy(), _palette("cityscapes")
    thr = H.entropy_threshold(ent, 50)
    want_thr = np.asarray(np.percentile(e_np, 50)).astype(np.float32)
    assert thr.cpu().numpy().view(np.uint32)[0] == want_thr.view(np.uint32)
    rgb, heat, nd = H.reliable_map(label, ent, thr, torch.from_numpy(pal_np).to(DEV), 19)
    want, want_rgb, want_heat, count = R.reliable_map_np(l_np, e_np, want_thr, pal_np, 19)
    assert np.array_equal(label.cpu().numpy(), want) and np.array_equal(rgb.cpu().numpy(), want_rgb)
    assert np.array_equal(heat.cpu().numpy(), want_heat) and int(nd) == count
    assert int(lbuf[0]) == 0 and int(lbuf[1 + n:].max()) == 0                               # nothing outside the run


# ------------------------------------------------------------------ 5. rejections
def test_rejections():
    from u2pl_amd import hipops as H
    from u2pl_amd import infer as I
    from u2pl_amd._lib import HipError
    with pytest.raises(HipError):
        H.predict_entropy(torch.zeros(1, 4, 3, 3), (4, 4))
    with pytest.raises(HipError):
        H.reliable_map(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4))
    with pytest.raises(HipError):
        H.predict_entropy(torch.zeros(1, 257, 3, 3, device=DEV), (4, 4))
    with pytest.raises(HipError):
        H.predict_entropy(torch.zeros(1, 4, 3, 3, device=DEV), (0, 4))
    label, ent = H.predict_entropy(torch.zeros(1, 256, 3, 3, device=DEV), (4, 4))            # 256 classes: labels still fit
    assert int(label.max()) == 0 and abs(float(ent.max()) - np.log(256)) <= TOL
    thr = H.entropy_threshold(ent, 50)
    with pytest.raises(HipError):
        H.reliable_map(label, ent, thr, heat_classes=256)                                    # 255 is the ignore value
    with pytest.raises(HipError):
        H.predict_reliable(torch.zeros(1, 256, 3, 3, device=DEV), (4, 4), drop_percent=50)
    assert H.predict_reliable(torch.zeros(1, 256, 3, 3, device=DEV), (4, 4), heat=True)[2]["heat"] is not None
    with pytest.raises(HipError):
        H.reliable_map(label, ent, heat_classes=1)
    with pytest.raises(HipError):
        H.reliable_map(label.long(), ent)
    for bad in (-1, 100.5):
        with pytest.raises(ValueError):
            H.predict_reliable(torch.zeros(1, 4, 3, 3, device=DEV), (4, 4), drop_percent=bad)
        with pytest.raises(ValueError):
            I.infer_image(None, torch.zeros(4, 4, 3, dtype=torch.uint8, device=DEV), None, (4, 4), drop_percent=bad)


# ------------------------------------------------------------------ 6. infer_image
@functools.lru_cache(maxsize=None)
def _net():
    return _model()


@pytest.mark.parametrize("mode", ["plain", "flip_prob", "half"])
def test_infer_image_with_entropy_and_drop_percent(mode):
    from u2pl_amd import hipops as H
    from u2pl_amd import infer as I
    g = golden("infer_r50_97")
    model = _net()
    img = torch.from_numpy(g["img_0"]).to(DEV)
    lut, pal = torch.from_numpy(_lut()).to(DEV), torch.from_numpy(_palette("pascal")).to(DEV)
    scale = tuple(int(v) for v in g["input_scale"])
    kw, prob = {}, False
    if mode == "flip_prob":
        kw, prob = dict(flip=True, prob=True), True
    elif mode == "half":
        from u2pl_amd.half import HalfPredictor
        kw = dict(half=HalfPredictor(model))
    h, w = img.shape[:2]
    base = I.infer_image(model, img, lut, scale, pal, **kw)
    out = I.infer_image(model, img, lut, scale, pal, entropy=True, **kw)
    assert len(out) == len(base) + 1
    assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1])
    rel = out[-1]
    assert rel["threshold"] is None and rel["ndropped"] is None
    assert tuple(rel["entropy"].shape) == (h, w) and rel["entropy"].dtype == torch.float32
    assert np.array_equal(rel["heat"].cpu().numpy(), R.heat_bytes(rel["entropy"].cpu().numpy(), 19))
    out = I.infer_image(model, img, lut, scale, pal, drop_percent=80, entropy=True, **kw)
    label, rgb, pred, rel = out[0], out[1], out[2], out[-1]
    if mode == "half":
        assert out[3] == base[3]
    # the composition of the pieces tested above, on the returned scores
    label2, ent2 = H.predict_entropy(pred, (h, w), prob)
    assert torch.equal(label2[0], base[0]) and torch.equal(_bits(ent2[0]), _bits(rel["entropy"]))
    thr = H.entropy_threshold(ent2, 80)
    assert torch.equal(_bits(thr), _bits(rel["threshold"]))
    rgb2, heat2, nd2 = H.reliable_map(label2, ent2, thr, pal, 19)
    assert torch.equal(label, label2[0]) and torch.equal(rgb, rgb2[0]) and torch.equal(rel["heat"], heat2[0])
    e_np = rel["entropy"].cpu().numpy()
    want_thr = np.asarray(np.percentile(e_np.ravel(), 80)).astype(np.float32)
    assert rel["threshold"].cpu().numpy().view(np.uint32)[0] == want_thr.view(np.uint32)
    nd, ties = int(rel["ndropped"]), int((e_np == want_thr).sum())
    assert nd == int(nd2) == int((label == 255).sum()) == int((e_np >= want_thr).sum())
    print(f"{mode}: threshold {float(want_thr):.6f}, {nd} of {h * w} pixels are 255 ({100.0 * nd / (h * w):.2f} %), "
          f"{ties} at the threshold; entropy range {e_np.min():.4f} .. {e_np.max():.4f}")
    assert 0.19 * h * w <= nd and nd - ties <= 0.21 * h * w
    assert not np.isnan(e_np).any() and e_np.min() >= -TOL and e_np.max() <= np.log(19) + TOL


# ------------------------------------------------------------------ 7. evaluate
def test_evaluate_reports_reliable_and_unreliable_pixels():
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
    plain, filtered = {}, {}
    miou0, iou0 = E.evaluate(m, samples, 19, on_prediction=lambda i, gray, color: plain.__setitem__(i, (gray, color)),
                             palette=city, **kw)
    miou1, iou1, rel = E.evaluate(m, samples, 19, on_prediction=lambda i, *maps: filtered.__setitem__(i, maps), palette=city,
                                  drop_percent=80, entropy=True, **kw)
    assert miou1 == miou0 and np.array_equal(iou0, iou1)
    total, reliable, live = np.zeros((3, 19), np.int64), np.zeros((3, 19), np.int64), 0
    for i, (img, lab) in enumerate(samples):
        gray, color, heat = filtered[i]
        kept = gray != 255
        assert gray.dtype == np.uint8 and gray.shape == lab.shape and heat.dtype == np.uint8 and heat.shape == lab.shape
        assert np.array_equal(gray[kept], plain[i][0][kept]) and np.array_equal(color, city[gray])
        share = 1.0 - kept.mean()
        print(f"image {i}: {100 * share:.2f} % of the pixels are 255")
        assert 0.19 <= share <= 0.22
        reliable += R.hists_from_maps(gray, lab, 19)
        total += R.hists_from_maps(plain[i][0], lab, 19)
        live += int((lab != 255).sum())
    assert np.array_equal(rel["hist_reliable"], reliable)
    assert np.array_equal(rel["hist_reliable"] + rel["hist_unreliable"], total)
    assert rel["coverage"] == reliable[1].sum() / live
    want = reliable[0] / (reliable[1] + reliable[2] - reliable[0] + 1e-10)
    assert np.array_equal(rel["iou_reliable"], want) and rel["miou_reliable"] == float(np.mean(want))
    unrel = total - reliable
    assert np.array_equal(rel["iou_unreliable"], unrel[0] / (unrel[1] + unrel[2] - unrel[0] + 1e-10))
    assert iou0.tolist() == (total[0] / (total[1] + total[2] - total[0] + 1e-10)).tolist()


# ------------------------------------------------------------------ 8. command lines
def test_command_lines_with_drop_percent_and_entropy(tmp_path):
    import make_synth_dataset as M
    import yaml
    from PIL import Image

    d, s = M.make_cityscapes(str(tmp_path), H=110, W=150)
    cfgp = M.write_city_config(str(tmp_path), d, s, crop=97, epochs=1)
    cfg = yaml.load(open(cfgp), Loader=yaml.Loader)
    from u2pl_amd.models.model_helper import ModelBuilder
    sd = formula_state_dict(ModelBuilder(cfg["net"]))
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"teacher_state": {"module." + k: v for k, v in sd.items()}}, ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(script, out, *extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--config", cfgp, "--model_path", ckpt,
                            "--save_folder", out, *extra], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout + r.stderr

    rels = [ln.strip() for ln in open(cfg["dataset"]["val"]["data_list"]) if ln.strip()]
    assert len(rels) == 4
    # the same model in this process: what the files must hold, and how many pixels tie with the threshold (these weights
    # saturate the softmax over most of some images: entropy exactly 0 there, and entropy >= thr keeps no tied pixel)
    from u2pl_amd import evaluate as E
    from u2pl_amd import hipops as H
    from u2pl_amd import infer as I
    model = ModelBuilder(cfg["net"])
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    ds = cfg["dataset"]
    lut = torch.from_numpy(I.normalise_lut(ds["mean"], ds["std"])).to(DEV)
    mean, std = np.asarray(ds["mean"], np.float32), np.asarray(ds["std"], np.float32)

    def expect(script, img):
        """-> (filtered labels, heat, entropy, threshold) as numpy, by the calls the script makes"""
        if script == "infer.py":
            label, _, _, rel = I.infer_image(model, torch.from_numpy(img).to(DEV), lut, (97, 97), drop_percent=80, entropy=True)
        else:
            x = torch.from_numpy((img.astype(np.float32) - mean) / std).permute(2, 0, 1).contiguous().unsqueeze(0).to(DEV)
            scores = E.predict_image(model, x, cfg["net"]["num_classes"], 150, ds["val"]["crop"]["size"], [1.0], True, None, True,
                                     True)
            label, _, rel = H.predict_reliable(scores.unsqueeze(0), img.shape[:2], True, None, 80, True)
            label = label[0]
        return label.cpu().numpy(), rel["heat"].cpu().numpy(), rel["entropy"].cpu().numpy(), rel["threshold"].cpu().numpy()[0]

    pascal, city = _palette("pascal"), _palette("cityscapes")
    jobs = [("infer.py", ("--input_scale", "97", "97"), ("--drop_percent", "80", "--entropy"), pascal, lambda n: n),
            ("eval.py", ("--crop", "--base_size", "150", "--flip", "--prob"), ("--drop_percent", "80", "--entropy"), city,
             lambda n: n.split(".")[0] + ".png")]
    for script, common, new, pal, out_name in jobs:
        before, after = str(tmp_path / (script + ".before")), str(tmp_path / (script + ".after"))
        text0 = run(script, before, *common)
        text1 = run(script, after, *common, *new)
        assert sorted(os.listdir(before)) == ["color", "gray"] and sorted(os.listdir(after)) == ["color", "entropy", "gray"]
        assert "dropped" not in text0 and "reliable" not in text0 and "coverage" not in text0
        if script == "infer.py":
            assert " * dropped pixels (drop_percent 80): mean share" in text1
        else:
            assert " * mIoU reliable (80) " in text1 and " * mIoU unreliable " in text1 and " * coverage " in text1
            assert [ln for ln in text0.splitlines() if "IoU" in ln] == [ln for ln in text1.splitlines() if "IoU" in ln and
                                                                        "reliable" not in ln]
        for rel_path in rels:
            name = out_name(os.path.basename(rel_path))
            gray0, color0 = (np.array(Image.open(os.path.join(before, k, name))) for k in ("gray", "color"))
            gray1, color1 = (np.array(Image.open(os.path.join(after, k, name))) for k in ("gray", "color"))
            heat = Image.open(os.path.join(after, "entropy", name.split(".")[0] + ".png"))
            assert heat.mode == "L" and heat.size == (150, 110)
            assert gray0.max() < 19 and np.array_equal(color0, pal[gray0])                   # as before
            dropped = gray1 == 255
            assert dropped.any()
            assert np.array_equal(gray1[~dropped], gray0[~dropped]) and np.array_equal(color1, pal[gray1])
            want, want_heat, ent, thr = expect(script, np.array(Image.open(os.path.join(d, rel_path)).convert("RGB")))
            assert np.array_equal(gray1, want) and np.array_equal(np.array(heat), want_heat)
            assert np.array_equal(dropped, ent >= thr)
            nd, ties, n = int(dropped.sum()), int((ent == thr).sum()), dropped.size
            print(f"{script} {name}: {nd} of {n} pixels are 255 ({100.0 * nd / n:.2f} %), {ties} at the threshold {thr:.6g}, "
                  f"heat {np.array(heat).min()} .. {np.array(heat).max()}")
            assert 0.19 * n <= nd and nd - ties <= 0.21 * n        # 20 % unless the entropy has ties at the threshold
