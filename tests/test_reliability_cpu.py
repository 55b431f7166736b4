"""Host side of the reliability maps (--entropy / --drop_percent: u2pl_amd/infer.py, u2pl_amd/evaluate.py, hipops.predict_reliable,
the two command lines) without a GPU: the kernels are replaced by the restatements of tests/reliability_ref.py and the call
sequence is held to a hand composition; the restatements themselves are held to the reference expression in float64."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import reliability_ref as R
import tta_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 5


# ------------------------------------------------------------------ command lines, declarations
def _script(name):
    spec = importlib.util.spec_from_file_location(name[:-3] + "_rel_cli", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _opts(p):
    return {s for act in p._actions for s in act.option_strings}


@pytest.mark.parametrize("script", ["infer.py", "eval.py"])
def test_reliability_options_are_added_by_their_keyword_only(script, capsys):
    mod = _script(script)
    ref = _opts(mod.get_parser())
    assert _opts(mod.get_cli_parser()) == ref | {"--half"}
    assert _opts(mod.get_cli_parser(fusion=True)) == ref | {"--half", "--flip", "--prob"}
    p = mod.get_cli_parser(fusion=True, reliability=True)
    assert _opts(p) == ref | {"--half", "--flip", "--prob", "--drop_percent", "--entropy"}
    a = p.parse_args([])
    assert a.drop_percent is None and a.entropy is False and a.flip is False and a.prob is False and a.half is False
    a = p.parse_args(["--drop_percent", "80", "--entropy"])
    assert a.drop_percent == 80.0 and isinstance(a.drop_percent, float) and a.entropy is True
    for opt in (["--entropy"], ["--drop_percent", "80"]):
        for q in (mod.get_parser(), mod.get_cli_parser(), mod.get_cli_parser(fusion=True)):
            with pytest.raises(SystemExit):
                q.parse_args(opt)
    capsys.readouterr()


def test_the_entry_points_are_declared_and_exported():
    import ctypes
    from u2pl_amd import _lib
    decls = _lib.parse_header()
    ret, argtypes, names = decls["u2pl_predict_entropy_f32"]
    assert names == ["in", "sn", "sc", "sh", "sw", "N", "C", "h", "w", "H", "W", "prob", "label", "entropy", "stream"]
    assert argtypes[1] is ctypes.c_long and argtypes[11] is ctypes.c_int and ret is ctypes.c_int
    ret, argtypes, names = decls["u2pl_reliable_map_u8"]
    assert names == ["label", "entropy", "thr_bits", "n", "palette", "rgb", "heat", "heat_scale", "ndropped", "stream"]
    assert argtypes[3] is ctypes.c_long and argtypes[7] is ctypes.c_float
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(so, "u2pl_predict_entropy_f32") and hasattr(so, "u2pl_reliable_map_u8")


def test_new_ops_have_no_cpu_fallback_and_check_their_arguments():
    from u2pl_amd import hipops as H
    from u2pl_amd._lib import HipError
    with pytest.raises(HipError):
        H.predict_entropy(torch.zeros(1, 4, 3, 3), (4, 4))
    with pytest.raises(HipError):
        H.reliable_map(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4))
    for bad in (-0.5, 100.5, float("nan")):
        with pytest.raises(ValueError):
            H.check_drop_percent(bad)
        with pytest.raises(ValueError):
            H.predict_reliable(torch.zeros(1, 4, 3, 3), (4, 4), drop_percent=bad)
    for good in (None, 0, 100, 99.5):
        H.check_drop_percent(good)


# ------------------------------------------------------------------ the restatements against the reference expression
@pytest.mark.parametrize("scale", [0.1, 3.0, 80.0])
@pytest.mark.parametrize("classes", [2, 5, 19, 21])
def test_logits_restatements_agree_with_the_reference_expression(classes, scale):
    """log(s) - t / s is -sum(p log p); the reference's + 1e-10 inside the log moves the value by at most C * 1e-10.  In
    float32, term for term, the restatement stays inside the project's entropy tolerance of 2e-6."""
    z = (np.random.default_rng(classes).standard_normal((2, classes, 13, 16)) * scale).astype(np.float32)
    ref = R.entropy_ref64(z)
    e64, e32 = R.entropy_logits_f64(z), R.entropy_logits_f32(z)
    assert e32.dtype == np.float32 and e64.dtype == np.float64
    d64, d32 = np.abs(e64 - ref).max(), np.abs(e32.astype(np.float64) - ref).max()
    print(f"C {classes} scale {scale}: |f64 - ref| {d64:.3e}  |f32 - ref| {d32:.3e}")
    assert d64 <= classes * 1e-10 + 1e-12
    assert d32 <= 2e-6
    assert (ref >= -1e-9).all() and (ref <= np.log(classes) + 1e-9).all()


@pytest.mark.parametrize("classes", [2, 5, 19, 21])
def test_prob_restatements_agree_with_the_reference_expression(classes):
    """one view's softmax as class weights, times any positive factor: the entropy of the logits; an all-zero pixel: log C"""
    z = np.random.default_rng(10 + classes).standard_normal((classes, 9, 11)) * 3
    e = np.exp(z - z.max(0))
    p = e / e.sum(0)
    ref = R.entropy_ref64(z)
    for factor in (1.0, 3.0):
        a = (factor * p).astype(np.float32)
        a[:, 0, 0] = 0
        want = ref.copy()
        want[0, 0] = np.log(classes)
        e64, e32 = R.entropy_prob_f64(a), R.entropy_prob_f32(a)
        d32 = np.abs(e32.astype(np.float64) - e64).max()
        print(f"C {classes} factor {factor}: |f64 - ref| {np.abs(e64 - want).max():.3e}  |f32 - f64| {d32:.3e}")
        assert np.abs(e64 - want).max() <= 5e-7              # the weights were rounded to float32
        assert d32 <= 2e-6 and not np.isnan(e32).any()
    a = np.zeros((classes, 2, 2), np.float32)
    a[0] = 1                                                  # a one-hot pixel: zero terms contribute nothing
    assert np.array_equal(R.entropy_prob_f32(a), np.zeros((2, 2), np.float32))


def test_heat_bytes_span_the_byte_range():
    for classes in (2, 19, 21):
        ent = np.array([0.0, np.log(classes) / 4, np.log(classes), 10.0, -1.0], np.float32)
        assert R.heat_bytes(ent, classes).tolist() == [0, 64, 255, 255, 0]


# ------------------------------------------------------------------ host logic on stand-in kernels
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.randn(C, 3, 5, 5, generator=torch.Generator().manual_seed(7))
        self.p = torch.nn.Parameter(torch.zeros(1))

    def low(self, x):
        return F.conv2d(x, self.w, stride=4, padding=2)

    def forward(self, x, need_aux=False, need_rep=False):
        return {"pred": self.low(x)}


@pytest.fixture
def K(monkeypatch):
    """u2pl_amd.hipops with its prediction-side kernels restated on CPU tensors (hipops.predict_reliable itself is the real
    one), u2pl_amd.evaluate.call likewise; K.log lists every launch by name"""
    from u2pl_amd import evaluate as E
    from u2pl_amd import hipops as H
    log = []

    def logged(name, fn):
        def wrapper(*a, **kw):
            log.append(name)
            return fn(*a, **kw)
        return wrapper

    def window_fuse(pred, count, logits, origin, size, flip=False, softmax=False, weight=1.0, bump=True):
        T.window_fuse_ref(pred[0] if pred.dim() == 4 else pred, count, logits[0] if logits.dim() == 4 else logits, origin, size,
                          flip, softmax, weight, bump)

    def predict_map(x, size, palette=None):
        label = F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True).argmax(1).to(torch.uint8)
        return label, None if palette is None else palette[label.long()]

    def call(name, *a):
        log.append(name)
        if name == "u2pl_window_accumulate_f32":
            pred, count, _, _, _, src, h0, w0, hc, wc = a
            pred[0, :, h0:h0 + hc, w0:w0 + wc] += src[0]
            count[h0:h0 + hc, w0:w0 + wc] += 1
        elif name == "u2pl_window_normalize_f32":
            a[0].div_(a[1])
        elif name == "u2pl_confusion_hist_f32":
            logits, target, ignore, _, classes, _, _, hist = a
            R.confusion_hist_t(logits, target, ignore, classes, hist)
        else:
            raise AssertionError(name)

    fakes = dict(window_fuse=window_fuse, predict_map=predict_map, predict_entropy=R.predict_entropy_t,
                 entropy_threshold=R.entropy_threshold_t, reliable_map=R.reliable_map_t, drop_high_entropy_=R.drop_high_entropy_t,
                 bilinear_up=lambda x, size: F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True),
                 infer_input=lambda img, lut, size: torch.randn(1, 3, *size, generator=torch.Generator().manual_seed(2)))
    for name, fn in fakes.items():
        monkeypatch.setattr(H, name, logged(name, fn))
    monkeypatch.setattr(E, "call", call)
    H.log = log
    yield H
    del H.log


PAL = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (256, 3), dtype=np.uint8))


def test_infer_image_options_off_make_todays_calls(K):
    from u2pl_amd import infer as I
    net, img = _Net(), torch.zeros(30, 40, 3, dtype=torch.uint8)
    out = I.infer_image(net, img, None, (17, 21), PAL)
    assert K.log == ["infer_input", "predict_map"] and len(out) == 3
    del K.log[:]
    again = I.infer_image(net, img, None, (17, 21), PAL, drop_percent=None, entropy=False)
    assert K.log == ["infer_input", "predict_map"] and len(again) == 3
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    del K.log[:]
    I.infer_image(net, img, None, (17, 21), PAL, flip=True, prob=True)
    assert K.log == ["infer_input", "window_fuse", "window_fuse", "predict_map"]
    for bad in (-1, 100.001):
        del K.log[:]
        with pytest.raises(ValueError):
            I.infer_image(net, img, None, (17, 21), PAL, drop_percent=bad)
        assert K.log == []                                   # refused before anything is launched


@pytest.mark.parametrize("flip,prob", [(False, False), (True, True), (True, False)])
def test_infer_image_options_on_make_the_hand_composition(K, flip, prob):
    from u2pl_amd import infer as I
    net, img = _Net(), torch.zeros(30, 40, 3, dtype=torch.uint8)
    fuse = ["window_fuse"] * (2 if flip else 1) if (flip or prob) else []
    label0, rgb0, pred0 = I.infer_image(net, img, None, (17, 21), PAL, flip=flip, prob=prob)
    # entropy alone: the same label and colours, one entropy launch and one epilogue launch, no threshold
    del K.log[:]
    label, rgb, pred, rel = I.infer_image(net, img, None, (17, 21), PAL, flip=flip, prob=prob, entropy=True)
    assert K.log == ["infer_input"] + fuse + ["predict_entropy", "reliable_map"]
    assert torch.equal(label, label0) and torch.equal(rgb, rgb0) and torch.equal(pred, pred0)
    assert rel["threshold"] is None and rel["ndropped"] is None
    assert rel["entropy"].shape == (30, 40) and rel["entropy"].dtype == torch.float32
    up = F.interpolate(pred0, size=(30, 40), mode="bilinear", align_corners=True).numpy()
    ent = (R.entropy_prob_f32 if prob else R.entropy_logits_f32)(up)[0]
    assert np.array_equal(rel["entropy"].numpy(), ent)
    assert np.array_equal(rel["heat"].numpy(), R.heat_bytes(ent, C))
    # drop_percent: threshold per image, then the epilogue; heat only with entropy=True; half= puts the dict last
    for want_heat in (False, True):
        del K.log[:]
        out = I.infer_image(net, img, None, (17, 21), PAL, flip=flip, prob=prob, drop_percent=80, entropy=want_heat,
                            half=lambda x: (net.low(x), 0))
        assert K.log == ["infer_input"] + fuse + ["predict_entropy", "entropy_threshold", "reliable_map"]
        label, rgb, pred, fell_back, rel = out
        assert fell_back is False
        thr = np.percentile(ent.ravel(), 80).astype(np.float32)
        want, want_rgb, heat, nd = R.reliable_map_np(label0.numpy(), ent, thr, PAL.numpy(), C if want_heat else None)
        assert rel["threshold"].numpy().view(np.uint32)[0] == thr.view(np.uint32)
        assert np.array_equal(label.numpy(), want) and np.array_equal(rgb.numpy(), want_rgb)
        assert int(rel["ndropped"]) == nd == int((want == 255).sum()) and 0.19 * 1200 <= nd <= 0.21 * 1200
        assert (rel["heat"] is None) == (not want_heat)
        if want_heat:
            assert np.array_equal(rel["heat"].numpy(), heat)


def _samples():
    g = torch.Generator().manual_seed(4)
    out = []
    for (h, w) in [(20, 28), (17, 28)]:          # the long side is base_size: no rescaling
        lab = torch.randint(0, C, (h, w), generator=g).numpy().astype(np.uint8)
        lab[:2] = 255
        out.append((torch.randn(3, h, w, generator=g), lab))
    return out


KW = dict(base_size=28, crop=(17, 17), scales=(1.0,), use_crop=False)
PER_IMAGE = ["bilinear_up", "bilinear_up", "u2pl_confusion_hist_f32"]       # net_process, scale_whole_process, histogram


def test_evaluate_options_off_make_todays_calls(K):
    from u2pl_amd import evaluate as E
    net, samples = _Net(), _samples()
    seen = []
    m0, iou0 = E.evaluate(net, samples, C, palette=PAL, on_prediction=lambda *a: seen.append(len(a)), **KW)
    assert K.log == (PER_IMAGE + ["predict_map"]) * 2 and seen == [3, 3]
    del K.log[:], seen[:]
    m1, iou1 = E.evaluate(net, samples, C, palette=PAL, on_prediction=lambda *a: seen.append(len(a)), drop_percent=None,
                          entropy=False, **KW)
    assert K.log == (PER_IMAGE + ["predict_map"]) * 2 and seen == [3, 3] and m1 == m0 and np.array_equal(iou0, iou1)
    del K.log[:]
    assert E.evaluate(net, samples, C, **KW)[0] == m0 and K.log == PER_IMAGE * 2
    del K.log[:]
    assert E.evaluate(net, samples, C, entropy=True, **KW)[0] == m0 and K.log == PER_IMAGE * 2      # nobody to hand it to
    with pytest.raises(ValueError):
        E.evaluate(net, samples, C, drop_percent=101, **KW)


@pytest.mark.parametrize("prob", [False, True])
def test_evaluate_options_on_make_the_hand_composition(K, prob):
    from u2pl_amd import evaluate as E
    net, samples = _Net(), _samples()
    m0, iou0 = E.evaluate(net, samples, C, prob=prob, **KW)
    # net_process (one fused window with prob, else a bilinear_up), scale_whole_process, the histogram
    per_image = ["window_fuse" if prob else "bilinear_up", "bilinear_up", "u2pl_confusion_hist_f32"]
    # entropy alone: filtered maps are today's maps, heat is handed out last, the return value keeps its two elements
    got = {}
    del K.log[:]
    res = E.evaluate(net, samples, C, prob=prob, palette=PAL, on_prediction=lambda i, *a: got.__setitem__(i, a), entropy=True, **KW)
    assert len(res) == 2 and res[0] == m0
    assert K.log == (per_image + ["predict_entropy", "reliable_map"]) * 2
    ents = []
    for i, (img, lab) in enumerate(samples):
        scores = E.predict_image(net, img.unsqueeze(0), C, KW["base_size"], KW["crop"], KW["scales"], False, prob=prob)
        ent = (R.entropy_prob_f32 if prob else R.entropy_logits_f32)(scores.numpy())
        ents.append((scores, ent))
        gray, color, heat = got[i]
        assert np.array_equal(gray, scores.argmax(0).numpy().astype(np.uint8)) and np.array_equal(color, PAL.numpy()[gray])
        assert np.array_equal(heat, R.heat_bytes(ent, C))
    # drop_percent: three return values, the first two unchanged; rel from the filtered maps and the ground truth
    for palette, want_heat in ((PAL, True), (None, False)):
        got.clear()
        del K.log[:]
        m, iou, rel = E.evaluate(net, samples, C, prob=prob, palette=palette, on_prediction=lambda i, *a: got.__setitem__(i, a),
                                 drop_percent=80, entropy=want_heat, **KW)
        assert K.log == (per_image + ["predict_entropy", "entropy_threshold", "reliable_map", "drop_high_entropy_",
                                      "u2pl_confusion_hist_f32"]) * 2
        assert m == m0 and np.array_equal(iou, iou0)
        total, reliable, live = np.zeros((3, C), np.int64), np.zeros((3, C), np.int64), 0
        for i, (img, lab) in enumerate(samples):
            scores, ent = ents[i]
            assert len(got[i]) == (3 if palette is not None else 2)
            gray, heat = got[i][0], got[i][-1]
            thr = np.percentile(ent.ravel(), 80).astype(np.float32)
            want = R.reliable_map_np(scores.argmax(0).numpy().astype(np.uint8), ent, thr, None, None)[0]
            assert np.array_equal(gray, want)
            if palette is not None:
                assert np.array_equal(got[i][1], PAL.numpy()[gray])
            assert (heat is None) == (not want_heat)
            reliable += R.hists_from_maps(gray, lab, C)
            total += R.hists_from_maps(scores.argmax(0).numpy(), lab, C)
            live += int((lab != 255).sum())
        assert np.array_equal(rel["hist_reliable"], reliable)
        assert np.array_equal(rel["hist_reliable"] + rel["hist_unreliable"], total)
        assert rel["coverage"] == reliable[1].sum() / live
        want_iou = reliable[0] / (reliable[1] + reliable[2] - reliable[0] + 1e-10)
        assert np.array_equal(rel["iou_reliable"], want_iou) and rel["miou_reliable"] == float(np.mean(want_iou))
        unrel = total - reliable
        assert np.array_equal(rel["iou_unreliable"], unrel[0] / (unrel[1] + unrel[2] - unrel[0] + 1e-10))
    # without anybody to hand the maps to, the threshold and the second histogram are still needed
    del K.log[:]
    rel2 = E.evaluate(net, samples, C, prob=prob, drop_percent=80, **KW)[2]
    assert K.log == (per_image + ["predict_entropy", "entropy_threshold", "reliable_map", "drop_high_entropy_",
                                  "u2pl_confusion_hist_f32"]) * 2
    assert np.array_equal(rel2["hist_reliable"], reliable)
