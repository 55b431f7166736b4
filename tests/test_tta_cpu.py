"""Host side of test-time flip / probability fusion (u2pl_amd/evaluate.py, u2pl_amd/infer.py, the two command lines) without
a GPU: the forward and the kernels are replaced by the torch restatement of tests/tta_ref.py, and the control flow --
windows, padding, views, weights, which view bumps the count, scales -- is held to a hand composition."""
import importlib.util
import os
import types

import pytest
import torch
import torch.nn.functional as F

import tta_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 5


class _Net(torch.nn.Module):
    """a stride-4 convolution with weights that have no left-right symmetry: the mirrored view differs from the plain one"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        self.w = torch.randn(C, 3, 5, 5, generator=g)
        self.calls = 0

    def low(self, x):
        return F.conv2d(x, self.w.to(x.dtype), stride=4, padding=2)

    def forward(self, x, need_aux=False, need_rep=False):
        self.calls += 1
        return {"pred": self.low(x)}


@pytest.fixture
def E(monkeypatch):
    """u2pl_amd.evaluate with its kernels restated on CPU tensors; E.log lists the fused launches"""
    from u2pl_amd import evaluate as E
    log = []

    def window_fuse(pred, count, logits, origin, size, flip=False, softmax=False, weight=1.0, bump=True):
        log.append((tuple(origin), tuple(size), bool(flip), bool(softmax), float(weight), bool(bump), count is not None))
        T.window_fuse_ref(pred[0] if pred.dim() == 4 else pred, count, logits[0] if logits.dim() == 4 else logits, origin, size,
                          flip, softmax, weight, bump)

    def call(name, *a):
        if name == "u2pl_window_accumulate_f32":
            pred, count, _, _, _, src, h0, w0, hc, wc = a
            pred[0, :, h0:h0 + hc, w0:w0 + wc] += src[0]
            count[h0:h0 + hc, w0:w0 + wc] += 1
        elif name == "u2pl_window_normalize_f32":
            a[0].div_(a[1])
        else:
            raise AssertionError(name)

    fake = types.SimpleNamespace(window_fuse=window_fuse,
                                 bilinear_up=lambda x, size: F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True))
    monkeypatch.setattr(E, "H", fake)
    monkeypatch.setattr(E, "call", call)
    E.log = log
    return E


def _image(h, w, seed=0):
    return torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(seed))


# float32 sums of a handful of O(1) terms, associated differently by the launches (pred += w*a; pred += w*b) and by the hand
# composition (pred += w*a + w*b): a few ulp of the largest partial sum
TOL = dict(rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("flip,prob", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("hw,windows", [((17, 24), 2), ((12, 14), 1), ((30, 17), 3)])
def test_scale_crop_process_is_the_hand_composition(E, hw, windows, flip, prob):
    """17 x 24: two windows that overlap; 12 x 14: an image smaller than the 17 x 17 crop, padded; 30 x 17: three in a column"""
    net, x = _Net(), _image(*hw)
    out = E.scale_crop_process(net, x, C, 17, 17, 21, 29, flip=flip, prob=prob)
    ref = T.scale_crop_ref(net.low, x, C, 17, 17, 21, 29, flip, prob)
    assert out.shape == (C, 21, 29)
    torch.testing.assert_close(out, ref, **TOL)
    views = 2 if flip else 1
    assert net.calls == views * windows and len(E.log) == views * windows
    for k, (origin, size, fl, sm, weight, bump, has_count) in enumerate(E.log):
        assert size == (17, 17) and sm == prob and weight == 1.0 / views and has_count
        assert fl == (k % views == 1) and bump == (k % views == 0)         # the plain view bumps the count, the mirrored one not
    if prob:                                                              # a mean of probabilities stays one
        torch.testing.assert_close(out.sum(0), torch.ones(21, 29), **TOL)


def test_options_off_take_todays_calls(E, monkeypatch):
    """a guard for the untouched path: with the options off (by default and spelt out) the accumulate / normalise calls of
    before and no fused launch; with one on, fused launches and no accumulate call"""
    net, x = _Net(), _image(17, 24)
    seen = []
    real = E.call
    monkeypatch.setattr(E, "call", lambda name, *a: seen.append(name) or real(name, *a))
    out = E.scale_crop_process(net, x, C, 17, 17, 17, 24)
    assert seen == ["u2pl_window_accumulate_f32"] * 2 + ["u2pl_window_normalize_f32"] and E.log == []
    torch.testing.assert_close(out, T.scale_crop_ref(net.low, x, C, 17, 17, 17, 24, False, False), **TOL)
    del seen[:]
    assert torch.equal(E.scale_crop_process(net, x, C, 17, 17, 17, 24, flip=False, prob=False), out)
    assert seen == ["u2pl_window_accumulate_f32"] * 2 + ["u2pl_window_normalize_f32"] and E.log == []
    del seen[:]
    E.scale_crop_process(net, x, C, 17, 17, 17, 24, prob=True)
    assert seen == ["u2pl_window_normalize_f32"] and len(E.log) == 2
    del E.log[:]
    whole = E.scale_whole_process(net, x, 20, 30)
    assert E.log == []
    up = lambda t, size: F.interpolate(t, size, mode="bilinear", align_corners=True)       # noqa: E731
    torch.testing.assert_close(whole, up(up(net.low(x), (17, 24)), (20, 30))[0], **TOL)


@pytest.mark.parametrize("use_crop", [True, False])
def test_predict_image_sums_two_scales_of_fused_windows(E, use_crop):
    net, x = _Net(), _image(20, 28, seed=1)
    out = E.predict_image(net, x, C, 28, (17, 17), scales=(1.0, 0.75), use_crop=use_crop, flip=True, prob=True)
    ref = T.predict_image_ref(net.low, x, C, 28, (17, 17), (1.0, 0.75), use_crop, True, True)
    torch.testing.assert_close(out, ref, **TOL)
    torch.testing.assert_close(out.sum(0), torch.full((20, 28), 2.0), **TOL)      # scales are summed, not averaged
    if not use_crop:                                                              # one window = the scaled image, no count
        assert [(e[0], e[1], e[6]) for e in E.log] == [((0, 0), (20, 28), False)] * 2 + [((0, 0), (15, 21), False)] * 2


def test_net_process_with_half_redoes_a_saturated_view_per_view(E):
    net, x = _Net(), _image(17, 17)

    class Half:
        calls = 0

        def __call__(self, image):
            self.calls += 1
            return net.low(image) + 100.0, self.calls == 2          # the mirrored view saturates; its fp16 result is dropped

    half = Half()
    out = E.net_process(net, x, half, flip=True, prob=False)
    a = F.interpolate(net.low(x) + 100.0, (17, 17), mode="bilinear", align_corners=True)
    b = F.interpolate(net.low(x.flip(3)), (17, 17), mode="bilinear", align_corners=True).flip(3)
    assert half.calls == 2 and net.calls == 1
    torch.testing.assert_close(out, 0.5 * a + 0.5 * b, **TOL)


def test_infer_image_fuses_at_the_image_size(monkeypatch):
    from u2pl_amd import infer as I
    net = _Net()
    x = _image(17, 21, seed=2)
    launches = []

    def window_fuse(pred, count, logits, origin, size, flip, softmax, weight, bump):
        launches.append((tuple(pred.shape), count, tuple(origin), tuple(size), flip, softmax, weight, bump))
        T.window_fuse_ref(pred, count, logits[0], origin, size, flip, softmax, weight, bump)

    monkeypatch.setattr(I.H, "infer_input", lambda img, lut, size: x)
    monkeypatch.setattr(I.H, "window_fuse", window_fuse)
    monkeypatch.setattr(I.H, "predict_map", lambda pred, size, palette: (pred.argmax(1).to(torch.uint8), None))
    img = torch.zeros(30, 40, 3, dtype=torch.uint8)
    label, rgb, pred = I.infer_image(net, img, None, (17, 21), flip=True, prob=True)
    assert launches == [((C, 30, 40), None, (0, 0), (30, 40), False, True, 0.5, False),
                        ((C, 30, 40), None, (0, 0), (30, 40), True, True, 0.5, False)]
    up = lambda t: F.softmax(F.interpolate(t, (30, 40), mode="bilinear", align_corners=True), 1)       # noqa: E731
    ref = 0.5 * up(net.low(x)) + 0.5 * up(net.low(x.flip(3))).flip(3)
    assert pred.shape == (1, C, 30, 40) and label.shape == (30, 40) and rgb is None
    torch.testing.assert_close(pred, ref, **TOL)
    # options off: the low-resolution logits go to predict_map as they are, and nothing is fused
    del launches[:]
    label, rgb, pred = I.infer_image(net, img, None, (17, 21))
    assert launches == [] and pred.shape == (1, C, 5, 6) and label.shape == (5, 6)     # (this fake predict_map does not resize)
    assert torch.equal(pred, net.low(x))


def _script(name):
    spec = importlib.util.spec_from_file_location(name[:-3] + "_tta_cli", os.path.join(ROOT, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("script", ["infer.py", "eval.py"])
def test_fusion_options_parse_and_default_to_off(script, capsys):
    mod = _script(script)
    p = mod.get_cli_parser(fusion=True)
    a = p.parse_args([])
    assert a.flip is False and a.prob is False and a.half is False
    a = p.parse_args(["--flip", "--prob"])
    assert a.flip is True and a.prob is True
    assert p.parse_args(["--prob"]).flip is False
    ref_opts = {s for act in mod.get_parser()._actions for s in act.option_strings}
    assert {s for act in p._actions for s in act.option_strings} == ref_opts | {"--half", "--flip", "--prob"}
    for opt in ("--flip", "--prob"):                       # the reference's surface has neither
        with pytest.raises(SystemExit):
            mod.get_parser().parse_args([opt])
    capsys.readouterr()


def test_the_entry_point_is_declared_and_exported():
    import ctypes
    from u2pl_amd import _lib
    decls = _lib.parse_header()
    ret, argtypes, names = decls["u2pl_window_fuse_f32"]
    assert names == ["pred", "count", "C", "H", "W", "in", "sc", "sh", "sw", "h", "w", "h0", "w0", "hc", "wc", "flip", "softmax",
                     "weight", "bump", "stream"]
    assert argtypes[17] is ctypes.c_float and argtypes[6] is ctypes.c_long
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "u2pl_window_fuse_f32")


def test_window_fuse_has_no_cpu_fallback():
    from u2pl_amd import hipops as H
    from u2pl_amd._lib import HipError
    with pytest.raises(HipError):
        H.window_fuse(torch.zeros(2, 4, 4), torch.zeros(4, 4), torch.zeros(2, 2, 2), (0, 0), (4, 4))
