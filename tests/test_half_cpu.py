"""CPU checks of the fp16 prediction path: the float64 bound of tests/half_bounds.py accepts a faithful emulation of the
layer and rejects four faulty ones; HalfPredictor's scale / shift folding; what it refuses at construction; the public
surface (infer_image, the two command lines, the header)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import half_bounds as HB
from model_utils import formula_state_dict, net_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (N, H, W, Cin, Cout, k, stride, dil, res, relu)
LAYERS = {
    "1x1_res_relu": (1, 9, 11, 64, 21, 1, 1, 1, True, True),
    "3x3_res":      (2, 9, 9, 32, 19, 3, 1, 1, True, False),
    "3x3_s2_d2":    (1, 17, 17, 32, 24, 3, 2, 2, True, True),
}


def _layer(name):
    N, H, W, Cin, Cout, k, stride, dil, has_res, relu = LAYERS[name]
    rng = np.random.default_rng(len(name) + Cin)
    pad = dil * (k - 1) // 2
    x, w = HB.draw(rng, (N, Cin, H, W)), HB.draw(rng, (Cout, Cin, k, k), lo=-10, hi=0)
    scale = (rng.uniform(0.5, 1.5, Cout) * rng.choice([-1, 1], Cout)).astype(np.float32)
    shift = rng.uniform(-2, 2, Cout).astype(np.float32)
    ref0, _ = HB.layer_ref(x, w, scale, shift, None, False, stride, pad, dil)
    # a residual that nearly cancels the branch (the case a second rounding before the add cannot survive)
    res = (-ref0 * rng.uniform(0.9, 1.1, ref0.shape)).astype(np.float16).astype(np.float64) if has_res else None
    kw = dict(scale=scale, shift=shift, res=res, relu=relu, stride=stride, pad=pad, dil=dil)
    return x, w, kw


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_faithful_emulation_passes_the_bound(name, out_f32):
    x, w, kw = _layer(name)
    ref, bound = HB.layer_ref(x, w, out_f32=out_f32, **kw)
    ex = HB.excess(HB.emulate(x, w, out_f32=out_f32, **kw), ref, bound)
    print(f"{name} out_f32={out_f32}: max err / bound = {ex:.4f}")
    assert ex <= 1.0


@pytest.mark.parametrize("fault", ["round_before_res", "scale_after_round", "drop_tap", "fp16_acc"])
def test_faulty_emulations_fail_the_bound(fault):
    worst = {}
    for name in sorted(LAYERS):
        x, w, kw = _layer(name)
        ref, bound = HB.layer_ref(x, w, **kw)
        worst[name] = HB.excess(HB.emulate(x, w, fault=fault, **kw), ref, bound)
    print(fault, {k: round(v, 2) for k, v in worst.items()})
    assert all(v > 1.0 for v in worst.values()), worst


def test_draw_gives_fp16_normal_values_or_zero():
    v = HB.draw(np.random.default_rng(0), (4096,))
    assert np.array_equal(v, v.astype(np.float16).astype(np.float64))
    nz = np.abs(v[v != 0])
    assert (v == 0).any() and nz.min() >= 2.0 ** -10 * (1 - 2.0 ** -11) and nz.max() <= 16.0


def _model(cfg=None):
    from u2pl_amd.models.model_helper import ModelBuilder
    m = ModelBuilder(cfg or net_cfg("resnet50", 19, True))
    m.load_state_dict(formula_state_dict(m))
    return m.eval()


def test_scale_shift_folding_is_the_float64_batchnorm_rounded_once():
    from u2pl_amd import nn as K
    from u2pl_amd.half import HalfPredictor
    m = _model()
    p = HalfPredictor(m)                      # CPU tensors: the plan's vectors exist, the fp16 planes need the GPU
    assert len(p.units) == 53 + 5 + 1 + 1 + 3 + 2      # R50 convolutions (with the deep stem's 3 and 4 downsamples), ASPP, head, low, classifier
    with_bn = with_bias = 0
    for u in p.units:
        conv, bn = u.conv, u.bn
        assert u.w16 is None
        C = conv.out_channels
        v = torch.linspace(-3, 3, C, dtype=torch.float64)              # a conv output per channel (without its bias)
        z = v if conv.bias is None else v + conv.bias.detach().double()
        if bn is None:
            assert u.scale is None
            want = z
            got = v + (0 if u.shift is None else u.shift.double())
        else:
            assert isinstance(bn, K.BatchNorm2d)
            with_bn += 1
            want = (z - bn.running_mean.double()) / torch.sqrt(bn.running_var.double() + bn.eps) * bn.weight.detach().double() \
                + bn.bias.detach().double()
            s64 = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
            b64 = bn.bias.detach().double() - bn.running_mean.double() * s64
            if conv.bias is not None:
                with_bias += 1
                b64 = b64 + conv.bias.detach().double() * s64
            assert u.scale.dtype == torch.float32 and torch.equal(u.scale, s64.float()) and torch.equal(u.shift, b64.float())
            got = v * u.scale.double() + u.shift.double()
        # one fp32 rounding of each vector: 2^-24 relative on scale and on shift
        tol = 2.0 ** -24 * (v.abs() * (1 if u.scale is None else u.scale.double().abs()) + (0 if u.shift is None else u.shift.double().abs())) + 1e-300
        assert ((got - want).abs() <= 1.0001 * tol).all(), u.name
    assert with_bn == len(p.units) - 1 and with_bias == 3       # low_conv and the classifier's two 3x3 carry a bias under BN


def test_construction_refuses_grouped_layers_and_unknown_classes():
    import torch.nn as nn
    from u2pl_amd.half import HalfPredictor
    from u2pl_amd.models.model_helper import ModelBuilder
    cfg = net_cfg("resnet50", 19, True)
    cfg["encoder"]["kwargs"].update(groups=32, width_per_group=4)
    with pytest.raises(ValueError, match=r"encoder\.layer1\.0\.conv2.*groups=32"):
        HalfPredictor(ModelBuilder(cfg))

    m = _model()

    class other_decoder(nn.Module):
        pass

    m.decoder = other_decoder()
    with pytest.raises(TypeError, match="decoder class other_decoder"):
        HalfPredictor(m)
    m = _model()

    class plug_in(type(m.encoder)):
        pass

    m.encoder.__class__ = plug_in
    with pytest.raises(TypeError, match="encoder class plug_in"):
        HalfPredictor(m)


def test_predictor_has_no_cpu_fallback():
    from u2pl_amd._lib import HipError
    from u2pl_amd.half import HalfPredictor
    with pytest.raises(HipError):
        HalfPredictor(_model())(torch.zeros(1, 3, 33, 33))


def test_both_decoders_and_basic_blocks_build_a_plan():
    from u2pl_amd.half import HalfPredictor
    cfg = net_cfg("resnet50", 21, True)
    cfg["encoder"]["kwargs"]["fpn"] = False
    cfg["decoder"] = dict(type="u2pl.models.decoder.dec_deeplabv3", kwargs=dict(inner_planes=256, dilations=[12, 24, 36]))
    p = HalfPredictor(_model(cfg))
    assert not p.plus and [u.conv.out_channels for u in p.head] == [256, 21]
    cfg = net_cfg("resnet18", 19, False)
    cfg["encoder"]["kwargs"].update(multi_grid=False, replace_stride_with_dilation=[False, False, False])   # BasicBlock: no dilation
    cfg["encoder"]["kwargs"]["fpn"] = False
    cfg["decoder"] = dict(type="u2pl.models.decoder.dec_deeplabv3", kwargs=dict(inner_planes=256, dilations=[12, 24, 36]))
    p = HalfPredictor(_model(cfg))
    assert all(us[2] is None for layer in p.blocks for us in layer)


def test_infer_image_without_half_keeps_its_three_elements(monkeypatch):
    from u2pl_amd import infer as I

    class fake_model:
        def __call__(self, x, need_aux, need_rep):
            return {"pred": "pred"}

    class fake_half:
        def __init__(self, saturated):
            self.saturated = saturated

        def __call__(self, x):
            return "pred16", self.saturated

    monkeypatch.setattr(I.H, "infer_input", lambda img, lut, size: "x")
    monkeypatch.setattr(I.H, "predict_map", lambda pred, size, palette: (["label of " + pred], None))
    img = torch.zeros(4, 5, 3, dtype=torch.uint8)
    assert I.infer_image(fake_model(), img, None, (4, 5)) == ("label of pred", None, "pred")
    assert I.infer_image(fake_model(), img, None, (4, 5), half=fake_half(0)) == ("label of pred16", None, "pred16", False)
    assert I.infer_image(fake_model(), img, None, (4, 5), half=fake_half(3)) == ("label of pred", None, "pred", True)


@pytest.mark.parametrize("script", ["infer.py", "eval.py"])
def test_half_option_parses_and_defaults_to_off(script):
    spec = importlib.util.spec_from_file_location(script[:-3] + "_cli", os.path.join(ROOT, script))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.get_cli_parser()
    assert p.parse_args([]).half is False
    assert p.parse_args(["--half"]).half is True
    ref_opts = {s for act in mod.get_parser()._actions for s in act.option_strings}
    assert {s for act in p._actions for s in act.option_strings} == ref_opts | {"--half"}


def test_new_exports_are_declared_and_exported():
    import ctypes
    from u2pl_amd import _lib
    decls = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("u2pl_half_weight_f16", "u2pl_hconv2d_fwd_f16", "u2pl_hconv2d_stem_f16", "u2pl_hmaxpool3s2_f16",
                 "u2pl_hgap_f16", "u2pl_hbilinear_f16"):
        assert name in decls and decls[name][2][-1] == "stream", name
        assert hasattr(cdll, name), name
    assert len(decls["u2pl_hconv2d_fwd_f16"][1]) == 26
