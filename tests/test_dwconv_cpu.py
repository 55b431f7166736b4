"""Depthwise 3x3 convolutions and the separable DeepLabv3+ decoder, the parts that need no GPU: K.Conv2d(C, C, 3, groups=C) draws
torch's parameters, dwconv_constraint names what csrc/dwconv.hip refuses, a numpy float32 emulation of the kernels holds the
float64 bound of tests/dw_bounds.py on every shape the GPU tests use while three faulty emulations break it (so bound and shape
list can tell a wrong kernel from a right one), and the decoders build with `separable` (keys as DESIGN 3.14 lists them) and are
unchanged without it."""
import pytest
import torch

import dw_bounds as B
from model_utils import net_cfg


def test_depthwise_conv2d_draws_torchs_parameters_and_exchanges_state_dicts():
    from u2pl_amd import nn as K
    for bias in (False, True):
        torch.manual_seed(7)
        ours = K.Conv2d(32, 32, 3, padding=2, dilation=2, groups=32, bias=bias)
        a = torch.rand(4)
        torch.manual_seed(7)
        ref = torch.nn.Conv2d(32, 32, 3, padding=2, dilation=2, groups=32, bias=bias)
        assert torch.equal(a, torch.rand(4))                  # the generator is where torch leaves it
        assert ours.weight.shape == ref.weight.shape == (32, 1, 3, 3)
        assert torch.equal(ours.weight, ref.weight)
        assert (ours.bias is None) == (not bias) and (not bias or torch.equal(ours.bias, ref.bias))
        torch.manual_seed(11)
        fresh = torch.nn.Conv2d(32, 32, 3, groups=32, bias=bias)
        fresh.load_state_dict(ours.state_dict())
        assert torch.equal(fresh.weight, ours.weight)
        back = K.Conv2d(32, 32, 3, groups=32, bias=bias)
        back.load_state_dict(fresh.state_dict())
        assert torch.equal(back.weight, ref.weight) and set(back.state_dict()) == set(ref.state_dict())
        assert "g=32" in ours.extra_repr()


def test_dwconv_constraint_names_what_the_kernels_refuse():
    from u2pl_amd import nn as K
    assert K.dwconv_constraint(32, 32, 32, 3, 3, 1) is None
    assert K.dwconv_constraint(2048, 2048, 2048, 3, 3, 2) is None
    assert "depth multiplier" in K.dwconv_constraint(32, 64, 32, 3, 3, 1)
    assert "multiple of 4" in K.dwconv_constraint(6, 6, 6, 3, 3, 1)
    assert "3x3" in K.dwconv_constraint(32, 32, 32, 5, 5, 1)
    assert "stride" in K.dwconv_constraint(32, 32, 32, 3, 3, 3)
    assert "groups" in K.dwconv_constraint(32, 32, 8, 3, 3, 1)
    assert K.gconv_constraint(32, 32, 32, 1) is not None      # the grouped route still refuses it: Conv2d decides depthwise first


@pytest.mark.parametrize("kw,text", [(dict(in_channels=8, out_channels=16, kernel_size=3, groups=8), "depth multiplier"),
                                     (dict(in_channels=8, out_channels=8, kernel_size=5, groups=8), "3x3"),
                                     (dict(in_channels=6, out_channels=6, kernel_size=3, groups=6), "multiple of 4")])
def test_unsupported_depthwise_layers_construct_and_are_refused_at_the_first_call(kw, text):
    from u2pl_amd import nn as K
    from u2pl_amd._lib import HipError
    conv = K.Conv2d(**kw)                                     # torch.nn.Conv2d constructs such layers too
    k = kw["kernel_size"]
    assert text in K.dwconv_constraint(conv.in_channels, conv.out_channels, conv.groups, k, k, conv.stride)
    with pytest.raises(HipError):                             # (a CPU tensor: no CPU fallback either; the text: test_gpu_dwconv)
        conv(torch.zeros(1, kw["in_channels"], 7, 7))


# ---- the bound and the shape list can tell a wrong kernel from a right one ----------------------------------------------------
@pytest.fixture(scope="module")
def emulated():
    """per shape: the float64 references with their bounds and the operands (computed once, not modified)"""
    out = []
    for N, C, H, W, stride, dil in B.shape_list():
        x, w, gy, pad = B.operands(C, H, W, stride, dil, N=N)
        out.append(((N, C, H, W, stride, dil), (x, w, gy, pad), B.refs(x, w, gy, stride, pad, dil)))
    return out


def test_shape_list_covers_the_edges_the_kernels_have():
    shapes = B.shape_list()
    cs = {s[1] for s in shapes}
    assert {4, 8} <= cs and all(c % 4 == 0 for c in cs)
    for edge in (128, 256):                                   # both sides of each channel-tile edge
        assert edge in cs and edge + 4 in cs and (edge == 256 or edge - 4 in cs)
    assert any(c > 128 and c % 8 for c in cs)
    assert {1, 2} == {s[4] for s in shapes} and {1, 2, 4, 12} == {s[5] for s in shapes}
    N, C, H, W, stride, dil = B.SLAB_CASE
    rows, slabs = B.wgrad_slabs(N * B.out_size(H, stride, dil, dil) * B.out_size(W, stride, dil, dil), C)
    assert slabs == B.SLAB_CASE_SLABS and rows % W                # two slab edges, neither at the end of an image row


def test_fp32_emulation_holds_the_bound_on_every_shape(emulated):
    for shape, (x, w, gy, pad), refs in emulated:
        got = B.emulate(x, w, gy, shape[4], pad, shape[5])
        worst = B.worst(got, refs)
        assert all(v <= 1.0 for v in worst.values()), (shape, worst)
        assert all(float(got[k].abs().max()) > 0 for k in got), shape


def test_centre_tap_only_geometry_has_exact_zeros(emulated):
    """(9, 9, 1, 12): every off-centre tap meets padding only -- cond and the bound are 0 there, dw must be exactly 0"""
    for shape, (x, w, gy, pad), refs in emulated:
        if shape[5] != 12:
            continue
        bound = refs["dw"][1]
        off_centre = torch.ones(3, 3, dtype=torch.bool)
        off_centre[1, 1] = False
        assert float(bound[:, 0][:, off_centre].max()) == 0 and float(bound[:, 0, 1, 1].min()) > 0
        broken = {k: v.clone() for k, v in B.emulate(x, w, gy, shape[4], pad, shape[5]).items()}
        broken["dw"][0, 0, 0, 0] = 1e-30                      # anything but 0 where only padding is met
        assert B.worst(broken, refs)["dw"] > 1.0


@pytest.mark.parametrize("fault,outputs", [("border", ("y", "dw")), ("dilation", ("y", "dx", "dw")), ("parity", ("dx",))])
def test_faulty_emulations_break_the_bound(emulated, fault, outputs):
    broken = {k: 0 for k in outputs}
    for shape, (x, w, gy, pad), refs in emulated:
        worst = B.worst(B.emulate(x, w, gy, shape[4], pad, shape[5], fault=fault), refs)
        for k in outputs:
            broken[k] += worst[k] > 1.0
    print(fault, broken)
    assert all(v > 0 for v in broken.values()), (fault, broken)


# ---- models ---------------------------------------------------------------------------------------------------------------------
def _bn(prefix, C):
    return {prefix + ".weight": (C,), prefix + ".bias": (C,), prefix + ".running_mean": (C,), prefix + ".running_var": (C,),
            prefix + ".num_batches_tracked": ()}


def _sep(prefix, i, C, out, bias):
    """the five parameter-carrying entries of a separable unit that starts at index i of a Sequential"""
    keys = {"%s.%d.weight" % (prefix, i): (C, 1, 3, 3), "%s.%d.weight" % (prefix, i + 3): (out, C, 1, 1)}
    if bias:
        keys["%s.%d.bias" % (prefix, i + 3)] = (out,)
    keys.update(_bn("%s.%d" % (prefix, i + 1), C))
    keys.update(_bn("%s.%d" % (prefix, i + 4), out))
    return keys


def separable_v3plus_keys(in_planes=2048, num_classes=19):
    keys = {"low_conv.0.weight": (256, 256, 1, 1), "low_conv.0.bias": (256,), **_bn("low_conv.1", 256),
            "aspp.conv1.1.weight": (256, in_planes, 1, 1), **_bn("aspp.conv1.2", 256),
            "aspp.conv2.0.weight": (256, in_planes, 1, 1), **_bn("aspp.conv2.1", 256)}
    for b in ("aspp.conv3", "aspp.conv4", "aspp.conv5"):
        keys.update(_sep(b, 0, in_planes, 256, False))
    keys.update(_sep("head", 0, 1280, 256, False))
    for tower, out in (("classifier", num_classes), ("representation", 256)):
        keys.update(_sep(tower, 0, 512, 256, True))
        keys.update(_sep(tower, 7, 256, 256, True))
        keys.update({tower + ".14.weight": (out, 256, 1, 1), tower + ".14.bias": (out,)})
    return keys


def test_separable_v3plus_decoder_builds_with_the_documented_keys():
    from u2pl_amd import nn as K
    from u2pl_amd.models.decoder import dec_deeplabv3_plus
    dec = dec_deeplabv3_plus(in_planes=2048, separable=True)
    got = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
    assert got == separable_v3plus_keys()
    dw = [m for m in dec.modules() if isinstance(m, K.Conv2d) and m.groups != 1]
    assert sorted(tuple(m.weight.shape) for m in dw) == sorted([(2048, 1, 3, 3)] * 3 + [(1280, 1, 3, 3)] + [(512, 1, 3, 3)] * 2
                                                              + [(256, 1, 3, 3)] * 2)
    assert all(m.groups == m.in_channels == m.out_channels and m.bias is None for m in dw)
    assert [m.dilation for m in dw[:3]] == [12, 24, 36] and [m.padding for m in dw[:3]] == [12, 24, 36]
    assert all(K.dwconv_constraint(m.in_channels, m.out_channels, m.groups, 3, 3, m.stride) is None for m in dw)
    # the Dropout2d entries are where the dense layers had them: after each unit of the head and the towers
    assert [i for i, m in enumerate(dec.classifier) if isinstance(m, torch.nn.Dropout2d)] == [6, 13]
    assert [i for i, m in enumerate(dec.head) if isinstance(m, torch.nn.Dropout2d)] == [6]


def test_separable_v3_decoder_and_aspp_build():
    from u2pl_amd.models.base import ASPP
    from u2pl_amd.models.decoder import dec_deeplabv3
    sd = dec_deeplabv3(in_planes=512, num_classes=21, separable=True).state_dict()
    assert tuple(sd["aspp.conv4.0.weight"].shape) == (512, 1, 3, 3) and tuple(sd["head.3.weight"].shape) == (256, 1280, 1, 1)
    assert tuple(sd["head.7.weight"].shape) == (21, 256, 1, 1) and "head.3.bias" not in sd
    assert ASPP(64, inner_planes=32, separable=True).get_outplanes() == ASPP(64, inner_planes=32).get_outplanes() == 160


@pytest.mark.parametrize("cls", ["dec_deeplabv3", "dec_deeplabv3_plus"])
def test_separable_false_is_the_decoder_built_without_the_keyword(cls):
    from u2pl_amd.models import decoder
    torch.manual_seed(3)
    a = getattr(decoder, cls)(in_planes=128)
    ra = torch.rand(4)
    torch.manual_seed(3)
    b = getattr(decoder, cls)(in_planes=128, separable=False)
    assert torch.equal(ra, torch.rand(4))                     # the same RNG draws
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]) for k in sa)
    assert [type(m) for m in a.modules()] == [type(m) for m in b.modules()]
    assert "classifier.8.weight" in sa or cls == "dec_deeplabv3"   # the reference's indices


def test_a_checkpoint_of_the_other_kind_is_refused_by_load_state_dict():
    from u2pl_amd.models.decoder import dec_deeplabv3_plus
    dense, sep = dec_deeplabv3_plus(in_planes=64), dec_deeplabv3_plus(in_planes=64, separable=True)
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key|size mismatch"):
        sep.load_state_dict(dense.state_dict())
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key|size mismatch"):
        dense.load_state_dict(sep.state_dict())


def test_model_builder_takes_decoder_separable():
    from u2pl_amd.models.model_helper import ModelBuilder
    cfg = net_cfg("resnet50", 19, True)
    cfg["decoder"]["kwargs"]["separable"] = True
    sd = ModelBuilder(cfg).state_dict()
    assert tuple(sd["decoder.aspp.conv3.0.weight"].shape) == (2048, 1, 3, 3)
    assert tuple(sd["decoder.classifier.14.weight"].shape) == (19, 256, 1, 1)
    assert tuple(sd["auxor.aux.0.weight"].shape) == (256, 1024, 3, 3)          # the auxiliary head stays dense


def test_separable_example_config_sets_the_option():
    import os
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tools", "city_semi_separable_example.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["net"]["decoder"]["kwargs"]["separable"] is True
    assert cfg["net"]["decoder"]["type"].endswith("dec_deeplabv3_plus")
