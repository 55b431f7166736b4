"""Grouped convolutions (ResNeXt encoders), the parts that need no GPU: K.Conv2d(groups=g) draws the parameters torch.nn.Conv2d
draws and exchanges state_dicts with it, the encoder builds with the reference's `groups` / `width_per_group` keywords (also
through ModelBuilder), BasicBlock keeps upstream's ValueError, and the shape constraints of csrc/gconv.hip are reported at the
first call rather than at construction (torch.nn.Conv2d constructs such layers too)."""
import pytest
import torch

from model_utils import net_cfg


def test_grouped_conv2d_draws_torchs_parameters_and_exchanges_state_dicts():
    from u2pl_amd import nn as K
    torch.manual_seed(7)
    ours = K.Conv2d(16, 32, 3, groups=4, bias=True)
    torch.manual_seed(7)
    ref = torch.nn.Conv2d(16, 32, 3, groups=4, bias=True)
    assert ours.weight.shape == ref.weight.shape == (32, 4, 3, 3)
    assert torch.equal(ours.weight, ref.weight) and torch.equal(ours.bias, ref.bias)
    assert ours.weight.is_contiguous(memory_format=torch.channels_last)
    assert "g=4" in ours.extra_repr() and "g=" not in K.Conv2d(16, 32, 3).extra_repr()
    torch.manual_seed(11)
    fresh = torch.nn.Conv2d(16, 32, 3, groups=4, bias=True)
    fresh.load_state_dict(ours.state_dict())
    assert torch.equal(fresh.weight, ours.weight) and torch.equal(fresh.bias, ours.bias)
    back = K.Conv2d(16, 32, 3, groups=4, bias=True)
    back.load_state_dict(fresh.state_dict())
    assert torch.equal(back.weight, ref.weight) and torch.equal(back.bias, ref.bias)


def test_grouped_and_dense_conv2d_leave_the_generator_where_torch_leaves_it():
    from u2pl_amd import nn as K
    for kw in (dict(groups=4), dict()):
        torch.manual_seed(3)
        K.Conv2d(16, 32, 3, bias=True, **kw)
        a = torch.rand(4)
        torch.manual_seed(3)
        torch.nn.Conv2d(16, 32, 3, bias=True, **kw)
        assert torch.equal(a, torch.rand(4))


def test_resnext50_32x4d_constructs_with_the_reference_widths():
    from u2pl_amd.models import resnet
    m = resnet.resnet50(pretrained=False, groups=32, width_per_group=4)
    seen = 0
    for li, planes in ((1, 64), (2, 128), (3, 256), (4, 512)):
        width = int(planes * 4 / 64) * 32
        for blk in getattr(m, "layer%d" % li):
            assert blk.conv2.groups == 32
            assert tuple(blk.conv2.weight.shape) == (width, width // 32, 3, 3)
            assert blk.conv1.groups == 1 and blk.conv3.groups == 1
            seen += 1
    assert seen == 3 + 4 + 6 + 3
    keys = set(m.state_dict())
    assert "layer3.5.conv2.weight" in keys


def test_basic_block_still_refuses_groups():
    from u2pl_amd.models import resnet
    with pytest.raises(ValueError):
        resnet.resnet18(pretrained=False, groups=32)


def test_model_builder_takes_encoder_groups():
    from u2pl_amd.models.model_helper import ModelBuilder
    cfg = net_cfg("resnet50", 19, True)
    cfg["encoder"]["kwargs"].update(groups=32, width_per_group=4)
    model = ModelBuilder(cfg)
    sd = model.state_dict()
    assert tuple(sd["encoder.layer1.0.conv2.weight"].shape) == (128, 4, 3, 3)
    assert tuple(sd["encoder.layer4.2.conv2.weight"].shape) == (1024, 32, 3, 3)


def test_unsupported_group_width_is_reported_at_the_first_call_not_at_construction():
    from u2pl_amd import nn as K
    from u2pl_amd._lib import HipError
    conv = K.Conv2d(6, 6, 3, groups=2)                    # 3 channels per group: torch builds it, csrc/gconv.hip cannot run it
    assert tuple(conv.weight.shape) == (6, 3, 3, 3)
    assert "multiple of 4" in K.gconv_constraint(6, 6, 2, 1)
    assert "stride" in K.gconv_constraint(64, 64, 4, 3)
    assert "divisible" in K.gconv_constraint(30, 64, 4, 1)
    assert K.gconv_constraint(128, 128, 32, 2) is None and K.gconv_constraint(36, 36, 3, 1) is None
    assert K.gconv_constraint(32, 32, 32, 1) is not None  # depthwise
    with pytest.raises(HipError):                         # (a CPU tensor: the layer has no CPU fallback either)
        conv(torch.zeros(1, 6, 5, 5))
    with pytest.raises(ValueError):                       # torch's own construction error
        K.Conv2d(6, 8, 3, groups=4)
