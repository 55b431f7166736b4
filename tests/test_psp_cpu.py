"""Pyramid pooling without a GPU: the window rule of tests/psp_bounds.py is torch's; its inverse is the contiguous range the
backward kernel walks; the numpy fp32 emulations of both kernels' own order meet their bounds on every shape of the tables; four
named faulty emulations leave them; the calibrated ceilings are re-measured from torch's own fp32 arithmetic (-s -k ceilings
prints them); dec_pspnet builds with the documented keys, refuses what the kernels refuse and routes its inputs.  (The HIP
kernels are held to the same bounds in tests/test_gpu_psp.py.)"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psp_bounds as B  # noqa: E402
from model_utils import net_cfg  # noqa: E402
from u2pl_amd import nn as K  # noqa: E402
from u2pl_amd.models.decoder import dec_pspnet  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_HIP = open(os.path.join(ROOT, "u2pl_amd", "csrc", "pool.hip")).read()      # the kernels this file's emulations restate

f32, f64 = np.float32, np.float64
T = torch.from_numpy
CPU_C = (4, 20)         # the emulations are loops over pixels: the channel edges (tiles of 64, C = 260) are the GPU file's


# ------------------------------------------------------------------ the window rule and its inverse
@pytest.mark.parametrize("b", B.RULE_B)
def test_window_rule_is_torchs(b):
    for H in B.RULE_H:
        for W in (H, B.RULE_H[(B.RULE_H.index(H) + 3) % len(B.RULE_H)]):
            x = np.random.default_rng([H, W, b]).standard_normal((2, 3, H, W))
            ref = F.adaptive_avg_pool2d(T(x), b).numpy()
            y, _, area = B.fwd64(x, b)
            assert np.abs(y - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max()), (H, W, b)
            assert area.min() >= 1
        w = [B.window(i, H, b) for i in range(b)]
        assert w[0][0] == 0 and w[-1][1] == H and all(0 <= s < e <= H for s, e in w)
        assert all(w[i + 1][0] <= w[i][1] for i in range(b - 1))                 # no gap
        if H % b and b <= H:
            assert any(w[i + 1][0] == w[i][1] - 1 for i in range(b - 1)), (H, b)   # a shared row


@pytest.mark.parametrize("b", B.RULE_B + (4, 5, 7, 12))
def test_cover_is_the_inverse_of_the_window_rule(b):
    for H in B.RULE_H:
        for h in range(H):
            inside = [i for i in range(b) if B.window(i, H, b)[0] <= h < B.window(i, H, b)[1]]
            lo, hi = B.cover(h, H, b)
            assert inside == list(range(lo, hi + 1)) and inside, (H, b, h)
            if b <= H:
                assert len(inside) <= 2
            else:
                assert len(inside) <= -(-b // H) + 1
    # b > H: a pixel lies in more than two windows (the range is not capped at two)
    assert B.cover(0, 1, 6) == (0, 5) and B.cover(1, 2, 6) == (3, 5)


def test_backward_reference_is_torchs_autograd_in_float64():
    for (H, W) in B.PSP_HW:
        x, gs, add = B.case(2, 4, H, W, (1, 2, 3, 6))
        xt = T(x.astype(f64)).requires_grad_(True)
        loss = (xt * T(add.astype(f64))).sum()
        for k, b in B.used((1, 2, 3, 6)):
            loss = loss + (F.adaptive_avg_pool2d(xt, b) * T(gs[k].astype(f64))).sum()
        loss.backward()
        dx, unit, cnt = B.bwd64(gs, (1, 2, 3, 6), add, x.shape)
        assert np.abs(dx - xt.grad.numpy()).max() <= 1e-13 * unit.max()
        assert cnt.min() >= 4 and (unit >= np.abs(dx) - 1e-12).all()


# ------------------------------------------------------------------ the faithful emulations inside their bounds
@pytest.mark.parametrize("levels", B.PSP_LEVEL_SETS, ids=str)
@pytest.mark.parametrize("HW", B.PSP_HW, ids=lambda s: "x".join(map(str, s)))
def test_emulations_of_the_kernels_order_hold_the_bounds(HW, levels):
    for N in B.PSP_N:
        for C in CPU_C:
            x, gs, add = B.case(N, C, *HW, levels)
            for k, b in B.used(levels):
                e = B.fwd_excess(B.emu_fwd(x, b), x, b)
                assert e <= 1.0, ("forward", N, C, b, e)
            for g_, a_ in ((gs, add), (gs, None), ({k: v for k, v in gs.items() if k != B.used(levels)[0][0]}, add)):
                e = B.bwd_excess(B.emu_bwd(g_, levels, a_, x.shape), g_, levels, a_, x.shape)
                assert e <= 1.0, ("backward", N, C, sorted(g_), a_ is None, e)


def test_torch_fp32_holds_the_bounds_where_the_calibrated_term_decides():
    """the bound is min(derived, CAL_MARGIN measured): torch's own order (one add per pixel of the window) stays inside it
    wherever its rounding count is not above the kernel's"""
    for HW in B.PSP_HW[:6]:
        x, gs, add = B.case(3, 20, *HW, (1, 2, 3, 6))
        assert B.bwd_excess(B.torch_bwd_fp32(gs, (1, 2, 3, 6), add, x.shape), gs, (1, 2, 3, 6), add, x.shape) <= 1.0


def test_counts_are_the_roundings_of_the_order():
    assert list(B.fwd_count([1, 2, 3, 16, 17, 1155, 9409])) == [1, 2, 3, 5, 6, 77, 593]
    assert list(B.bwd_count([0, 1, 4, 13], True)) == [1, 3, 6, 15] and list(B.bwd_count([0, 1, 4], False)) == [0, 2, 5]


# ------------------------------------------------------------------ the calibrated ceilings, re-measured
def test_ceilings_are_what_torch_fp32_reaches():
    tor, emu = B.measure("torch"), B.measure("emu")
    print()
    for name, t, e in zip(("CAL_PSP_FWD", "CAL_PSP_BWD"), tor, emu):
        print(f"  {name:12s} = {getattr(B, name):<5}  torch fp32 {t:.2f}   [emulation {e:.2f}]")
        assert t <= getattr(B, name) <= 2 * t, (name, t)
        assert e <= B.CAL_MARGIN * getattr(B, name)


# ------------------------------------------------------------------ the bounds reject faulty arithmetic
def test_fault_window_end_rounded_down_drops_the_shared_row():
    """end = floor((i + 1) H / b): at 7 x 10 with 3 levels per axis the windows lose their last row; 6 x 6 with b = 3 has none to lose"""
    x, _, _ = B.case(3, 20, 7, 10, (1, 2, 3, 6))
    assert B.fwd_excess(B.emu_fwd(x, 3), x, 3) <= 1.0
    assert B.fwd_excess(B.emu_fwd(x, 3, fault="end_floor"), x, 3) > 100.0
    assert B.fwd_excess(B.emu_fwd(x, 2, fault="end_floor"), x, 2) > 100.0          # 7 % 2 != 0 on one axis only
    x, _, _ = B.case(3, 20, 6, 6, (1, 2, 3, 6))
    assert B.bits_equal(B.emu_fwd(x, 3, fault="end_floor"), B.emu_fwd(x, 3))


def test_fault_division_by_the_nominal_area():
    """(H / b)(W / b) is not the size of a window when H % b != 0: 13 x 11 at b = 2, 3 and 6"""
    x, _, _ = B.case(3, 20, 13, 11, (1, 2, 3, 6))
    for b in (2, 3, 6):
        assert B.fwd_excess(B.emu_fwd(x, b, fault="nominal_area"), x, b) > 100.0, b
    assert B.fwd_excess(B.emu_fwd(x, 1, fault="nominal_area"), x, 1) <= 1.0        # one window: nominal = true


def test_fault_backward_visits_one_window_per_axis():
    """a pixel of a shared row lies in two windows per axis (33 x 35, b = 2, 3, 6); at 6 x 6 no window shares anything"""
    lv = (1, 2, 3, 6)
    x, gs, add = B.case(3, 20, 33, 35, lv)
    assert B.bwd_excess(B.emu_bwd(gs, lv, add, x.shape), gs, lv, add, x.shape) <= 1.0
    got = B.emu_bwd(gs, lv, add, x.shape, fault="one_window_per_axis")
    assert B.bwd_excess(got, gs, lv, add, x.shape) > 100.0
    dx, unit, cnt = B.bwd64(gs, lv, add, x.shape)
    wrong = np.abs(got - dx) > B.E_bwd(cnt, True)[None, None] * unit
    assert wrong.any((0, 1))[cnt > 4].all() and not wrong[:, :, cnt == 4].any()    # exactly the pixels of shared rows and columns
    x, gs, add = B.case(3, 20, 6, 6, lv)
    assert B.bits_equal(B.emu_bwd(gs, lv, add, x.shape, fault="one_window_per_axis"), B.emu_bwd(gs, lv, add, x.shape))
    x, gs, add = B.case(1, 4, 2, 3, (6,))                                          # b > H: up to three windows per axis
    assert B.bwd_excess(B.emu_bwd(gs, (6,), add, x.shape, fault="one_window_per_axis"), gs, (6,), add, x.shape) > 100.0


def test_fault_backward_takes_the_area_from_another_level():
    lv = (1, 2, 3, 6)
    for HW in ((5, 6), (13, 11)):
        x, gs, add = B.case(3, 20, *HW, lv)
        assert B.bwd_excess(B.emu_bwd(gs, lv, add, x.shape, fault="area_of_another_level"), gs, lv, add, x.shape) > 100.0
    x, gs, add = B.case(3, 20, 5, 6, (1, 1, 1, 1))                                 # four equal levels: nothing to confuse
    assert B.bwd_excess(B.emu_bwd(gs, (1, 1, 1, 1), add, x.shape, fault="area_of_another_level"), gs, (1, 1, 1, 1), add,
                        x.shape) <= 1.0


def test_tables_use_the_constants_of_the_kernels():
    import re
    defs = {k: int(v) for k, v in re.findall(r"#define (PSP_\w+) (\d+)", POOL_HIP)}
    assert defs["PSP_LANES"] == B.FWD_LANES and defs["PSP_CH4"] * 4 == B.FWD_CHANNELS
    assert defs["PSP_FWD_MAX_BLOCKS"] == B.FWD_GRID_CAP and 64 * defs["PSP_KC"] * 4 == B.BWD_LANE_CHANNELS and defs["PSP_SEG"] == B.BWD_SEG
    assert K.PSP_MAX_LEVELS == 4 == max(len(lv) for lv in B.PSP_LEVEL_SETS)
    from u2pl_amd._lib import parse_header
    decl = parse_header()
    assert len(decl["u2pl_pyramid_pool_fwd_f32"][1]) == 19 and len(decl["u2pl_pyramid_pool_bwd_f32"][1]) == 21


def test_stride_cases_are_past_the_grid_caps():
    c = B.FWD_STRIDE_CASE
    items = c["N"] * sum(b * b for b in c["levels"]) * -(-c["C"] // B.FWD_CHANNELS)
    assert B.FWD_GRID_CAP < items < B.FWD_GRID_CAP + 64
    c = B.BWD_STRIDE_CASE
    assert B.BWD_GRID_CAP < c["N"] * c["HW"][0] * -(-c["HW"][1] // B.BWD_SEG) < B.BWD_GRID_CAP + 512
    assert B.BWD_CHANNEL_CASE["C"] == B.BWD_LANE_CHANNELS + 4


# ------------------------------------------------------------------ dec_pspnet
def psp_keys(in_planes=2048, num_classes=19, inner=512, bins=(1, 2, 3, 6), rep=False):
    keys, red = {}, in_planes // len(bins)

    def bn(prefix, c):
        keys.update({prefix + ".weight": (c,), prefix + ".bias": (c,), prefix + ".running_mean": (c,),
                     prefix + ".running_var": (c,), prefix + ".num_batches_tracked": ()})
    for i in range(len(bins)):
        keys["ppm.%d.1.weight" % i] = (red, in_planes, 1, 1)
        bn("ppm.%d.2" % i, red)
    keys["head.0.weight"] = (inner, 2 * in_planes, 3, 3)
    bn("head.1", inner)
    keys.update({"classifier.weight": (num_classes, inner, 1, 1), "classifier.bias": (num_classes,)})
    if rep:
        keys["representation.0.weight"] = (256, inner, 3, 3)
        bn("representation.1", 256)
        keys.update({"representation.4.weight": (256, 256, 1, 1), "representation.4.bias": (256,)})
    return keys


@pytest.mark.parametrize("rep", [False, True])
def test_dec_pspnet_builds_with_the_documented_keys(rep):
    dec = dec_pspnet(in_planes=2048, rep_head=rep)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == psp_keys(rep=rep)
    assert [type(m[0]) for m in dec.ppm] == [torch.nn.AdaptiveAvgPool2d] * 4
    assert [m[0].output_size for m in dec.ppm] == [1, 2, 3, 6]
    assert isinstance(dec.head[3], torch.nn.Dropout2d) and dec.head[3].p == 0.1
    dec = dec_pspnet(in_planes=96, num_classes=21, inner_planes=64, bins=(2, 4, 8), rep_head=rep)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == psp_keys(96, 21, 64, (2, 4, 8), rep)


def test_dec_pspnet_refuses_what_the_kernels_refuse():
    with pytest.raises(ValueError, match="one to 4 levels"):
        dec_pspnet(in_planes=2560, bins=(1, 2, 3, 6, 8))
    with pytest.raises(ValueError, match="one to 4 levels"):
        dec_pspnet(in_planes=2048, bins=())
    with pytest.raises(ValueError, match=">= 1"):
        dec_pspnet(in_planes=2048, bins=(1, 0, 3, 6))
    with pytest.raises(ValueError, match=">= 1"):
        dec_pspnet(in_planes=2048, bins=(-2,))
    with pytest.raises(ValueError, match="multiple of 4"):
        dec_pspnet(in_planes=2040)              # 2040 / 4 = 510 channels per branch: no float4 rows
    with pytest.raises(ValueError, match="multiple of 4"):
        dec_pspnet(in_planes=64, bins=(1, 2, 3))
    dec_pspnet(in_planes=48, bins=(1, 2, 3))


def test_dec_pspnet_resolves_through_the_alias_package_and_model_builder():
    import importlib
    from u2pl_amd.models.model_helper import ModelBuilder
    assert importlib.import_module("u2pl.models.decoder").dec_pspnet is dec_pspnet
    cfg = net_cfg("resnet50", 19, True)
    cfg["decoder"] = dict(type="u2pl.models.decoder.dec_pspnet", kwargs=dict(rep_head=True))
    model = ModelBuilder(cfg)
    assert isinstance(model.decoder, dec_pspnet) and model.decoder.bins == (1, 2, 3, 6)
    sd = model.state_dict()
    assert tuple(sd["decoder.head.0.weight"].shape) == (512, 4096, 3, 3)
    assert tuple(sd["decoder.representation.4.weight"].shape) == (256, 256, 1, 1)
    assert tuple(sd["auxor.aux.0.weight"].shape) == (256, 1024, 3, 3)


def _torch_ops(monkeypatch):
    """the decoder's wiring without a GPU: every u2pl_amd.nn operation it calls replaced by the torch function it stands for, and
    the calls recorded (the HIP operations themselves are tests/test_gpu_psp.py's)"""
    seen = []

    def seq(s, x):
        for m in s:
            if isinstance(m, K.Conv2d):
                x = F.conv2d(x, m.weight, m.bias, padding=m.padding)
            elif isinstance(m, K.BatchNorm2d):
                x = F.batch_norm(x, None, None, m.weight, m.bias, training=True)
            elif isinstance(m, torch.nn.ReLU):
                x = torch.relu(x)
        return x

    def pyramid_pool(x, bins):
        seen.append(("pyramid_pool", tuple(x.shape), tuple(bins)))
        return (x,) + tuple(F.adaptive_avg_pool2d(x, b) for b in bins)

    def group(units):
        seen.append(("conv_bn_group", len(units)))
        return [torch.relu(F.batch_norm(F.conv2d(x, c.weight), None, None, b.weight, b.bias, training=True)) for c, b, x, r, d in units]

    def up(x, size):
        seen.append(("upsample", tuple(x.shape[2:]), tuple(size)))
        return F.interpolate(x, size=size, mode="bilinear", align_corners=True)
    monkeypatch.setattr(K, "pyramid_pool", pyramid_pool)
    monkeypatch.setattr(K, "conv_bn_group", group)
    monkeypatch.setattr(K, "upsample_bilinear", up)
    monkeypatch.setattr(K, "cat_channels", lambda ts: torch.cat(tuple(ts), 1))
    monkeypatch.setattr(K, "run_seq", lambda s, x, grad_link=None: seq(s, x))
    monkeypatch.setattr(K.Conv2d, "forward", lambda self, x: F.conv2d(x, self.weight, self.bias, padding=self.padding))
    return seen


def test_dec_pspnet_output_dict_on_the_fpn_list_and_on_a_single_tensor(monkeypatch):
    seen = _torch_ops(monkeypatch)
    torch.manual_seed(0)
    x = torch.randn(2, 32, 9, 7)
    others = [torch.randn(2, 8, 17, 13), torch.randn(2, 16, 9, 7), torch.randn(2, 24, 9, 7)]
    dec = dec_pspnet(in_planes=32, num_classes=5, inner_planes=16, rep_head=True)
    a = dec(x)
    assert sorted(a) == ["pred", "rep"] and a["pred"].shape == (2, 5, 9, 7) and a["rep"].shape == (2, 256, 9, 7)
    assert seen[0] == ("pyramid_pool", (2, 32, 9, 7), (1, 2, 3, 6)) and seen[1] == ("conv_bn_group", 4)
    assert [s for s in seen if s[0] == "upsample"] == [("upsample", (b, b), (9, 7)) for b in (1, 2, 3, 6)]
    b = dec(others + [x])                       # the encoder's four maps: the last one is read
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert sorted(dec(others + [x], need_rep=False)) == ["pred"]
    plain = dec_pspnet(in_planes=32, num_classes=5, inner_planes=16)
    assert sorted(plain(x)) == ["pred"] and sorted(plain(x, need_rep=True)) == ["pred"] and not hasattr(plain, "representation")


def test_pspnet_example_config_names_the_decoder():
    import yaml
    from u2pl_amd.models.model_helper import ModelBuilder
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tools", "city_semi_pspnet_example.yaml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(root, "tools", "city_semi_template.yaml")) as f:
        base = yaml.safe_load(f)
    assert cfg["net"]["decoder"] == dict(type="u2pl.models.decoder.dec_pspnet",
                                         kwargs=dict(inner_planes=512, bins=[1, 2, 3, 6], rep_head=True))
    cfg["net"]["decoder"] = base["net"]["decoder"]
    assert cfg == base                          # the template with the decoder swapped, nothing else
    with open(os.path.join(root, "tools", "city_semi_pspnet_example.yaml")) as f:
        net = yaml.safe_load(f)["net"]
    net["sync_bn"] = False
    net["encoder"]["type"] = "u2pl.models.resnet.resnet50"
    net["encoder"]["kwargs"]["pretrained"] = False
    assert "decoder.representation.4.bias" in ModelBuilder(net).state_dict()
