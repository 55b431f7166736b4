"""Grouped convolutions (ResNeXt encoders), the parts that need no GPU: K.Conv2d(groups=g) draws the parameters torch.nn.Conv2d
draws and exchanges state_dicts with it, the encoder builds with the reference's `groups` / `width_per_group` keywords (also
through ModelBuilder), BasicBlock keeps upstream's ValueError, and the shape constraints of csrc/gconv.hip are reported at the
first call rather than at construction (torch.nn.Conv2d constructs such layers too).

The contract of tests/gconv_bounds.py: its table holds every path of the three kernels (asserted below, edge by edge), a numpy float32
emulation of the kernels' addressing holds the float64 bound on every case, each of seven one-line faults breaks the bound on a
new case and passes on the table tests/test_gpu_gconv.py ran before (so that table could not have seen it), and the library's
workspace query and refusals (no launch is reachable from them) agree with the restated plan and the header's contract."""
import ctypes

import pytest
import torch

import gconv_bounds as B
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


# ---- the table of tests/gconv_bounds.py holds the edges the kernels have ------------------------------------------------------------
def _plan(case):
    g, ci, co, R, S = case[:5]
    return B.wgrad_plan(B.pixels(case)[0], g, ci, co, R * S)


def test_table_holds_every_width_tap_and_pixel_edge():
    old, new = B.old_table(), B.new_cases()
    assert B.shape_list() == old + new and len(set(old + new)) == len(old + new)
    assert len(old) == len(B.WIDTHS) * len(B.GEOMS) + 1
    assert all(c[1] == c[2] and c[3] == c[4] and c[3] * c[4] in (1, 9) and B.out_hw(c)[1] >= 4 for c in old)      # what it could not see
    # cig != cog in both orders
    assert any(c[1] < c[2] for c in new) and any(c[1] > c[2] for c in new)
    # every tile count 1..4 on either side, a partial last tile for each of 2, 3, 4 (JT of the forward and of the weight gradient from
    # cog; JT of the data gradient and CT of the weight gradient from cig), and JT != CT in both orders
    for side in (1, 2):
        widths = {c[side] for c in old + new}
        assert {B.col_tiles(c) for c in widths} == {1, 2, 3, 4}, side
        for tiles in (2, 3, 4):
            assert any(B.col_tiles(c) == tiles and c % 16 for c in widths), (side, tiles)
            assert any(B.col_tiles(c) == tiles and c % 16 == 0 for c in widths), (side, tiles)
    assert any(B.col_tiles(c[1]) < B.col_tiles(c[2]) for c in new) and any(B.col_tiles(c[1]) > B.col_tiles(c[2]) for c in new)
    assert all(c[1] % 4 == 0 and c[2] % 4 == 0 and c[1] <= 64 and c[2] <= 64 for c in old + new)
    # every width: stride 1, and stride 2 with dilation 2, on odd and on even extents
    for g, ci, co in B.NEW_WIDTHS:
        mine = [c for c in new if c[:3] == (g, ci, co) and c[3:5] == (3, 3)]
        assert any(c[7] == 1 for c in mine) and any(c[7] == 2 and c[9] == 2 for c in mine)
        assert any(c[5] % 2 and c[6] % 2 for c in mine) and any(c[5] % 2 == 0 and c[6] % 2 == 0 for c in mine)
    assert {(c[5], c[6]) for c in new if c[:3] == (2, 64, 60)} == {(13, 11), (9, 17)} and all(c[3:5] == (1, 1) for c in new if c[1] == 64)
    # filter shapes: R != S in both orders, R * S outside {1, 9} (one tap per wave), R * S = 121, Hout != Hin on one axis only
    shapes = {c[3:5] for c in new}
    assert {(5, 5), (1, 7), (7, 1), (3, 5), (2, 2), (11, 11)} <= shapes
    assert any(c[3:5] == (5, 5) and c[7] == 2 and c[9] == 2 for c in new) and any(c[3:5] == (2, 2) and c[7] == 2 and c[8] == 0 for c in new)
    for c in new:
        assert (_plan(c)[3] > 1) == (c[3] * c[4] not in (1, 9)) and _plan(c)[3] in (1, c[3] * c[4])
        if c[3:5] == (1, 7):
            assert B.out_hw(c) == (c[5] + 6, c[6])
        if c[3:5] == (7, 1):
            assert B.out_hw(c) == (c[5], c[6] + 6)
    assert B.BIG_KERNEL_CASE in new and B.BIG_KERNEL_CASE[3] * B.BIG_KERNEL_CASE[4] == 121 and B.BIG_KERNEL_CASE[5:7] == (9, 9)
    # pixel counts: 5 pixels of 1x1 images, both sides of 32 and of 128, fewer than 32
    ms = {B.pixels(c)[0] for c in new if c[:5] == (4, 8, 16, 3, 3) and c[7:10] == (1, 1, 1)}
    assert {5, 31, 32, 33, 127, 128, 129} <= ms
    assert all(B.pixels(c)[0] == B.pixels(c)[1] for c in new if c[:5] == (4, 8, 16, 3, 3) and c[7:10] == (1, 1, 1))
    assert any(c[5:7] == (1, 1) and c[10] == 5 for c in new)
    # the pixel walk: Wout < 4 with more than one slab; 130 images of 1x1 in three slabs; Wout = 3 in four slabs of 52, edges inside rows
    assert any(B.out_hw(c)[1] < 4 and _plan(c)[1] > 1 for c in new)
    assert B.out_hw(B.WALK_CASE_IMAGES) == (1, 1) and _plan(B.WALK_CASE_IMAGES)[:2] == (44, 3)
    assert B.out_hw(B.WALK_CASE_NARROW) == (23, 3) and _plan(B.WALK_CASE_NARROW)[:2] == (52, 4) and 52 % 3
    # the slab cap: ns is cut at 512 and all 512 slabs are there, their edges inside image rows
    g, ci, co = B.SLAB_CAP_CASE[:3]
    M = B.pixels(B.SLAB_CAP_CASE)[0]
    rows, NS, tiles, ntc = _plan(B.SLAB_CAP_CASE)
    assert M > 64 * 512 and B.cdiv(8192, tiles) > 512 and NS == 512 and (NS - 1) * rows < M and B.out_hw(B.SLAB_CAP_CASE)[1] % rows
    assert max(_plan(c)[1] for c in old) == 5                                   # (the old table: five slabs at most)
    # both remap states for y and for dx, in the new cases alone
    for side in (0, 1):
        assert {B.conv_blocks(B.pixels(c)[side], c[0])[1] for c in new} == {True, False}, side
    # the table stays small: a few hundred pixels but for the slab cap
    assert all(max(B.pixels(c)) <= 640 for c in new if c != B.SLAB_CAP_CASE)


def test_restated_plans_hold_their_invariants():
    for M in list(range(1, 700)) + [32767, 32768, 32769, 34816, 10 ** 6]:
        for g, ci, co, RS in ((4, 8, 16, 9), (2, 4, 4, 9), (32, 4, 4, 9), (2, 64, 60, 1), (8, 4, 12, 25), (2, 4, 8, 121), (3, 20, 52, 9)):
            rows, NS, tiles, ntc = B.wgrad_plan(M, g, ci, co, RS)
            assert rows % 4 == 0 and 1 <= NS <= 512 and (NS - 1) * rows < M <= NS * rows, (M, g, ci, co, RS)
            assert tiles == g * B.col_tiles(co) * B.col_tiles(ci) * ntc and ntc * B.wgrad_family(RS) == RS
        n, remap = B.conv_blocks(M, 4)
        assert (n // 4 - 1) * 128 < M <= (n // 4) * 128 and remap == (n % 8 == 0)


# ---- the bound and the table can tell a wrong kernel from a right one ----------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    """per case: the operands and the float64 references with their bounds (computed once, not modified)"""
    out = {}
    for case in B.shape_list():
        ops = B.operands(case)
        out[case] = (ops, B.refs(case, *ops))
    return out


def test_fp32_emulation_holds_the_bound_on_every_case(table):
    top = {k: 0.0 for k in B.NAMES}
    for case, (ops, refs) in table.items():
        got = B.emulate(case, *ops)
        worst = B.worst(got, refs)
        assert all(v <= 1.0 for v in worst.values()), (B.case_id(case), worst)
        assert all(float(got[k].abs().max()) > 0 for k in got), B.case_id(case)
        assert all(float(refs[k][0].abs().max()) > 0 for k in refs), B.case_id(case)
        top = {k: max(top[k], worst[k]) for k in top}
    print("largest excess of the emulation", {k: round(v, 3) for k, v in top.items()})


def test_torchs_fp32_convolution_holds_the_bound_too(table):
    """the bound holds for a correct fp32 implementation in any summation order: torch's own, on the new cases (it reaches about a
    third of it on the 5-pixel case, where n = 5, and less elsewhere; printed)"""
    import torch.nn.functional as F
    top = {k: 0.0 for k in B.NAMES}
    for case in B.new_cases():
        (x, w, gy), refs = table[case]
        kw = dict(stride=case[7], padding=case[8], dilation=case[9], groups=case[0])
        got = dict(y=F.conv2d(x, w, **kw), dx=torch.nn.grad.conv2d_input(tuple(x.shape), w, gy, **kw),
                   dw=torch.nn.grad.conv2d_weight(x, tuple(w.shape), gy, **kw))
        worst = B.worst(got, refs)
        top = {k: max(top[k], worst[k]) for k in top}
    print("largest excess of torch's fp32 convolution", {k: round(v, 3) for k, v in top.items()})
    assert all(v <= 1.0 for v in top.values()), top


def test_padding_only_taps_of_the_11x11_case_are_exact_zeros(table):
    """dilation 4, pad 20 on a 9x9 map: only the taps r, s in 3..7 meet the map; everywhere else cond and the bound are 0"""
    case = B.BIG_KERNEL_CASE
    ops, refs = table[case]
    bound = refs["dw"][1]
    inside = torch.zeros(11, 11, dtype=torch.bool)
    inside[3:8, 3:8] = True
    assert float(bound[:, :, ~inside].max()) == 0 and float(bound[:, :, inside].amax((0, 1)).min()) > 0
    assert int((~inside).sum()) == 96
    got = B.emulate(case, *ops, names=("dw",))
    assert bool((got["dw"][:, :, ~inside] == 0).all()) and B.worst(got, refs, ("dw",))["dw"] <= 1.0
    broken = {"dw": got["dw"].clone()}
    broken["dw"][3, 1, 0, 10] = 1e-30                         # anything but 0 where only padding is met
    assert B.worst(broken, refs, ("dw",))["dw"] > 1.0


@pytest.mark.parametrize("fault", sorted(B.FAULTS))
def test_each_fault_passes_the_old_table_and_breaks_the_new_one(table, fault):
    names = B.FAULTS[fault]
    for case in B.old_table():                                # the proof that the old table could not see it
        ops, refs = table[case]
        worst = B.worst(B.emulate(case, *ops, fault=fault, names=names), refs, names)
        assert all(v <= 1.0 for v in worst.values()), (fault, B.case_id(case), worst)
    broken = {k: [] for k in names}
    for case in B.new_cases():
        ops, refs = table[case]
        worst = B.worst(B.emulate(case, *ops, fault=fault, names=names), refs, names)
        for k in names:
            if worst[k] > 1.0:
                broken[k].append(B.case_id(case))
    print(fault, {k: len(v) for k, v in broken.items()})
    assert all(broken[k] for k in names), (fault, broken)


# ---- the library against the restatement, and its refusals --------------------------------------------------------------------------
EINVAL = 1001


@pytest.fixture(scope="module")
def L():
    from u2pl_amd._lib import lib
    return lib().cdll


def test_workspace_query_is_the_restated_plan_on_the_whole_table(L):
    for case in B.shape_list():
        g, ci, co, R, S, H, W, stride, pad, dil, N = case
        Ho, Wo = B.out_hw(case)
        assert L.u2pl_gconv2d_wgrad_workspace_bytes(N, Ho, Wo, g * ci, g * co, R, S, g) == B.workspace_bytes(case), B.case_id(case)
    assert L.u2pl_gconv2d_wgrad_workspace_bytes(1, 5, 5, 30, 64, 3, 3, 4) == 0


def _three_entries(L, base, case, ldx=None, ldy=None, Ho=None, shift_x=0, shift_y=0, shift_w=0):
    """the return codes of the three entry points on one geometry; the pointers are 16-byte aligned host addresses that are never
    read (every call of this file returns before a launch), shift_*: bytes added to one of them"""
    g, ci, co, R, S, H, W, stride, pad, dil, N = case
    Cin, Cout = g * ci, g * co
    ho, wo = (B.out_size(H, R, stride, pad, max(dil, 0)), B.out_size(W, S, stride, pad, max(dil, 0)))
    ho = ho if Ho is None else Ho
    ldx, ldy = ldx or Cin, ldy or Cout
    x, y, w, ws = base + shift_x, base + 64 + shift_y, base + 128 + shift_w, base + 192
    geo = (N, H, W, Cin, ho, wo, Cout, R, S, stride, pad, dil, g, None)
    return (L.u2pl_gconv2d_fwd_f32(x, ldx, w, None, y, ldy, *geo), L.u2pl_gconv2d_dgrad_f32(y, ldy, w, x, ldx, *geo),
            L.u2pl_gconv2d_wgrad_f32(y, ldy, x, ldx, w, ws, 0, *geo))


def test_refusals_just_outside_the_contract(L):
    """U2PL_EINVAL from all three entry points, each case one step outside what include/u2pl_hip.h admits (an in-contract call is
    never made here: it would launch)"""
    buf = (ctypes.c_char * 512)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    inside = (2, 8, 16, 3, 3, 20, 20, 1, 1, 1, 1)
    outside = {
        "R * S = 128": dict(case=(2, 8, 16, 8, 16, 20, 20, 1, 0, 1, 1)),
        "S = 17": dict(case=(2, 8, 16, 1, 17, 20, 20, 1, 0, 1, 1)),
        "68 channels per group in": dict(case=(2, 68, 16, 3, 3, 20, 20, 1, 1, 1, 1)),
        "68 channels per group out": dict(case=(2, 8, 68, 3, 3, 20, 20, 1, 1, 1, 1)),
        "ldx % 4": dict(case=inside, ldx=18),
        "ldy % 4": dict(case=inside, ldy=34),
        "ldx < Cin": dict(case=inside, ldx=12),
        "ldy < Cout": dict(case=inside, ldy=28),
        "x off by 4 bytes": dict(case=inside, shift_x=4),
        "y off by 4 bytes": dict(case=inside, shift_y=4),
        "w off by 8 bytes": dict(case=inside, shift_w=8),
        "Hout one too large": dict(case=inside, Ho=21),
        "Hout one too small": dict(case=inside, Ho=19),
        "dil = 0": dict(case=(2, 8, 16, 3, 3, 20, 20, 1, 1, 0, 1)),
        "stride 3": dict(case=(2, 8, 16, 3, 3, 20, 20, 3, 1, 1, 1)),
    }
    assert 8 * 16 == 128 and 7 * 16 < 128                     # (7 x 16 is inside, 8 x 16 is the first filter outside)
    for why, kw in outside.items():
        assert _three_entries(L, base, **kw) == (EINVAL,) * 3, why
