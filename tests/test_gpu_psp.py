"""-m gpu: pyramid pooling (csrc/pool.hip, nn._PyramidPoolFn) and the PSPNet decoder (models.decoder.dec_pspnet).

Kernels through the C ABI, element-wise against float64: references, operands, tables and the bounds
|got - ref64| <= EPS min(derived, CAL_MARGIN measured) unit are those of tests/psp_bounds.py; tests/test_psp_cpu.py shows that
these bounds on these tables separate a float32 emulation of the kernels' order from four faulty ones.  x and add are read from
pitched buffers whose gaps hold NaN; every output lies in a sentinel frame that must survive; each call runs twice and must give
the same bits.

The decoder against its float64 twin (F.adaptive_avg_pool2d, F.conv2d, F.batch_norm, F.interpolate): dec_pspnet(in_planes=128,
inner_planes=64, rep_head=True), Dropout2d p = 0, 4 x 128 x 9 x 9, train mode.  Figures: max|got - ref| / max|ref| of pred, rep,
dx and every parameter gradient; yardstick: dec_deeplabv3(in_planes=128, dilations=(1, 2, 12)) against its own twin in the same
test on the same device; every dec_pspnet figure must be <= 2x the largest dec_deeplabv3 figure (the factor of
test_separable_decoder_is_no_worse_than_the_dense_decoder).  Both tables are printed.

The whole path: ResNet-50 + dec_pspnet through ModelBuilder at 65 x 65 (a 9 x 9 decoder input: levels 2 and 6 overlap)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import psp_bounds as B
from decoder_harness import (CL, DEV, SENT, D, Rows, _ptr, _seq64, _twice, assert_default_config_is_untouched,
                             assert_eval_forward_ignores_the_graph, assert_no_worse_than_deeplabv3, assert_replay_equals_eager,
                             build_net, call, decoder_cfg, net_input, step_calls, train_steps)
from model_utils import net_cfg
from split_bounds import EPS, recorded_calls

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FWD, BWD = "u2pl_pyramid_pool_fwd_f32", "u2pl_pyramid_pool_bwd_f32"


def lv4(levels):
    return tuple(levels) + (0,) * (4 - len(levels))


def framed(a, pitched):
    """[N, C, H, W] numpy -> its rows as an input (one image of N H W pixels: the gaps hold NaN)"""
    return Rows((1, a.size // a.shape[1], a.shape[1]), pitched, np.nan, B.rows_of(a))


def raw_fwd(x, levels, pitched):
    """-> {slot: y [N, C, b, b]} through the C ABI, twice, frames checked"""
    N, C, H, W = x.shape
    xin = framed(x, pitched)
    used = dict(B.used(lv4(levels)))

    def run(ys):
        call(FWD, xin.ptr, xin.ld, N, H, W, C, *lv4(levels), *(a for k in range(4) for a in _ptr(ys.get(k))))
    r = _twice("forward level slot", run, lambda: {k: Rows((1, N * b * b, C), pitched, SENT) for k, b in used.items()})
    return {k: B.from_rows(v[0], N, used[k], used[k]) for k, v in r.items()}


def raw_bwd(gs, levels, add, shape, pitched):
    """-> dx [N, C, H, W]; gs: {slot: g}, a missing slot of a used level goes in as a null pointer; add may be None"""
    N, C, H, W = shape
    gin = {k: framed(g, pitched) for k, g in gs.items()}
    ain = None if add is None else framed(add, pitched)

    def run(o):
        call(BWD, *(a for k in range(4) for a in _ptr(gin.get(k))), *_ptr(ain), N, H, W, C, *lv4(levels), *_ptr(o["dx"]))
    return B.from_rows(_twice("backward", run, lambda: dict(dx=Rows((1, N * H * W, C), pitched, SENT)))["dx"][0], N, H, W)


def check_case(N, C, H, W, levels, pitched, variants=True):
    worst = dict(fwd=0.0, bwd=0.0)
    x, gs, add = B.case(N, C, H, W, lv4(levels))
    ys = raw_fwd(x, levels, pitched)
    assert sorted(ys) == [k for k, _ in B.used(lv4(levels))]
    for k, b in B.used(lv4(levels)):
        worst["fwd"] = max(worst["fwd"], B.fwd_excess(ys[k], x, b))
    first = B.used(lv4(levels))[0][0]
    forms = [(gs, add)]
    if variants:
        forms += [(gs, None), ({k: v for k, v in gs.items() if k != first}, add)]       # a null add; a null g for one level
    for g_, a_ in forms:
        dx = raw_bwd(g_, levels, a_, x.shape, pitched)
        worst["bwd"] = max(worst["bwd"], B.bwd_excess(dx, g_, lv4(levels), a_, x.shape))
    return worst


@pytest.mark.parametrize("levels", B.PSP_LEVEL_SETS, ids=str)
@pytest.mark.parametrize("HW", B.PSP_HW, ids=lambda s: "x".join(map(str, s)))
def test_kernels_hold_the_float64_bounds(HW, levels):
    worst = dict(fwd=0.0, bwd=0.0)
    for N in B.PSP_N:
        for C in B.PSP_C:
            w = check_case(N, C, *HW, levels, pitched=(N == 3) == (C % 8 == 4))
            worst = {k: max(worst[k], w[k]) for k in worst}
    print("\n  pyramid pool %s %s: largest error / bound  forward %.3f  backward %.3f" % (HW, levels, worst["fwd"], worst["bwd"]), end="")
    assert worst["fwd"] <= 1.0 and worst["bwd"] <= 1.0, worst


def test_first_size_past_the_forward_grid_cap():
    c = B.FWD_STRIDE_CASE
    x, _, _ = B.case(c["N"], c["C"], *c["HW"], c["levels"])
    for pitched in (False, True):
        ys = raw_fwd(x, c["levels"], pitched)
        worst = max(B.fwd_excess(ys[k], x, b) for k, b in B.used(c["levels"]))
        print("\n  forward, %d work items: %.3f" % (c["N"] * 50 * c["C"] // B.FWD_CHANNELS, worst), end="")
        assert worst <= 1.0


def test_first_size_past_the_backward_grid_cap_and_past_one_pass_of_a_wave():
    for c in (B.BWD_STRIDE_CASE, B.BWD_CHANNEL_CASE):
        x, gs, add = B.case(c["N"], c["C"], *c["HW"], lv4(c["levels"]))
        dx = raw_bwd(gs, c["levels"], add, x.shape, c["C"] < 64)
        worst = B.bwd_excess(dx, gs, lv4(c["levels"]), add, x.shape)
        print("\n  backward, %d pixels of %d channels: %.3f" % (x.size // c["C"], c["C"], worst), end="")
        assert worst <= 1.0
    c = B.BWD_STRIDE_CASE
    assert c["N"] * c["HW"][0] * -(-c["HW"][1] // B.BWD_SEG) > B.BWD_GRID_CAP and B.BWD_CHANNEL_CASE["C"] > B.BWD_LANE_CHANNELS


def test_out_of_contract_arguments_return_1001_and_leave_the_outputs_alone():
    from u2pl_amd._lib import HipError
    x = torch.ones(4 * 6 * 8, device=DEV)
    outs = [torch.full((36 * 8,), float(SENT), device=DEV) for _ in range(4)]
    dx = torch.full((4 * 6 * 8,), float(SENT), device=DEV)
    ya = [a for o in outs for a in (o, 8)]
    bad = [(FWD, x, 6, 1, 2, 2, 6, 1, 2, 3, 6, *ya),               # C % 4
           (FWD, x, 8, 1, 2, 2, 8, 1, -2, 3, 6, *ya),              # a level < 0
           (FWD, x, 8, 1, 2, 2, 8, 0, 0, 0, 0, *ya),               # all levels 0
           (FWD, None, 8, 1, 2, 2, 8, 1, 2, 3, 6, *ya),            # a null x
           (FWD, x, 8, 1, 2, 2, 8, 1, 2, 3, 6, *ya[:2], None, 8, *ya[4:]),      # a null output of a used level
           (BWD, *ya, x, 6, 1, 2, 2, 6, 1, 2, 3, 6, dx, 6),
           (BWD, *ya, x, 8, 1, 2, 2, 8, 1, 2, -1, 6, dx, 8),
           (BWD, *ya, x, 8, 1, 2, 2, 8, 0, 0, 0, 0, dx, 8),
           (BWD, *ya, x, 8, 1, 2, 2, 8, 1, 2, 3, 6, None, 8)]     # a null dx
    for args in bad:
        with pytest.raises(HipError, match="1001"):
            call(*args)
    torch.cuda.synchronize()
    assert all(bool((o.view(torch.int32) == B.SENTINEL_BITS).all()) for o in outs + [dx])


# ---- the autograd Function ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,HW,bins", [(3, 20, (7, 10), (1, 2, 3, 6)), (1, 64, (2, 3), (6,)), (2, 260, (13, 11), (2, 3))],
                         ids=["7x10", "2x3", "13x11"])
def test_pyramid_pool_function_gives_the_bits_of_the_raw_calls(N, C, HW, bins):
    from u2pl_amd import nn as K
    x, gs, add = B.case(N, C, *HW, lv4(bins))
    xd = D(x).contiguous(memory_format=CL).requires_grad_(True)
    with recorded_calls(K) as seen:
        outs = K.pyramid_pool(xd, bins)
        assert len(outs) == 1 + len(bins) and all(o.requires_grad for o in outs)
        assert outs[0].data_ptr() == xd.data_ptr() and outs[0].shape == xd.shape      # handed through, not copied
        torch.autograd.backward(outs, [D(add).contiguous(memory_format=CL)] + [D(gs[k]).contiguous(memory_format=CL)
                                                                               for k in range(len(bins))])
    torch.cuda.synchronize()
    assert {k: len(v) for k, v in seen.items()} == {FWD: 1, BWD: 1}
    ys = raw_fwd(x, bins, False)
    for k in range(len(bins)):
        assert outs[1 + k].is_contiguous(memory_format=CL) or outs[1 + k].shape[2] == 1
        assert B.bits_equal(outs[1 + k].detach().cpu().numpy(), ys[k]), k
    assert B.bits_equal(xd.grad.cpu().numpy(), raw_bwd(gs, bins, add, x.shape, False))
    # only the pooled outputs used: a null add; only the pass-through used: dx is the incoming gradient
    xd.grad = None
    torch.autograd.backward(K.pyramid_pool(xd, bins)[1:], [D(gs[k]).contiguous(memory_format=CL) for k in range(len(bins))])
    assert B.bits_equal(xd.grad.cpu().numpy(), raw_bwd(gs, bins, None, x.shape, False))
    xd.grad = None
    K.pyramid_pool(xd, bins)[0].backward(D(add).contiguous(memory_format=CL))
    assert B.bits_equal(xd.grad.cpu().numpy(), add)


def test_bins_are_checked_before_any_call():
    from u2pl_amd import nn as K
    x = torch.zeros(1, 4, 2, 2, device=DEV)
    for bins in ((), (1, 2, 3, 4, 5), (0,), (2, -1)):
        with pytest.raises(ValueError):
            K.pyramid_pool(x, bins)


def test_concat_consumer_gradient_goes_in_as_the_add_operand():
    """x -> (x_pass, p_i); cat(x_pass, up(p_i)) -> loss: the slice of the concat's gradient reaches the gather kernel as `add`
    (no copy: its pitch is the concat's width), and x.grad is add + pooled part within the backward bound, whose count holds
    exactly one rounding for the add"""
    from u2pl_amd import nn as K
    N, C, H, W, bins = 3, 20, 7, 10, (1, 2, 3, 6)
    x, _, _ = B.case(N, C, H, W, bins)
    G = np.random.default_rng(5).standard_normal((N, 5 * C, H, W), dtype=f32)
    xd = D(x).contiguous(memory_format=CL).requires_grad_(True)
    Gd = D(G).contiguous(memory_format=CL)
    with recorded_calls(K) as seen:
        x_pass, *ps = K.pyramid_pool(xd, bins)
        feat = K.cat_channels((x_pass, *(K.upsample_bilinear(p, (H, W)) for p in ps)))
        feat.backward(Gd)
    torch.cuda.synchronize()
    assert len(seen[BWD]) == 1
    a = seen[BWD][0]
    gts, add_t, ldadd = [a[0], a[2], a[4], a[6]], a[8], a[9]
    assert ldadd == 5 * C and add_t.data_ptr() == Gd.data_ptr()                       # the slice itself, at the concat's pitch
    assert not [args for args in seen.get("u2pl_copy_rows_f32", []) if args[6]]       # no accumulating copy anywhere
    assert [tuple(g.shape) for g in gts] == [(N, C, b, b) for b in bins]
    gs = {k: np.ascontiguousarray(g.detach().cpu().numpy()) for k, g in enumerate(gts)}
    add = G[:, :C]
    e = B.bwd_excess(xd.grad.cpu().numpy(), gs, bins, add, x.shape)
    print("\n  x.grad against add + pooled part in float64: %.3f of the bound" % e, end="")
    assert e <= 1.0
    assert B.bits_equal(xd.grad.cpu().numpy(), raw_bwd(gs, bins, add, x.shape, False))
    # and against the whole route in float64 (bilinear backward included), loosely: the pooled part's operands are fp32 results
    xt = torch.from_numpy(x.astype(f64)).requires_grad_(True)
    twin = torch.cat([xt] + [F.interpolate(F.adaptive_avg_pool2d(xt, b), size=(H, W), mode="bilinear", align_corners=True)
                             for b in bins], 1)
    twin.backward(torch.from_numpy(G.astype(f64)))
    assert float((torch.from_numpy(xd.grad.cpu().numpy().astype(f64)) - xt.grad).abs().max()) <= 64 * EPS * float(xt.grad.abs().max())


# ---- the decoder against its float64 twin -------------------------------------------------------------------------------------
def _psp_twin(dec, p, x):
    h, w = x.shape[2:]
    ups = [F.interpolate(_seq64(m, p, "ppm.%d" % i, x), size=(h, w), mode="bilinear", align_corners=True)
           for i, m in enumerate(dec.ppm)]
    feat = _seq64(dec.head, p, "head", torch.cat([x] + ups, 1))
    pred = F.conv2d(feat, p["classifier.weight"], p["classifier.bias"])
    return dict(pred=pred, rep=_seq64(dec.representation, p, "representation", feat))


def test_pspnet_decoder_is_no_worse_than_the_deeplabv3_decoder():
    from u2pl_amd.models.decoder import dec_pspnet
    assert_no_worse_than_deeplabv3(
        "dec_pspnet", lambda: dec_pspnet(in_planes=128, inner_planes=64, rep_head=True), _psp_twin, ("pred", "rep"),
        {"pred", "rep", "dx", "ppm.0.1.weight", "ppm.3.2.bias", "head.0.weight", "classifier.bias", "representation.4.weight"},
        show_v3=True)


# ---- the whole path -----------------------------------------------------------------------------------------------------------
PSP_DECODER = dict(type="u2pl.models.decoder.dec_pspnet", kwargs=dict(rep_head=True))


@pytest.fixture(scope="module")
def pspnet():
    return build_net(decoder_cfg(PSP_DECODER)), net_input()


def test_pspnet_train_step_reaches_every_parameter(pspnet):
    from u2pl_amd import nn as K
    model, x = pspnet
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    seen, _ = step_calls(model, x)
    assert len(seen[FWD]) == 1 and len(seen[BWD]) == 1
    assert seen[FWD][0][2:10] == (4, 9, 9, 2048, 1, 2, 3, 6) and seen[BWD][0][8] is not None      # the add operand is there
    missing = [n_ for n_, p in model.named_parameters() if p.grad is None]
    assert not missing, missing
    bad = [n_ for n_, p in model.named_parameters() if not bool(torch.isfinite(p.grad).all())]
    zero = [n_ for n_, p in model.named_parameters() if not bool(p.grad.ne(0).any())]
    assert not bad and not zero, (bad, zero)
    before = [p.detach().clone() for p in model.parameters()]
    opt.step()
    K.invalidate_weights()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))


def test_pspnet_eval_forward_is_the_same_with_and_without_a_graph(pspnet):
    assert_eval_forward_ignores_the_graph(pspnet)


def test_pspnet_state_dict_round_trip_gives_the_same_forward(pspnet):
    from u2pl_amd.models.model_helper import ModelBuilder
    model, x = pspnet
    fresh = build_net(decoder_cfg(PSP_DECODER), seed=99)
    fresh.load_state_dict(model.state_dict())
    model.eval(), fresh.eval()
    try:
        with torch.no_grad():
            a, b = model(x), fresh(x)
        for k in ("pred", "rep"):
            assert torch.equal(a[k], b[k]), k
    finally:
        model.train()
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key|size mismatch"):
        fresh.load_state_dict(ModelBuilder(net_cfg("resnet50", 19, True)).state_dict())


def test_default_config_makes_no_pyramid_pool_call_and_the_same_calls_after_a_pspnet_step(pspnet):
    assert_default_config_is_untouched(pspnet, FWD, "u2pl_pyramid_pool")


def test_pspnet_graph_replay_is_bit_identical_to_eager(monkeypatch):
    a, b = (train_steps(monkeypatch, on, lambda cfg: cfg["net"].update(decoder=PSP_DECODER)) for on in (True, False))
    print("graph stats", a["stats"])
    assert_replay_equals_eager(a, b)


