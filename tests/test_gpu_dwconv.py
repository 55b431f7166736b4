"""-m gpu: depthwise 3x3 convolutions (csrc/dwconv.hip, nn._GroupedConvFn on the depthwise route) and the separable DeepLabv3+
decoder (decoder.kwargs.separable).

Kernels against float64: oracle, operands and the bound |got - ref| <= (n + 2) * 2^-24 * cond are those of tests/dw_bounds.py
(n = 9 for y and dx, N*Ho*Wo for dw; cond = 0 asks for an exact 0); tests/test_dwconv_cpu.py shows that this bound on this shape
list separates a float32 emulation of the kernels from three faulty ones.

Tile widths of the kernels as built: one channel tile = 128 channels (32 lanes x 4 channels) in all three kernels; a block of the
forward / data-gradient kernel covers 32 pixels (8 lane groups x 4 pixels); the weight gradient cuts the N*Ho*Wo pixels into
slabs of ceil(M / ns), ns = min(ceil(2048 / channel tiles), ceil(M / 64), 512).  Channels: 4, 8, 124 / 128 / 132 (first tile
edge), 256 / 260 (second edge); 132 and 260 are no multiples of 8.  dw_bounds.SLAB_CASE: 145 pixels in 3 slabs of 49.

The separable decoder against its float64 twin: dec_deeplabv3_plus(in_planes=64, dilations=(1, 2, 12), separable=True) in train
mode (Dropout2d p = 0) against the same network written from F.conv2d / F.batch_norm / relu in float64.  Figures:
max|got - ref| / max|ref| of pred, rep, both input gradients and every parameter gradient; yardstick: the same test on the dense
decoder.  Every figure the two models share (what the option leaves alone: low_conv, aspp.conv1, aspp.conv2, the outputs and the
input gradients) must be <= 2x the dense figure, every separable-only one <= 2x the largest dense figure (the factor of
test_resnext_block_is_no_worse_than_the_dense_block).  Measured on an MI355X: every separable figure <= 4.6e-6; the dense decoder's
outputs and classifier tower <= 8e-6, but its representation.0.weight 8.9e-2 and everything upstream of the towers 0.5-4e-2: the
pattern of one ReLU mask bit flipped at a pre-activation within rounding of zero (it moves to another layer with U2PL_CONV_H=0 or
U2PL_CONV_WINO=0), which makes this yardstick loose on these seeds.  A convolution bias directly in front of a train-mode BatchNorm has a
gradient that is identically zero (the batch mean is subtracted again), so max|ref| is rounding noise of the float64 twin and the
quotient means nothing; for those biases the denominator is max_c sum_pixels |dy| of the twin, the condition of the sum that
produces them.

The whole path: ResNet-50 + the separable DeepLabv3+ decoder through ModelBuilder at 65 x 65."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dw_bounds as B
from decoder_harness import CL, DEV, assert_replay_equals_eager, build_net, decoder_cfg, net_input, step_calls, train_steps
from model_utils import net_cfg
from split_bounds import EPS, recorded_calls

pytestmark = pytest.mark.gpu
STEM = "u2pl_dwconv2d"


def _device_kernels(x_dev, w, gy, stride, pad, dil, bias=None, sink=None):
    """the three C entry points on device tensors; x_dev may be a channel slice of a wider channels_last buffer"""
    from u2pl_amd import nn as K
    from u2pl_amd.layout import _ws, as_rows, new_act
    xr, ldx = as_rows(x_dev)
    N, C, H, W = xr.shape
    Ho, Wo = gy.shape[2], gy.shape[3]
    wdv = w.to(DEV).contiguous(memory_format=CL)
    gr, ldg = as_rows(gy.to(DEV).contiguous(memory_format=CL))
    bd = None if bias is None else bias.to(DEV)
    geo = (N, H, W, C, Ho, Wo, C, 3, 3, stride, pad, dil, C)
    y = new_act(N, C, Ho, Wo, DEV)
    K.call(STEM + "_fwd_f32", xr, ldx, wdv, bd, y, C, *geo)
    dx = new_act(N, C, H, W, DEV)
    K.call(STEM + "_dgrad_f32", gr, ldg, wdv, dx, C, *geo)
    nbytes = int(K.query(STEM + "_wgrad_workspace_bytes", N, Ho, Wo, C, C, 3, 3, C))
    assert nbytes == 36 * C * B.wgrad_slabs(N * Ho * Wo, C)[1]
    wsb = _ws(nbytes, DEV)
    dws = []
    for _ in range(2):
        dw = torch.empty_like(wdv) if sink is None else sink.to(DEV).contiguous(memory_format=CL)
        K.call(STEM + "_wgrad_f32", gr, ldg, xr, ldx, dw, wsb, int(sink is not None), *geo)
        dws.append(dw)
    torch.cuda.synchronize()
    return dict(y=y, dx=dx, dw=dws[0], dw2=dws[1])


def _check(got, refs, tag):
    worst = B.worst(got, refs)
    print("dwconv", tag, {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)
    assert torch.equal(got["dw"], got["dw2"]), "the weight gradient must give the same bits twice"


@pytest.mark.parametrize("N,C,H,W,stride,dil", B.shape_list())
def test_depthwise_kernels_hold_the_fp32_bound(N, C, H, W, stride, dil):
    x, w, gy, pad = B.operands(C, H, W, stride, dil, N=N)
    refs = B.refs(x, w, gy, stride, pad, dil)
    got = _device_kernels(x.to(DEV).contiguous(memory_format=CL), w, gy, stride, pad, dil)
    _check(got, refs, (N, C, H, W, stride, dil))
    for name in ("y", "dx", "dw"):          # not vacuous: the outputs are there
        assert float(got[name].abs().max()) > 0


def test_channel_slice_of_a_wider_buffer():
    C, H, W, stride, dil = 132, 13, 11, 1, 2
    x, w, gy, pad = B.operands(C, H, W, stride, dil, seed=1)
    parent = torch.full((2, C + 24, H, W), 1e30).to(DEV).contiguous(memory_format=CL)       # poison beside the slice
    parent[:, 8:8 + C] = x.to(DEV)
    xs = parent[:, 8:8 + C]
    from u2pl_amd.layout import as_rows
    assert as_rows(xs)[1] == C + 24
    _check(_device_kernels(xs, w, gy, stride, pad, dil), B.refs(x, w, gy, stride, pad, dil), "slice")


def test_bias_and_accumulate_into_a_filled_sink():
    C, H, W, stride, dil = 132, 12, 10, 2, 2
    x, w, gy, pad = B.operands(C, H, W, stride, dil, seed=3)
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(C, generator=g)
    sink = torch.randn(w.shape, generator=g) * 1e-5
    got = _device_kernels(x.to(DEV).contiguous(memory_format=CL), w, gy, stride, pad, dil, bias=bias, sink=sink)
    _check(got, B.refs(x, w, gy, stride, pad, dil, bias=bias, sink=sink), "bias+accumulate")


def test_bad_arguments_raise_and_launch_nothing():
    from u2pl_amd import nn as K
    from u2pl_amd._lib import HipError
    from u2pl_amd.layout import _ws, new_act
    launches = lambda: int(K.query("u2pl_kernel_launches"))     # noqa: E731
    x = torch.randn(1, 8, 6, 6, device=DEV).contiguous(memory_format=CL)
    x6 = torch.randn(1, 6, 6, 6, device=DEV).contiguous(memory_format=CL)
    layers = [(K.Conv2d(8, 16, 3, padding=1, groups=8, bias=False), x, "depth multiplier"),
              (K.Conv2d(8, 8, 5, padding=2, groups=8, bias=False), x, "3x3"),
              (K.Conv2d(8, 8, 3, stride=3, padding=1, groups=8, bias=False), x, "stride"),
              (K.Conv2d(6, 6, 3, padding=1, groups=6, bias=False), x6, "multiple of 4")]
    layers = [(c.to(DEV), t, text) for c, t, text in layers]
    w = torch.randn(8, 1, 3, 3, device=DEV).contiguous(memory_format=CL)
    w5 = torch.randn(8, 1, 5, 5, device=DEV).contiguous(memory_format=CL)
    y = new_act(1, 8, 6, 6, DEV)
    ws = _ws(1 << 20, DEV)
    torch.cuda.synchronize()
    n0 = launches()
    for conv, t, text in layers:
        with pytest.raises(HipError, match="depthwise convolution: .*" + text):
            conv(t)
    # (Cin, Cout, R, S, stride, pad, dil, groups, Ho): depth multiplier, groups != C, C % 4, 5x5, stride 3, a wrong output size, dil 0
    bad = [(8, 16, 3, 3, 1, 1, 1, 8, 6), (8, 8, 3, 3, 1, 1, 1, 4, 6), (6, 6, 3, 3, 1, 1, 1, 6, 6), (8, 8, 5, 5, 1, 2, 1, 8, 6),
           (8, 8, 3, 3, 3, 1, 1, 8, 2), (8, 8, 3, 3, 1, 1, 1, 8, 5), (8, 8, 3, 3, 1, 0, 0, 8, 6)]
    for Cin, Cout, R, S, stride, pad, dil, groups, Ho in bad:
        wt = w5 if R == 5 else w
        geo = (1, 6, 6, Cin, Ho, Ho, Cout, R, S, stride, pad, dil, groups)
        with pytest.raises(HipError, match="1001"):
            K.call(STEM + "_fwd_f32", x, 8, wt, None, y, 8, *geo)
        with pytest.raises(HipError, match="1001"):
            K.call(STEM + "_dgrad_f32", y, 8, wt, x, 8, *geo)
        with pytest.raises(HipError, match="1001"):
            K.call(STEM + "_wgrad_f32", y, 8, x, 8, wt, ws, 0, *geo)
    good = (1, 6, 6, 8, 6, 6, 8, 3, 3, 1, 1, 1, 8)
    with pytest.raises(HipError, match="1001"):                     # ld % 4
        K.call(STEM + "_fwd_f32", x, 10, w, None, y, 8, *good)
    with pytest.raises(HipError, match="1001"):                     # ld < C
        K.call(STEM + "_fwd_f32", x, 4, w, None, y, 8, *good)
    with pytest.raises(HipError, match="1001"):                     # no workspace
        K.call(STEM + "_wgrad_f32", y, 8, x, 8, w, None, 0, *good)
    assert int(K.query(STEM + "_wgrad_workspace_bytes", 1, 6, 6, 8, 16, 3, 3, 8)) == 0
    assert launches() == n0
    K.call(STEM + "_fwd_f32", x, 8, w, None, y, 8, *good)           # ... and the good call does launch
    torch.cuda.synchronize()
    assert launches() == n0 + 1


# ---- through K.Conv2d -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W,stride,dil", [(132, 13, 11, 1, 2), (64, 12, 10, 2, 1)])
def test_conv2d_module_gives_the_bits_of_the_raw_calls(C, H, W, stride, dil):
    from u2pl_amd import nn as K
    x, w, gy, pad = B.operands(C, H, W, stride, dil, seed=4)
    bias = torch.randn(C, generator=torch.Generator().manual_seed(6))
    conv = K.Conv2d(C, C, 3, stride=stride, padding=pad, dilation=dil, groups=C, bias=True)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(bias)
    conv = conv.to(DEV)                                       # plain parameters: no arena, the gradients come back through autograd
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    with recorded_calls(K) as seen:
        y = conv(xd)
        y2, sums = conv(xd.detach(), stat_pivot=torch.zeros(C, device=DEV))
        y.backward(gy.to(DEV).contiguous(memory_format=CL))
        K.wgrad_stream_sync()
    torch.cuda.synchronize()
    assert sums is None and torch.equal(y2, y)                # BatchNorm statistics: by the stand-alone pass
    assert [len(seen.get(STEM + s, [])) for s in ("_fwd_f32", "_dgrad_f32", "_wgrad_f32")] == [2, 1, 1]
    assert not [n_ for n_ in seen if n_.startswith("u2pl_gconv2d")]
    raw = _device_kernels(x.to(DEV).contiguous(memory_format=CL), w, gy, stride, pad, dil, bias=bias)
    assert torch.equal(y.detach(), raw["y"])
    assert torch.equal(xd.grad, raw["dx"])
    assert torch.equal(conv.weight.grad, raw["dw"])
    assert float((conv.bias.grad.cpu().double() - gy.double().sum((0, 2, 3))).abs().max()) <= \
        (gy.shape[0] * gy.shape[2] * gy.shape[3] + 2) * EPS * float(gy.double().abs().sum((0, 2, 3)).max())


def test_grad_join_of_a_depthwise_and_a_pointwise_consumer():
    """x feeds a depthwise 3x3 and a dense 1x1 that share a GradJoin: x.grad is the fp32 sum of the two separate data gradients
    (one rounding: |got - (a + b)| <= 2^-24 |a + b|), whichever backward runs first"""
    from u2pl_amd import nn as K
    C, H, W = 64, 13, 11
    x, w, gy, pad = B.operands(C, H, W, 1, 2, seed=7)
    torch.manual_seed(8)
    dw = K.Conv2d(C, C, 3, padding=pad, dilation=2, groups=C, bias=False).to(DEV)
    pw = K.Conv2d(C, 32, 1, bias=False).to(DEV)
    ga = gy.to(DEV).contiguous(memory_format=CL)
    gb = torch.randn(2, 32, H, W).to(DEV).contiguous(memory_format=CL)
    xs = [x.to(DEV).contiguous(memory_format=CL).requires_grad_(True) for _ in range(4)]
    for order in (0, 1):
        xj = xs[order]
        join = K.grad_join(xj, 2)
        assert join is not None
        if order == 0:                                        # (autograd runs the later consumer's backward first)
            ya = dw(xj, grad_link=join)
            yb = pw(xj, grad_link=join)
        else:
            yb = pw(xj, grad_link=join)
            ya = dw(xj, grad_link=join)
        ((ya * ga).sum() + (yb * gb).sum()).backward()
    (dw(xs[2]) * ga).sum().backward()
    (pw(xs[3]) * gb).sum().backward()
    K.wgrad_stream_sync()
    torch.cuda.synchronize()
    a, b = xs[2].grad.cpu().double(), xs[3].grad.cpu().double()
    assert float(a.abs().max()) > 0 and float(b.abs().max()) > 0
    for order in (0, 1):
        got = xs[order].grad.cpu().double()
        assert bool(((got - (a + b)).abs() <= EPS * (a + b).abs()).all()), order


# ---- the separable decoder against its float64 twin --------------------------------------------------------------------------
def _seq64(seq, p, prefix, x, kept):
    """an nn.Sequential of the decoder in float64 from F.conv2d / F.batch_norm / relu (Dropout2d: p = 0 in these tests)"""
    from u2pl_amd import nn as K
    mods = list(seq)
    for i, m in enumerate(mods):
        name = "%s.%d" % (prefix, i)
        if isinstance(m, K.Conv2d):
            x = F.conv2d(x, p[name + ".weight"], p.get(name + ".bias"), stride=m.stride, padding=m.padding, dilation=m.dilation,
                         groups=m.groups)
            if m.bias is not None and i + 1 < len(mods) and isinstance(mods[i + 1], K.BatchNorm2d):
                x.retain_grad()
                kept[name + ".bias"] = x                      # its gradient: the terms of a bias gradient that is identically 0
        elif isinstance(m, K.BatchNorm2d):
            x = F.batch_norm(x, None, None, p[name + ".weight"], p[name + ".bias"], training=True, eps=m.eps)
        elif isinstance(m, torch.nn.ReLU):
            x = torch.relu(x)
        elif isinstance(m, torch.nn.AdaptiveAvgPool2d):
            x = x.mean((2, 3), keepdim=True)
        else:
            assert isinstance(m, torch.nn.Dropout2d) and m.p == 0, m
    return x


def _decoder_twin(dec, sd, x1, x4, G):
    p = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()
         and "running" not in k}
    x1 = x1.detach().cpu().double().clone().requires_grad_(True)
    x4 = x4.detach().cpu().double().clone().requires_grad_(True)
    kept = {}
    h, w = x4.shape[2:]
    a = dec.aspp
    pooled = F.interpolate(_seq64(a.conv1, p, "aspp.conv1", x4, kept), size=(h, w), mode="bilinear", align_corners=True)
    feats = [pooled] + [_seq64(getattr(a, n), p, "aspp." + n, x4, kept) for n in ("conv2", "conv3", "conv4", "conv5")]
    low = _seq64(dec.low_conv, p, "low_conv", x1, kept)
    up = F.interpolate(_seq64(dec.head, p, "head", torch.cat(feats, 1), kept), size=low.shape[2:], mode="bilinear",
                       align_corners=True)
    cat = torch.cat((low, up), 1)
    pred, rep = _seq64(dec.classifier, p, "classifier", cat, kept), _seq64(dec.representation, p, "representation", cat, kept)
    ((pred * G["pred"].double()).sum() + (rep * G["rep"].double()).sum()).backward()
    zero_bias_scale = {k: float(t.grad.abs().sum((0, 2, 3)).max()) for k, t in kept.items()}
    return dict(pred=pred.detach(), rep=rep.detach(), dx1=x1.grad, dx4=x4.grad, **{k: v.grad for k, v in p.items()}), zero_bias_scale


def _decoder_figures(separable, seed=0):
    from u2pl_amd import nn as K
    from u2pl_amd.models.decoder import dec_deeplabv3_plus
    torch.manual_seed(seed)
    dec = dec_deeplabv3_plus(in_planes=64, dilations=(1, 2, 12), separable=separable)
    for m in dec.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    with torch.no_grad():
        for n_, q in dec.named_parameters():
            if q.dim() == 1 and isinstance(dec.get_submodule(n_.rsplit(".", 1)[0]), K.BatchNorm2d):   # affine away from (1, 0)
                q.copy_(torch.rand(q.shape) + 0.5 if n_.endswith("weight") else torch.randn(q.shape) * 0.1)
    dec = dec.to(DEV).train()
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    x1 = torch.relu(torch.randn(4, 256, 17, 17, generator=g)).contiguous(memory_format=CL)
    x4 = torch.relu(torch.randn(4, 64, 9, 9, generator=g)).contiguous(memory_format=CL)
    G = dict(pred=torch.randn(4, 19, 17, 17, generator=g), rep=torch.randn(4, 256, 17, 17, generator=g))
    d1, d4 = x1.to(DEV).requires_grad_(True), x4.to(DEV).requires_grad_(True)
    out = dec([d1, None, None, d4])
    (sum((out[k] * G[k].to(DEV).contiguous(memory_format=CL)).sum() for k in ("pred", "rep"))).backward()
    K.wgrad_stream_sync()
    torch.cuda.synchronize()
    ref, zero_bias_scale = _decoder_twin(dec, sd, x1, x4, G)
    got = dict(pred=out["pred"], rep=out["rep"], dx1=d1.grad, dx4=d4.grad)
    for n_, q in dec.named_parameters():
        assert q.grad is not None, n_
        got[n_] = q.grad
    assert set(got) == set(ref)
    fig, shapes = {}, {}
    for k in got:
        err = float((got[k].detach().cpu().double() - ref[k]).abs().max())
        fig[k] = err / (zero_bias_scale[k] if k in zero_bias_scale else float(ref[k].abs().max()))
        shapes[k] = tuple(ref[k].shape)
    return fig, shapes, sorted(zero_bias_scale)


def test_separable_decoder_is_no_worse_than_the_dense_decoder():
    dense, dshape, dzero = _decoder_figures(False)
    sep, sshape, szero = _decoder_figures(True)
    # shared: what the option leaves alone (an index such as classifier.4 names a convolution in one model and a BatchNorm in the
    # other: the same name is not the same parameter there)
    shared = [k for k in dense if k in ("pred", "rep", "dx1", "dx4") or k.startswith(("low_conv.", "aspp.conv1.", "aspp.conv2."))]
    assert all(k in sep and dshape[k] == sshape[k] for k in shared)
    top = max(dense.values())
    print("decoder figures (max|got - ref| / max|ref|); largest dense figure %.3e" % top)
    for k in sorted(dense):
        print("   %-36s %-18s dense %.3e" % (k, dshape[k], dense[k]))
    for k in sorted(sep):
        print("   %-36s %-18s separable %.3e   dense %s" % (k, sshape[k], sep[k], "%.3e" % dense[k] if k in shared else "-"))
    print("   biases in front of a train-mode BatchNorm (denominator: sum |dy|): dense %s, separable %s" % (dzero, szero))
    assert {"pred", "rep", "dx1", "dx4", "low_conv.0.weight", "aspp.conv1.1.weight", "aspp.conv2.0.weight"} <= set(shared)
    assert len(sep) > len(dense) and all(np.isfinite(v) for v in sep.values())
    bad = {k: (sep[k], dense[k]) for k in shared if not sep[k] <= 2 * dense[k]}
    bad.update({k: (sep[k], top) for k in sep if k not in shared and not sep[k] <= 2 * top})
    assert not bad, bad


# ---- the whole path -----------------------------------------------------------------------------------------------------------
def _sep_cfg():
    cfg = decoder_cfg()
    cfg["decoder"]["kwargs"]["separable"] = True
    return cfg


@pytest.fixture(scope="module")
def sepnet():
    return build_net(_sep_cfg()), net_input()


def test_separable_train_step_reaches_every_parameter(sepnet):
    from u2pl_amd import nn as K
    model, x = sepnet
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    seen, _ = step_calls(model, x)
    n_dw = sum(1 for m in model.modules() if isinstance(m, K.Conv2d) and m.groups != 1)
    assert n_dw == 8
    for name in (STEM + "_fwd_f32", STEM + "_dgrad_f32", STEM + "_wgrad_f32"):
        assert len(seen.get(name, [])) == n_dw, (name, len(seen.get(name, [])))
    assert not [n_ for n_ in seen if n_.startswith("u2pl_gconv2d")]
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


def test_separable_eval_forward_is_the_same_with_and_without_a_graph(sepnet):
    model, x = sepnet
    model.eval()
    try:
        with torch.no_grad():
            a = model(x)["pred"].clone()          # the teacher's path
        b = model(x)["pred"]                      # records an autograd graph
        assert b.requires_grad
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b.detach())
    finally:
        model.train()


def test_separable_state_dict_round_trip_and_a_dense_checkpoint_is_refused(sepnet):
    from u2pl_amd.models.model_helper import ModelBuilder
    model, x = sepnet
    fresh = build_net(_sep_cfg(), seed=99)
    fresh.load_state_dict(model.state_dict())
    model.eval(), fresh.eval()
    try:
        with torch.no_grad():
            a, b = model(x), fresh(x)
        for k in ("pred", "rep"):
            assert torch.equal(a[k], b[k]), k
    finally:
        model.train()
    dense = ModelBuilder(net_cfg("resnet50", 19, True))
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key|size mismatch"):
        fresh.load_state_dict(dense.state_dict())


def test_default_decoder_makes_no_depthwise_call_and_the_calls_of_a_model_built_without_the_keyword():
    counts = []
    for kw in ({}, dict(separable=False)):
        cfg = net_cfg("resnet50", 19, True)
        cfg["decoder"]["kwargs"].update(kw)
        seen, _ = step_calls(build_net(cfg).train(), net_input(2, 3))
        assert len(seen) > 10
        assert not [n_ for n_ in seen if n_.startswith(STEM) or n_.startswith("u2pl_gconv2d")]
        counts.append({k: len(v) for k, v in seen.items()})
    assert counts[0] == counts[1]


def test_separable_graph_replay_is_bit_identical_to_eager(monkeypatch):
    a, b = (train_steps(monkeypatch, on, lambda cfg: cfg["net"]["decoder"]["kwargs"].update(separable=True)) for on in (True, False))
    print("graph stats", a["stats"])
    assert_replay_equals_eager(a, b)
