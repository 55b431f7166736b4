"""-m gpu: grouped convolutions (csrc/gconv.hip, nn._GroupedConvFn) -- the 3x3 of a ResNeXt bottleneck.

Kernels against float64.  Oracle: torch.nn.functional.conv2d(groups=g) (and torch.nn.grad's input / weight gradients) in float64
on the CPU, on the float32-rounded operands.  Bound of each output element:

    |got - ref| <= (n + 2) * 2^-24 * cond

cond: the same grouped convolution (or gradient) on absolute values (plus |bias| / |sink| where an epilogue adds one), n: the
reduction length (R*S*Cin/groups for y and dx, N*Ho*Wo for dw).  This is the worst case of an fp32 sum of n products in any
order (n roundings of partial sums that never exceed cond) plus the bias / accumulate add: derived, not fitted.  The weight
gradient's slab partial sums fit it too: a term passes through at most (pixels per slab + slabs) <= n additions.

A block against its float64 twin: Bottleneck(256, 64, groups=32, base_width=4) in train mode against the same block written
from F.conv2d / F.batch_norm / relu in float64; yardstick: the same test on the dense Bottleneck(256, 64); each grouped figure
(max|got - ref| / max|ref| of the output, the input gradient and every parameter gradient) must be <= 2x the dense block's.

The whole path: ResNeXt-50 32x4d + DeepLabv3+ through ModelBuilder at 65 x 65."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from model_utils import net_cfg
from split_bounds import EPS, excess, recorded_calls

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last

WIDTHS = [(32, 4), (32, 8), (8, 16), (4, 32), (2, 64), (3, 12)]                  # (groups, channels per group); last: generic width
GEOMS = [(13, 11, 1, 1), (9, 17, 2, 1), (13, 11, 1, 2), (9, 17, 1, 4), (12, 10, 2, 2)]      # (H, W, stride, dil)


def _out(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _operands(groups, cg, H, W, stride, dil, k=3, seed=0, N=2):
    """post-ReLU heavy-tailed x, weights N(0,1)/sqrt(9 cg), a gradient whose pixels span six decades (all float32, CPU)"""
    g = torch.Generator().manual_seed(1000 * seed + 17 * groups + cg)
    C = groups * cg
    pad = dil * (k // 2)
    x = torch.relu(torch.randn(N, C, H, W, generator=g) - 0.25) ** 3
    w = torch.randn(C, cg, k, k, generator=g) / math.sqrt(9 * cg)
    Ho, Wo = _out(H, k, stride, pad, dil), _out(W, k, stride, pad, dil)
    gy = torch.randn(N, C, Ho, Wo, generator=g) * 1e-4 * 10.0 ** (-6 * torch.rand(N, 1, Ho, Wo, generator=g))
    return x, w, gy, pad


def _refs(x, w, gy, stride, pad, dil, groups, bias=None, sink=None):
    """float64 (ref, bound) of y, dx, dw"""
    xd, wd, gd = x.double(), w.double(), gy.double()
    kw = dict(stride=stride, padding=pad, dilation=dil, groups=groups)
    cg, R, S = w.shape[1], w.shape[2], w.shape[3]
    n_k, n_px = R * S * cg, gy.shape[0] * gy.shape[2] * gy.shape[3]

    def three(a, b, c):
        return (F.conv2d(a, b, **kw), torch.nn.grad.conv2d_input(tuple(x.shape), b, c, **kw),
                torch.nn.grad.conv2d_weight(a, tuple(w.shape), c, **kw))
    ref, cond = list(three(xd, wd, gd)), list(three(xd.abs(), wd.abs(), gd.abs()))
    if bias is not None:
        ref[0] = ref[0] + bias.double().view(1, -1, 1, 1)
        cond[0] = cond[0] + bias.double().abs().view(1, -1, 1, 1)
    if sink is not None:
        ref[2] = ref[2] + sink.double()
        cond[2] = cond[2] + sink.double().abs()
    ns = (n_k, n_k, n_px)
    return {name: (r, (n + 2) * EPS * c) for name, r, c, n in zip(("y", "dx", "dw"), ref, cond, ns)}


def _device_kernels(x_dev, w, gy, stride, pad, dil, groups, bias=None, sink=None):
    """the three C entry points on device tensors; x_dev may be a channel slice of a wider channels_last buffer"""
    from u2pl_amd import nn as K
    from u2pl_amd.layout import _ws, as_rows, new_act
    xr, ldx = as_rows(x_dev)
    N, C, H, W = xr.shape
    Cout, _, R, S = w.shape
    Ho, Wo = gy.shape[2], gy.shape[3]
    wdv = w.to(DEV).contiguous(memory_format=CL)
    gr, ldg = as_rows(gy.to(DEV).contiguous(memory_format=CL))
    bd = None if bias is None else bias.to(DEV)
    y = new_act(N, Cout, Ho, Wo, DEV)
    K.call("u2pl_gconv2d_fwd_f32", xr, ldx, wdv, bd, y, Cout, N, H, W, C, Ho, Wo, Cout, R, S, stride, pad, dil, groups)
    dx = new_act(N, C, H, W, DEV)
    K.call("u2pl_gconv2d_dgrad_f32", gr, ldg, wdv, dx, C, N, H, W, C, Ho, Wo, Cout, R, S, stride, pad, dil, groups)
    wsb = _ws(K.query("u2pl_gconv2d_wgrad_workspace_bytes", N, Ho, Wo, C, Cout, R, S, groups), DEV)
    dws = []
    for _ in range(2):
        dw = torch.empty_like(wdv) if sink is None else sink.to(DEV).contiguous(memory_format=CL)
        K.call("u2pl_gconv2d_wgrad_f32", gr, ldg, xr, ldx, dw, wsb, int(sink is not None), N, H, W, C, Ho, Wo, Cout, R, S, stride,
               pad, dil, groups)
        dws.append(dw)
    torch.cuda.synchronize()
    return dict(y=y, dx=dx, dw=dws[0], dw2=dws[1])


def _check(got, refs, tag):
    worst = {}
    for name in ("y", "dx", "dw"):
        ref, bound = refs[name]
        assert tuple(got[name].shape) == tuple(ref.shape)
        worst[name] = excess(got[name], ref, bound)
    print("gconv", tag, {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)
    assert torch.equal(got["dw"], got["dw2"]), "the weight gradient must give the same bits twice"


@pytest.mark.parametrize("H,W,stride,dil", GEOMS)
@pytest.mark.parametrize("groups,cg", WIDTHS)
def test_grouped_kernels_hold_the_fp32_bound(groups, cg, H, W, stride, dil):
    x, w, gy, pad = _operands(groups, cg, H, W, stride, dil)
    refs = _refs(x, w, gy, stride, pad, dil, groups)
    got = _device_kernels(x.to(DEV).contiguous(memory_format=CL), w, gy, stride, pad, dil, groups)
    _check(got, refs, (groups, cg, H, W, stride, dil))
    for name in ("y", "dx", "dw"):          # not vacuous: the outputs are there
        assert float(got[name].abs().max()) > 0


def test_channel_slice_of_a_wider_buffer():
    groups, cg, H, W, stride, dil = 8, 16, 13, 11, 1, 2
    x, w, gy, pad = _operands(groups, cg, H, W, stride, dil, seed=1)
    C = groups * cg
    parent = torch.full((2, C + 24, H, W), 1e30).to(DEV).contiguous(memory_format=CL)       # poison beside the slice
    parent[:, 8:8 + C] = x.to(DEV)
    xs = parent[:, 8:8 + C]
    from u2pl_amd.layout import as_rows
    assert as_rows(xs)[1] == C + 24
    _check(_device_kernels(xs, w, gy, stride, pad, dil, groups), _refs(x, w, gy, stride, pad, dil, groups), "slice")


def test_pointwise_grouped_kernel():
    groups, cg, H, W, stride, dil = 4, 32, 9, 17, 2, 1
    x, w, gy, pad = _operands(groups, cg, H, W, stride, dil, k=1, seed=2)
    assert pad == 0 and w.shape[2:] == (1, 1)
    _check(_device_kernels(x.to(DEV).contiguous(memory_format=CL), w, gy, stride, pad, dil, groups),
           _refs(x, w, gy, stride, pad, dil, groups), "1x1")


def test_bias_and_accumulate_into_a_filled_sink():
    groups, cg, H, W, stride, dil = 32, 4, 12, 10, 2, 2
    x, w, gy, pad = _operands(groups, cg, H, W, stride, dil, seed=3)
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(groups * cg, generator=g)
    sink = torch.randn(w.shape, generator=g) * 1e-5
    got = _device_kernels(x.to(DEV).contiguous(memory_format=CL), w, gy, stride, pad, dil, groups, bias=bias, sink=sink)
    _check(got, _refs(x, w, gy, stride, pad, dil, groups, bias=bias, sink=sink), "bias+accumulate")


def test_bad_arguments_raise_and_launch_nothing():
    from u2pl_amd import nn as K
    from u2pl_amd._lib import HipError
    from u2pl_amd.layout import _ws, new_act
    launches = lambda: int(K.query("u2pl_kernel_launches"))     # noqa: E731
    x = torch.randn(1, 24, 6, 6, device=DEV).contiguous(memory_format=CL)
    conv = K.Conv2d(24, 24, 3, padding=1, groups=4, bias=False).to(DEV)            # 6 channels per group
    torch.cuda.synchronize()
    n0 = launches()
    with pytest.raises(HipError, match="multiple of 4"):
        conv(x)
    w = torch.randn(24, 8, 3, 3, device=DEV).contiguous(memory_format=CL)
    y = new_act(1, 24, 6, 6, DEV)
    for groups in (5, 4):                                           # Cin % groups; 6 channels per group
        with pytest.raises(HipError, match="1001"):
            K.call("u2pl_gconv2d_fwd_f32", x, 24, w, None, y, 24, 1, 6, 6, 24, 6, 6, 24, 3, 3, 1, 1, 1, groups)
        with pytest.raises(HipError, match="1001"):
            K.call("u2pl_gconv2d_dgrad_f32", y, 24, w, x, 24, 1, 6, 6, 24, 6, 6, 24, 3, 3, 1, 1, 1, groups)
        with pytest.raises(HipError, match="1001"):
            K.call("u2pl_gconv2d_wgrad_f32", y, 24, x, 24, w, _ws(1 << 20, DEV), 0, 1, 6, 6, 24, 6, 6, 24, 3, 3, 1, 1, 1, groups)
    with pytest.raises(HipError, match="1001"):                     # stride 3
        K.call("u2pl_gconv2d_fwd_f32", x, 24, w, None, y, 24, 1, 6, 6, 24, 2, 2, 24, 3, 3, 3, 1, 1, 3)
    assert launches() == n0


# ---- a block against its float64 twin ----------------------------------------------------------------------------------------
def _twin(sd, names, x, G, stride, dil, groups, has_ds):
    p = {k: sd[k].detach().cpu().double().clone().requires_grad_(True) for k in names}
    x = x.detach().cpu().double().clone().requires_grad_(True)

    def bn(t, pre):
        return F.batch_norm(t, None, None, p[pre + ".weight"], p[pre + ".bias"], training=True, eps=1e-5)
    o = torch.relu(bn(F.conv2d(x, p["conv1.weight"]), "bn1"))
    o = torch.relu(bn(F.conv2d(o, p["conv2.weight"], stride=stride, padding=dil, dilation=dil, groups=groups), "bn2"))
    o = bn(F.conv2d(o, p["conv3.weight"]), "bn3")
    idt = bn(F.conv2d(x, p["downsample.0.weight"], stride=stride), "downsample.1") if has_ds else x
    out = torch.relu(o + idt)
    (out * G.double()).sum().backward()
    return out.detach(), x.grad, {k: v.grad for k, v in p.items()}


def _block_figures(groups, base_width, stride, dil, seed):
    from u2pl_amd import nn as K
    from u2pl_amd.models.resnet import Bottleneck, conv1x1
    torch.manual_seed(seed)
    ds = None
    if stride != 1:
        ds = torch.nn.Sequential(conv1x1(256, 256, stride), K.BatchNorm2d(256))
    blk = Bottleneck(256, 64, stride=stride, downsample=ds, groups=groups, base_width=base_width, dilation=dil)
    with torch.no_grad():
        for n_, q in blk.named_parameters():
            if q.dim() == 1:                # BatchNorm affine parameters away from (1, 0)
                q.copy_(torch.rand(q.shape) + 0.5 if n_.endswith("weight") else torch.randn(q.shape) * 0.1)
    blk = blk.to(DEV).train()
    names = [n_ for n_, _ in blk.named_parameters()]
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    x = torch.relu(torch.randn(2, 256, 17, 15)).contiguous(memory_format=CL)
    Ho, Wo = _out(17, 3, stride, dil, dil), _out(15, 3, stride, dil, dil)
    G = torch.randn(2, 256, Ho, Wo)
    xd = x.to(DEV).requires_grad_(True)
    out = blk(xd)
    (out * G.to(DEV).contiguous(memory_format=CL)).sum().backward()
    K.wgrad_stream_sync()
    torch.cuda.synchronize()
    ref_out, ref_dx, ref_g = _twin(sd, names, x, G, stride, dil, groups, ds is not None)

    def rel(got, ref):
        return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())
    fig = {"out": rel(out, ref_out), "dx": rel(xd.grad, ref_dx)}
    for n_, q in blk.named_parameters():
        assert q.grad is not None, n_
        fig[n_] = rel(q.grad, ref_g[n_])
    return fig


@pytest.mark.parametrize("stride,dil", [(1, 1), (2, 1), (1, 2)])
def test_resnext_block_is_no_worse_than_the_dense_block(stride, dil):
    dense = _block_figures(1, 64, stride, dil, seed=0)
    grouped = _block_figures(32, 4, stride, dil, seed=0)
    print("block stride %d dil %d" % (stride, dil))
    for k in dense:
        print("   %-24s dense %.3e   grouped %.3e" % (k, dense[k], grouped[k]))
    assert set(dense) == set(grouped)
    bad = {k: (grouped[k], dense[k]) for k in dense if not grouped[k] <= 2 * dense[k]}
    assert not bad, bad


# ---- the whole path -----------------------------------------------------------------------------------------------------------
S_NET = 65


def _resnext_cfg(zero_init=False):
    cfg = net_cfg("resnet50", 19, True)
    cfg["encoder"]["kwargs"].update(groups=32, width_per_group=4, zero_init_residual=zero_init)
    return cfg


@pytest.fixture(scope="module")
def resnext():
    from u2pl_amd.models.model_helper import ModelBuilder
    torch.manual_seed(0)
    model = ModelBuilder(_resnext_cfg()).to(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 3, S_NET, S_NET, generator=g).to(DEV)
    return model, x


def test_resnext_train_step_reaches_every_parameter(resnext):
    from u2pl_amd import nn as K
    model, x = resnext
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    with recorded_calls(K) as seen:
        outs = model(x)
        g = torch.Generator().manual_seed(2)
        loss = sum((outs[k] * torch.randn(outs[k].shape, generator=g).to(DEV)).sum() for k in ("pred", "rep", "aux"))
        loss.backward()
        K.wgrad_stream_sync()
    torch.cuda.synchronize()
    n_g = sum(1 for m in model.modules() if isinstance(m, K.Conv2d) and m.groups != 1)
    assert n_g == 16
    for name in ("u2pl_gconv2d_fwd_f32", "u2pl_gconv2d_dgrad_f32", "u2pl_gconv2d_wgrad_f32"):
        assert len(seen.get(name, [])) == n_g, (name, len(seen.get(name, [])))
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


def test_resnext_eval_forward_is_the_same_with_and_without_a_graph(resnext):
    model, x = resnext
    model.eval()
    try:
        with torch.no_grad():
            a = model(x)["pred"].clone()          # the teacher's path
        b = model(x)["pred"]                      # records an autograd graph: the unfused conv -> BatchNorm launches
        assert b.requires_grad
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b.detach())
    finally:
        model.train()


def test_resnext_state_dict_round_trip_gives_the_same_forward(resnext):
    from u2pl_amd.models.model_helper import ModelBuilder
    model, x = resnext
    torch.manual_seed(99)
    fresh = ModelBuilder(_resnext_cfg()).to(DEV)
    fresh.load_state_dict(model.state_dict())
    model.eval(), fresh.eval()
    try:
        with torch.no_grad():
            a, b = model(x), fresh(x)
        for k in ("pred", "rep"):
            assert torch.equal(a[k], b[k]), k
    finally:
        model.train()


def test_dense_resnet50_step_makes_no_grouped_call():
    from u2pl_amd import nn as K
    from u2pl_amd.models.model_helper import ModelBuilder
    torch.manual_seed(0)
    model = ModelBuilder(net_cfg("resnet50", 19, True)).to(DEV).train()
    x = torch.randn(2, 3, S_NET, S_NET, device=DEV)
    with recorded_calls(K) as seen:
        outs = model(x)
        (outs["pred"].sum() + outs["aux"].sum() + outs["rep"].sum()).backward()
        K.wgrad_stream_sync()
    torch.cuda.synchronize()
    assert len(seen) > 10
    assert not [n_ for n_ in seen if n_.startswith("u2pl_gconv2d")]


def _train(monkeypatch, graphs_on, steps=4, S=S_NET):
    """tests/test_gpu_graphs.py::_run with a ResNeXt-50 32x4d encoder"""
    from u2pl_amd import configs, graphs as G
    from u2pl_amd.models.model_helper import ModelBuilder
    from u2pl_amd.trainer import SemiTrainer
    from u2pl_amd.utils.loss_helper import get_criterion

    monkeypatch.setenv("U2PL_GRAPHS", "1" if graphs_on else "0")
    cfg = configs.cityscapes_semi(arch="resnet50", crop=S, batch_size=2, sync_bn=False, epochs=20)
    cfg["net"]["encoder"]["kwargs"].update(groups=32, width_per_group=4)
    cfg["criterion"]["kwargs"]["min_kept"] = 1500
    cfg["trainer"]["contrastive"]["current_class_threshold"] = 0.055
    torch.manual_seed(0)
    model, teacher = ModelBuilder(copy.deepcopy(cfg["net"])), ModelBuilder(copy.deepcopy(cfg["net"]))
    teacher.load_state_dict(model.state_dict())
    model, teacher = model.to(DEV), teacher.to(DEV)
    tr = SemiTrainer(cfg, model, teacher, get_criterion(cfg), steps_per_epoch=4)
    g = torch.Generator().manual_seed(5)
    stats0 = dict(G.STATS)
    meters = []
    for step in range(steps):
        il, iu = torch.randn(2, 3, S, S, generator=g), torch.randn(2, 3, S, S, generator=g)
        ll = torch.randint(0, 19, (2, S, S), generator=g)
        ll[:, :6] = 255
        np.random.seed(30 + step)
        torch.manual_seed(40 + step)
        torch.cuda.manual_seed(50 + step)
        meters.append(tr.train_step(il.to(DEV), ll.to(DEV), iu.to(DEV), epoch=step // 4).cpu().numpy())
    torch.cuda.synchronize()
    return dict(meters=np.stack(meters), w=tr.arena.flat.clone(), t=tr.t_arena.flat.clone(),
                stats={k: G.STATS[k] - stats0[k] for k in stats0})


def test_resnext_graph_replay_is_bit_identical_to_eager(monkeypatch):
    a = _train(monkeypatch, True)
    b = _train(monkeypatch, False)
    print("graph stats", a["stats"])
    assert a["stats"]["replays"] > 0 and a["stats"]["aborted"] == 0 and b["stats"]["replays"] == 0
    assert np.isfinite(a["meters"]).all()
    assert np.array_equal(a["meters"], b["meters"]), (a["meters"], b["meters"])
    assert torch.equal(a["w"], b["w"]) and torch.equal(a["t"], b["t"])
