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

The whole path: ResNeXt-50 32x4d + DeepLabv3+ through ModelBuilder at 65 x 65.

Every width, tap and pixel edge (the second half of this file): the table of tests/gconv_bounds.py -- Cin/groups != Cout/groups, three
column tiles, partial last tiles, filters other than 3x3 and 1x1, Wout < 4, 5 to 34816 pixels -- through the three C entry points with
the same oracle and bound (n = R*S*Cin/groups for y, R*S*Cout/groups for dx, N*Ho*Wo for dw).  x, dy, y and dx are channel slices
of wider buffers: NaN beside the inputs, a sentinel around the outputs (the columns outside the slice, two rows in front, three rows
past M, the tail of dw) and behind the workspace, which is allocated at exactly the queried size and filled with NaN.
tests/test_gconv_cpu.py shows on an emulation that this bound on this table rejects seven one-line addressing mistakes that the
table above cannot see.  Each case prints its excess (pytest -s); U2PL_GCONV_RECORD=path writes the largest |got - f64| / bound per
entry point and kernel family as JSON (profiles/gconv_bounds.json is one such run: a record, not a threshold)."""
import functools
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

import gconv_bounds as B
from decoder_harness import CL, DEV, S_NET, assert_replay_equals_eager, build_net, decoder_cfg, net_input, step_calls, train_steps
from model_utils import net_cfg
from split_bounds import EPS, conv_dx_bound, excess, recorded_calls

pytestmark = pytest.mark.gpu

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
def _resnext_cfg():
    cfg = decoder_cfg()
    cfg["encoder"]["kwargs"].update(groups=32, width_per_group=4)
    return cfg


@pytest.fixture(scope="module")
def resnext():
    return build_net(_resnext_cfg()), net_input()


def test_resnext_train_step_reaches_every_parameter(resnext):
    from u2pl_amd import nn as K
    model, x = resnext
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    seen, _ = step_calls(model, x)
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
    model, x = resnext
    fresh = build_net(_resnext_cfg(), seed=99)
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


def test_resnext_graph_replay_is_bit_identical_to_eager(monkeypatch):
    a, b = (train_steps(monkeypatch, on, lambda cfg: cfg["net"]["encoder"]["kwargs"].update(groups=32, width_per_group=4))
            for on in (True, False))
    print("graph stats", a["stats"])
    assert_replay_equals_eager(a, b)


# ---- every width, tap and pixel edge: the table of tests/gconv_bounds.py in sentinel frames -------------------------------------
SENT = -7.25e22
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _records():
    yield
    for key in sorted(WORST):
        print("worst  %-40s %.4f" % (key, WORST[key]))
    path = os.environ.get("U2PL_GCONV_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump({k: round(v, 4) for k, v in sorted(WORST.items())}, f, indent=1)
            f.write("\n")


class Frame:
    """a [M][C] row tensor as a channel slice of a wider buffer: rows [front + M + back][C + extra] filled with `fill`, the slice
    at column `off`.  ptr: what an entry point is handed; rows(): the slice; intact(): the frame has kept its bits"""

    def __init__(self, M, C, extra, off, fill, front=2, back=3):
        assert extra % 4 == 0 and off % 4 == 0 and off <= extra
        self.M, self.C, self.ld = M, C, C + extra
        self.start = front * self.ld + off
        self.buf = torch.full(((front + M + back) * self.ld,), fill, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf[self.start:]
        self.before = None

    def rows(self):
        return torch.as_strided(self.buf, (self.M, self.C), (self.ld, 1), self.start)

    def arm(self):
        self.before = self.buf.clone()
        return self

    def intact(self):
        now = self.buf.clone()
        self.rows().copy_(torch.as_strided(self.before, (self.M, self.C), (self.ld, 1), self.start))    # the slice put back: the rest is the frame
        same = torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))
        self.buf.copy_(now)
        return same


def _to_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).to(DEV)


def _from_rows(rows, N, H, W):
    return rows.reshape(N, H, W, rows.shape[1]).permute(0, 3, 1, 2).cpu()


def run_case(case, x, w, gy, bias=None, sink=None):
    """the three C entry points on one case, every tensor in its frame -> y, dx, dw, dw2 (CPU, logical shapes)"""
    from u2pl_amd import nn as K
    groups, cig, cog, R, S, H, W, stride, pad, dil, N = case
    Cin, Cout = groups * cig, groups * cog
    Ho, Wo = B.out_hw(case)
    My, Mx = N * Ho * Wo, N * H * W
    nan = float("nan")
    xf, gf = Frame(Mx, Cin, 24, 8, nan), Frame(My, Cout, 40, 12, nan)                   # NaN beside and behind the inputs
    xf.rows().copy_(_to_rows(x))
    gf.rows().copy_(_to_rows(gy))
    yf, dxf = Frame(My, Cout, 12, 4, SENT).arm(), Frame(Mx, Cin, 20, 16, SENT).arm()
    E = Cout * R * S * cig
    wdv = w.permute(0, 2, 3, 1).contiguous().reshape(-1).to(DEV)                        # [Cout][R][S][cig]
    bd = None if bias is None else bias.to(DEV)
    geo = (N, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil, groups)
    K.call("u2pl_gconv2d_fwd_f32", xf.ptr, xf.ld, wdv, bd, yf.ptr, yf.ld, *geo)
    K.call("u2pl_gconv2d_dgrad_f32", gf.ptr, gf.ld, wdv, dxf.ptr, dxf.ld, *geo)
    nbytes = int(K.query("u2pl_gconv2d_wgrad_workspace_bytes", N, Ho, Wo, Cin, Cout, R, S, groups))
    assert nbytes == B.workspace_bytes(case) and nbytes % 16 == 0
    ws = torch.full((nbytes // 4 + 64,), nan, device=DEV)                               # exactly the queried size, then a sentinel tail
    ws[nbytes // 4:] = SENT
    dws = []
    for _ in range(2):
        dw = torch.full((E + 64,), SENT, device=DEV)
        if sink is not None:
            dw[:E] = sink.permute(0, 2, 3, 1).reshape(-1).to(DEV)
        K.call("u2pl_gconv2d_wgrad_f32", gf.ptr, gf.ld, xf.ptr, xf.ld, dw, ws, int(sink is not None), *geo)
        dws.append(dw)
    torch.cuda.synchronize()
    assert yf.intact(), "the forward wrote outside y"
    assert dxf.intact(), "the data gradient wrote outside dx"
    assert bool((ws[nbytes // 4:] == SENT).all()), "the weight gradient wrote past the queried workspace"
    assert all(bool((d[E:] == SENT).all()) for d in dws), "the weight gradient wrote past dw"
    dw, dw2 = (d[:E].reshape(Cout, R, S, cig).permute(0, 3, 1, 2).cpu() for d in dws)
    return dict(y=_from_rows(yf.rows(), N, Ho, Wo), dx=_from_rows(dxf.rows(), N, H, W), dw=dw, dw2=dw2)


def family(case):
    """entry point and kernel template per output"""
    return dict(y="fwd k_gconv<%d, false>" % B.col_tiles(case[2]), dx="dgrad k_gconv<%d, true>" % B.col_tiles(case[1]),
                dw="wgrad k_gconv_wgrad<%d>" % B.wgrad_family(case[3] * case[4]))


def held(case, got, refs, tag):
    worst = B.worst(got, refs)
    print("gconv", tag, {k: round(v, 4) for k, v in worst.items()})
    for name, key in family(case).items():
        WORST[key] = max(WORST.get(key, 0.0), worst[name])
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)
    assert torch.equal(got["dw"].view(torch.int32), got["dw2"].view(torch.int32)), "the weight gradient must give the same bits twice"
    for name in B.NAMES:                    # a bound of 0 (only padding is met, no bias, no sink): exactly 0
        ref, bound = refs[name]
        assert bool((got[name][bound == 0] == 0).all()), (tag, name)


@functools.lru_cache(maxsize=None)
def _case_data(case):
    """operands and float64 references of one case: computed once, shared, not modified"""
    ops = B.operands(case)
    return ops, B.refs(case, *ops)


TABLE = B.shape_list()


@pytest.mark.parametrize("case", TABLE, ids=[B.case_id(c) for c in TABLE])
def test_whole_table_in_sentinel_frames(case):
    (x, w, gy), refs = _case_data(case)
    got = run_case(case, x, w, gy)
    held(case, got, refs, B.case_id(case))
    for name in B.NAMES:                    # not vacuous: the outputs are there
        assert float(got[name].abs().max()) > 0


def test_bias_and_accumulate_on_a_5x5_with_unequal_widths():
    """bias in the forward's epilogue; the weight gradient added into a sink as large as dw itself"""
    case = (8, 4, 12, 5, 5, 13, 11, 1, 2, 1, 2)
    assert case in TABLE
    (x, w, gy), plain = _case_data(case)
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(case[0] * case[2], generator=g)
    sink = (torch.randn(w.shape, generator=g) * plain["dw"][0].abs().mean()).float()
    got = run_case(case, x, w, gy, bias=bias, sink=sink)
    held(case, got, B.refs(case, x, w, gy, bias=bias, sink=sink), "bias+accumulate " + B.case_id(case))
    assert not torch.equal(got["dw"], sink)


FUNCTION_LAYERS = [dict(in_channels=32, out_channels=64, kernel_size=5, padding=4, dilation=2, stride=2, groups=4, bias=True),
                   dict(in_channels=80, out_channels=96, kernel_size=3, padding=1, groups=2, bias=True)]


@pytest.mark.parametrize("kw", FUNCTION_LAYERS, ids=["5x5-s2-d2-8to16", "3x3-40to48"])
def test_conv2d_function_gives_the_bits_of_the_raw_calls(kw):
    from u2pl_amd import nn as K
    conv = K.Conv2d(**kw)
    groups, k = conv.groups, kw["kernel_size"]
    case = (groups, conv.in_channels // groups, conv.out_channels // groups, k, k, 13, 11, conv.stride, conv.padding, conv.dilation, 2)
    assert case[1] != case[2] and K.gconv_constraint(conv.in_channels, conv.out_channels, groups, conv.stride) is None
    x, w, gy = B.operands(case, seed=4)
    bias = torch.randn(conv.out_channels, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(bias)
    conv = conv.to(DEV)                                       # plain parameters: no arena, the gradients come back through autograd
    xd = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
    with recorded_calls(K) as seen:
        y = conv(xd)
        y.backward(gy.to(DEV).contiguous(memory_format=CL))
        K.wgrad_stream_sync()
    torch.cuda.synchronize()
    assert [len(seen.get("u2pl_gconv2d" + s, [])) for s in ("_fwd_f32", "_dgrad_f32", "_wgrad_f32")] == [1, 1, 1]
    assert not [n_ for n_ in seen if n_.startswith("u2pl_dwconv2d") or n_.startswith("u2pl_conv2d")]
    raw = run_case(case, x, w, gy, bias=bias)
    held(case, raw, B.refs(case, x, w, gy, bias=bias), "function " + B.case_id(case))
    for got, name in ((y.detach(), "y"), (xd.grad, "dx"), (conv.weight.grad, "dw")):
        assert torch.equal(got.cpu().view(torch.int32), raw[name].contiguous().view(torch.int32)), name
    assert float((conv.bias.grad.cpu().double() - gy.double().sum((0, 2, 3))).abs().max()) <= \
        (gy.shape[0] * gy.shape[2] * gy.shape[3] + 2) * EPS * float(gy.double().abs().sum((0, 2, 3)).max())


def test_grad_join_of_a_grouped_and_a_dense_consumer():
    """x feeds a grouped 3x3 (8 -> 16 channels per group) and a dense 1x1 that share a GradJoin: x.grad is the sum of the two data
    gradients, each within its own bound (the grouped one's above, the dense one's of tests/split_bounds.py), plus the one fp32
    rounding of the sum -- whichever backward runs first"""
    from u2pl_amd import nn as K
    case = (4, 8, 16, 3, 3, 13, 11, 1, 1, 1, 2)
    x, w, gy = B.operands(case, seed=7)
    torch.manual_seed(8)
    gc = K.Conv2d(32, 64, 3, padding=1, groups=4, bias=False)
    with torch.no_grad():
        gc.weight.copy_(w)
    gc = gc.to(DEV)
    pw = K.Conv2d(32, 32, 1, bias=False).to(DEV)
    ga = gy.to(DEV).contiguous(memory_format=CL)
    gb_cpu = torch.randn(2, 32, 13, 11)
    gb = gb_cpu.to(DEV).contiguous(memory_format=CL)
    xs = [x.to(DEV).contiguous(memory_format=CL).requires_grad_(True) for _ in range(2)]
    with recorded_calls(K) as seen:
        for order in (0, 1):
            xj = xs[order]
            join = K.grad_join(xj, 2)
            assert join is not None
            if order == 0:                                    # (autograd runs the later consumer's backward first)
                ya = gc(xj, grad_link=join)
                yb = pw(xj, grad_link=join)
            else:
                yb = pw(xj, grad_link=join)
                ya = gc(xj, grad_link=join)
            ((ya * ga).sum() + (yb * gb).sum()).backward()
        K.wgrad_stream_sync()
    torch.cuda.synchronize()
    assert len(seen.get("u2pl_gconv2d_dgrad_f32", [])) == 2
    ref_a, bound_a = B.refs(case, x, w, gy)["dx"]
    ref_b, bound_b = conv_dx_bound(gb_cpu, pw.weight.detach().cpu(), (13, 11))
    ref, part = ref_a + ref_b, bound_a + bound_b
    assert float(ref_a.abs().max()) > 0 and float(ref_b.abs().max()) > 0
    for order in (0, 1):
        e = excess(xs[order].grad, ref, part + EPS * (ref.abs() + part))
        print("grad join order %d: excess %.4f" % (order, e))
        assert e <= 1.0, (order, e)
    # ... and the join has added something: the grouped gradient alone misses the sum
    assert excess(xs[0].grad, ref_a, bound_a) > 1.0
