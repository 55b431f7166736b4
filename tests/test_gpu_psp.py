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
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import psp_bounds as B
from model_utils import net_cfg
from split_bounds import EPS, recorded_calls

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
f32, f64 = np.float32, np.float64
FWD, BWD = "u2pl_pyramid_pool_fwd_f32", "u2pl_pyramid_pool_bwd_f32"
SENT = B.sentinel()


def call(*a):
    from u2pl_amd._lib import call as c
    return c(*a)


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Rows:
    """rows [M, C] inside a buffer of M + 2 rows of ld floats filled with `fill`, starting at row 1 and column `off`: NaN for an
    input (no kernel may read the gaps), the sentinel for an output (no kernel may write the frame)"""

    def __init__(self, M, C, pitched, fill, rows=None):
        self.M, self.C = M, C
        self.ld, self.off = (C + 12, 8) if pitched else (C, 0)
        host = np.full((M + 2, self.ld), fill, dtype=f32)
        if rows is not None:
            host[1:M + 1, self.off:self.off + C] = rows
        self.buf = D(host)
        self.ptr = self.buf[1:, self.off:]      # the kernel's base pointer: row r, column c at ptr + r ld + c

    def rows(self):
        return self.buf.cpu().numpy()[1:self.M + 1, self.off:self.off + self.C].copy()

    def assert_frame_intact(self, what):
        bits = self.buf.cpu().numpy().view(np.uint32).copy()
        bits[1:self.M + 1, self.off:self.off + self.C] = B.SENTINEL_BITS
        assert (bits == B.SENTINEL_BITS).all(), f"{what}: wrote outside its {self.M} x {self.C} rows (ld {self.ld})"


def lv4(levels):
    return tuple(levels) + (0,) * (4 - len(levels))


def raw_fwd(x, levels, pitched):
    """-> {slot: y [N, C, b, b]} through the C ABI, twice, frames checked"""
    N, C, H, W = x.shape
    xin = Rows(N * H * W, C, pitched, np.nan, B.rows_of(x))
    outs = []
    for _ in range(2):
        ys = {k: Rows(N * b * b, C, pitched, SENT) for k, b in B.used(lv4(levels))}
        args = []
        for k in range(4):
            args += [ys[k].ptr, ys[k].ld] if k in ys else [None, 0]
        call(FWD, xin.ptr, xin.ld, N, H, W, C, *lv4(levels), *args)
        torch.cuda.synchronize()
        for k, r in ys.items():
            r.assert_frame_intact("forward level slot %d" % k)
        outs.append({k: r.rows() for k, r in ys.items()})
    assert all(B.bits_equal(outs[0][k], outs[1][k]) for k in outs[0]), "two forward runs differ"
    return {k: B.from_rows(v, N, lv4(levels)[k], lv4(levels)[k]) for k, v in outs[0].items()}


def raw_bwd(gs, levels, add, shape, pitched):
    """-> dx [N, C, H, W]; gs: {slot: g}, a missing slot of a used level goes in as a null pointer; add may be None"""
    N, C, H, W = shape
    gin = {k: Rows(g.shape[0] * g.shape[2] * g.shape[3], C, pitched, np.nan, B.rows_of(g)) for k, g in gs.items()}
    ain = None if add is None else Rows(N * H * W, C, pitched, np.nan, B.rows_of(add))
    args = []
    for k in range(4):
        args += [gin[k].ptr, gin[k].ld] if k in gin else [None, 0]
    outs = []
    for _ in range(2):
        dx = Rows(N * H * W, C, pitched, SENT)
        call(BWD, *args, None if ain is None else ain.ptr, 0 if ain is None else ain.ld, N, H, W, C, *lv4(levels), dx.ptr, dx.ld)
        torch.cuda.synchronize()
        dx.assert_frame_intact("backward")
        outs.append(dx.rows())
    assert B.bits_equal(outs[0], outs[1]), "two backward runs differ"
    return B.from_rows(outs[0], N, H, W)


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
def _seq64(seq, p, prefix, x):
    """an nn.Sequential of a decoder in float64 (Dropout2d: p = 0 in these tests; the pooling marker is the caller's)"""
    from u2pl_amd import nn as K
    for i, m in enumerate(seq):
        name = "%s.%d" % (prefix, i)
        if isinstance(m, K.Conv2d):
            x = F.conv2d(x, p[name + ".weight"], p.get(name + ".bias"), stride=m.stride, padding=m.padding, dilation=m.dilation)
        elif isinstance(m, K.BatchNorm2d):
            x = F.batch_norm(x, None, None, p[name + ".weight"], p[name + ".bias"], training=True, eps=m.eps)
        elif isinstance(m, torch.nn.ReLU):
            x = torch.relu(x)
        elif isinstance(m, torch.nn.AdaptiveAvgPool2d):
            x = F.adaptive_avg_pool2d(x, m.output_size)
        else:
            assert isinstance(m, torch.nn.Dropout2d) and m.p == 0, m
    return x


def _psp_twin(dec, p, x):
    h, w = x.shape[2:]
    ups = [F.interpolate(_seq64(m, p, "ppm.%d" % i, x), size=(h, w), mode="bilinear", align_corners=True)
           for i, m in enumerate(dec.ppm)]
    feat = _seq64(dec.head, p, "head", torch.cat([x] + ups, 1))
    pred = F.conv2d(feat, p["classifier.weight"], p["classifier.bias"])
    return dict(pred=pred, rep=_seq64(dec.representation, p, "representation", feat))


def _v3_twin(dec, p, x):
    h, w = x.shape[2:]
    a = dec.aspp
    pooled = F.interpolate(_seq64(a.conv1, p, "aspp.conv1", x), size=(h, w), mode="bilinear", align_corners=True)
    feats = [pooled] + [_seq64(getattr(a, n), p, "aspp." + n, x) for n in ("conv2", "conv3", "conv4", "conv5")]
    return dict(pred=_seq64(dec.head, p, "head", torch.cat(feats, 1)))


def _figures(dec, twin, keys, seed=0):
    from u2pl_amd import nn as K
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
    x = torch.relu(torch.randn(4, 128, 9, 9, generator=g)).contiguous(memory_format=CL)
    xd = x.to(DEV).requires_grad_(True)
    out = dec(xd)
    if not isinstance(out, dict):
        out = dict(pred=out)
    G = {k: torch.randn(out[k].shape, generator=g) for k in keys}
    sum((out[k] * G[k].to(DEV).contiguous(memory_format=CL)).sum() for k in keys).backward()
    K.wgrad_stream_sync()
    torch.cuda.synchronize()
    p = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()
         and "running" not in k}
    x64 = x.double().clone().requires_grad_(True)
    ref_out = twin(dec, p, x64)
    sum((ref_out[k] * G[k].double()).sum() for k in keys).backward()
    ref = dict(dx=x64.grad, **{k: ref_out[k].detach() for k in keys}, **{k: v.grad for k, v in p.items()})
    got = dict(dx=xd.grad, **{k: out[k] for k in keys})
    for n_, q in dec.named_parameters():
        assert q.grad is not None, n_
        got[n_] = q.grad
    assert set(got) == set(ref)
    fig = {k: float((got[k].detach().cpu().double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in got}
    return fig, {k: tuple(ref[k].shape) for k in got}


def test_pspnet_decoder_is_no_worse_than_the_deeplabv3_decoder():
    from u2pl_amd.models.decoder import dec_deeplabv3, dec_pspnet
    torch.manual_seed(0)
    v3, v3shape = _figures(dec_deeplabv3(in_planes=128, dilations=(1, 2, 12)), _v3_twin, ("pred",))
    torch.manual_seed(0)
    psp, pshape = _figures(dec_pspnet(in_planes=128, inner_planes=64, rep_head=True), _psp_twin, ("pred", "rep"))
    top = max(v3.values())
    print("\ndecoder figures (max|got - ref| / max|ref|); largest dec_deeplabv3 figure %.3e" % top)
    for k in sorted(v3):
        print("   %-36s %-18s dec_deeplabv3 %.3e" % (k, v3shape[k], v3[k]))
    for k in sorted(psp):
        print("   %-36s %-18s dec_pspnet    %.3e" % (k, pshape[k], psp[k]))
    assert {"pred", "rep", "dx", "ppm.0.1.weight", "ppm.3.2.bias", "head.0.weight", "classifier.bias",
            "representation.4.weight"} <= set(psp)
    assert all(np.isfinite(v) for v in psp.values()) and all(np.isfinite(v) for v in v3.values())
    bad = {k: (v, top) for k, v in psp.items() if not v <= 2 * top}
    assert not bad, bad


# ---- the whole path -----------------------------------------------------------------------------------------------------------
S_NET = 65
PSP_DECODER = dict(type="u2pl.models.decoder.dec_pspnet", kwargs=dict(rep_head=True))


def _psp_cfg():
    cfg = net_cfg("resnet50", 19, True)
    cfg["encoder"]["kwargs"]["zero_init_residual"] = False   # (a zero bn3 weight would cut the gradient of each block's branch)
    cfg["decoder"] = copy.deepcopy(PSP_DECODER)
    return cfg


@pytest.fixture(scope="module")
def pspnet():
    from u2pl_amd.models.model_helper import ModelBuilder
    torch.manual_seed(0)
    model = ModelBuilder(_psp_cfg()).to(DEV)
    x = torch.randn(4, 3, S_NET, S_NET, generator=torch.Generator().manual_seed(1)).to(DEV)
    return model, x


def _step_calls(model, x):
    from u2pl_amd import nn as K
    with recorded_calls(K) as seen:
        outs = model(x)
        g = torch.Generator().manual_seed(2)
        loss = sum((outs[k] * torch.randn(outs[k].shape, generator=g).to(DEV)).sum() for k in ("pred", "rep", "aux"))
        loss.backward()
        K.wgrad_stream_sync()
    torch.cuda.synchronize()
    return seen


def test_pspnet_train_step_reaches_every_parameter(pspnet):
    from u2pl_amd import nn as K
    model, x = pspnet
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    seen = _step_calls(model, x)
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
    model, x = pspnet
    model.eval()
    try:
        with torch.no_grad():
            a = model(x)                          # the teacher's path
        b = model(x)                              # records an autograd graph
        assert b["pred"].requires_grad and a["pred"].shape == (4, 19, 9, 9) and a["rep"].shape == (4, 256, 9, 9)
        for k in ("pred", "rep"):
            assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k].detach()), k
    finally:
        model.train()


def test_pspnet_state_dict_round_trip_gives_the_same_forward(pspnet):
    from u2pl_amd.models.model_helper import ModelBuilder
    model, x = pspnet
    torch.manual_seed(99)
    fresh = ModelBuilder(_psp_cfg()).to(DEV)
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
    """the default decoder's C-ABI calls: none of the new entry points, and the same list whether or not a dec_pspnet model has
    run in the process (the new Function keeps no state that another model could meet)"""
    from u2pl_amd.models.model_helper import ModelBuilder
    counts = []
    for psp_first in (False, True):
        if psp_first:
            pspnet[0].train()
            assert FWD in _step_calls(*pspnet)
            pspnet[0].zero_grad(set_to_none=True)
        torch.manual_seed(0)
        model = ModelBuilder(net_cfg("resnet50", 19, True)).to(DEV).train()
        x = torch.randn(2, 3, S_NET, S_NET, generator=torch.Generator().manual_seed(3)).to(DEV)
        seen = _step_calls(model, x)
        assert len(seen) > 10
        assert not [n_ for n_ in seen if n_.startswith("u2pl_pyramid_pool")]
        counts.append({k: len(v) for k, v in seen.items()})
    assert counts[0] == counts[1]


def _train(monkeypatch, graphs_on, steps=4, S=S_NET):
    """tests/test_gpu_dwconv.py::_train with the pyramid-pooling decoder"""
    from u2pl_amd import configs, graphs as G
    from u2pl_amd.models.model_helper import ModelBuilder
    from u2pl_amd.trainer import SemiTrainer
    from u2pl_amd.utils.loss_helper import get_criterion

    monkeypatch.setenv("U2PL_GRAPHS", "1" if graphs_on else "0")
    cfg = configs.cityscapes_semi(arch="resnet50", crop=S, batch_size=2, sync_bn=False, epochs=20)
    cfg["net"]["decoder"] = copy.deepcopy(PSP_DECODER)
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


def test_pspnet_graph_replay_is_bit_identical_to_eager(monkeypatch):
    a = _train(monkeypatch, True)
    b = _train(monkeypatch, False)
    print("graph stats", a["stats"])
    assert a["stats"]["replays"] > 0 and a["stats"]["aborted"] == 0 and b["stats"]["replays"] == 0
    assert np.isfinite(a["meters"]).all()
    assert np.array_equal(a["meters"], b["meters"]), (a["meters"], b["meters"])
    assert torch.equal(a["w"], b["w"]) and torch.equal(a["t"], b["t"])
