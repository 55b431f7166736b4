"""-m gpu: region pool and region attention (csrc/ocr.hip, nn._RegionPoolFn / nn._RegionAttnFn) and the OCRNet decoder
(models.decoder.dec_ocrnet).

The four entry points through the C ABI, element-wise against float64: references, operands, tables and the bounds
|got - ref64| <= EPS min(derived, CAL_MARGIN measured (1 + arg)) unit + floor are those of tests/ocr_bounds.py; tests/test_ocr_cpu.py
shows that these bounds on these tables separate a float32 emulation of the kernels' order from the faulty ones.  Inputs are read
from pitched buffers whose gaps hold NaN; every output lies in a sentinel frame that must survive; workspaces are filled with NaN
and followed by a sentinel tail; each call runs twice and must give the same bits.  The backward calls are handed the float64
forward's m, f and w rounded to fp32 (ocr_bounds: the references are evaluated on exactly those values).

The decoder against its float64 twin (torch softmax / einsum, F.conv2d, F.batch_norm): dec_ocrnet(in_planes=128, inner_planes=64,
key_planes=32, rep_head=True), Dropout2d p = 0, 4 x 128 x 9 x 9, train mode; figures and yardstick are those of
decoder_harness.assert_no_worse_than_deeplabv3: max|got - ref| / max|ref| of every output, dx and every
parameter gradient <= 2x the largest figure of dec_deeplabv3(in_planes=128, dilations=(1, 2, 12)) against its own twin.

The whole path: ResNet-50 + dec_ocrnet through ModelBuilder at 65 x 65 (a 9 x 9 decoder input)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ocr_bounds as B
from decoder_harness import (CL, DEV, S_NET, SENT, D, Rows, Ws, _merge, _ptr, _seq64, _show, _twice,
                             assert_default_config_is_untouched, assert_eval_forward_ignores_the_graph,
                             assert_no_worse_than_deeplabv3, assert_replay_equals_eager, build_net, call, decoder_cfg, net_input,
                             query, step_calls, train_steps)
from split_bounds import recorded_calls

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
PF, PB, AF, AB = "u2pl_region_pool_fwd_f32", "u2pl_region_pool_bwd_f32", "u2pl_region_attn_fwd_f32", "u2pl_region_attn_bwd_f32"


def raw_pool_fwd(s, x, scale, pitched):
    N, HW, K = s.shape
    C = x.shape[2]
    sin, xin = Rows(s.shape, pitched, np.nan, s, wide=False), Rows(x.shape, pitched, np.nan, x)

    def run(o):
        ws = Ws(query("u2pl_region_pool_fwd_ws_floats", N, HW, K, C))
        call(PF, sin.ptr, sin.ld, xin.ptr, xin.ld, scale, N, HW, K, C, *_ptr(o["m"]), *_ptr(o["f"]), ws.buf)
        return ws
    r = _twice("region pool forward", run, lambda: dict(m=Rows(s.shape, pitched, SENT, wide=False), f=Rows((N, K, C), pitched, SENT)))
    return r["m"], r["f"]


def raw_pool_bwd(g, m, x, f, add, scale, pitched, want=("dx", "ds")):
    N, HW, K = m.shape
    C = x.shape[2]
    gin = None if g is None else Rows(g.shape, pitched, np.nan, g)
    ain = None if add is None else Rows(add.shape, pitched, np.nan, add)
    min_, xin, fin = Rows(m.shape, pitched, np.nan, m, wide=False), Rows(x.shape, pitched, np.nan, x), Rows(f.shape, pitched, np.nan, f)

    def run(o):
        ws = Ws(query("u2pl_region_pool_bwd_ws_floats", N, HW, K, C))
        call(PB, *_ptr(gin), min_.ptr, min_.ld, xin.ptr, xin.ld, fin.ptr, fin.ld, *_ptr(ain), scale, N, HW, K, C, *_ptr(o["dx"]),
             *_ptr(o["ds"]), ws.buf)
        return ws
    r = _twice("region pool backward", run, lambda: dict(dx=Rows(x.shape, pitched, SENT) if "dx" in want else None,
                                                         ds=Rows(m.shape, pitched, SENT, wide=False) if "ds" in want else None))
    return r.get("dx"), r.get("ds")


def raw_attn_fwd(q, kk, v, scale, pitched):
    N, HW, Dm = q.shape
    K = kk.shape[1]
    qin, kin, vin = (Rows(t.shape, pitched, np.nan, t) for t in (q, kk, v))

    def run(o):
        call(AF, qin.ptr, qin.ld, kin.ptr, kin.ld, vin.ptr, vin.ld, scale, N, HW, K, Dm, *_ptr(o["w"]), *_ptr(o["y"]))
    r = _twice("region attention forward", run, lambda: dict(w=Rows((N, HW, K), pitched, SENT, wide=False), y=Rows(q.shape, pitched, SENT)))
    return r["w"], r["y"]


def raw_attn_bwd(gy, w, q, kk, v, scale, pitched, want=("dq", "dk", "dv")):
    N, HW, Dm = q.shape
    K = kk.shape[1]
    gin, qin, kin, vin = (Rows(t.shape, pitched, np.nan, t) for t in (gy, q, kk, v))
    win = Rows(w.shape, pitched, np.nan, w, wide=False)

    def run(o):
        ws = Ws(query("u2pl_region_attn_bwd_ws_floats", N, HW, K, Dm))
        call(AB, gin.ptr, gin.ld, win.ptr, win.ld, qin.ptr, qin.ld, kin.ptr, kin.ld, vin.ptr, vin.ld, scale, N, HW, K, Dm,
             *_ptr(o["dq"]), *_ptr(o["dk"]), *_ptr(o["dv"]), ws.buf)
        return ws
    shapes = dict(dq=q.shape, dk=kk.shape, dv=kk.shape)
    return _twice("region attention backward", run, lambda: {k: Rows(shapes[k], pitched, SENT) if k in want else None for k in shapes})


def check_case(N, HW, K, C, family, pitched, variants):
    """all four entry points on one shape -> {output: largest error / bound}"""
    worst = {}

    def up(**kw):
        for k, v in kw.items():
            worst[k] = max(worst.get(k, 0.0), v)
    hw = B.hw_of(HW)
    s, x, g, add = B.pool_case(N, hw, K, C, family)
    sc = B.pool_scale(N)
    m, f = raw_pool_fwd(s, x, sc, pitched)
    em, ef = B.pool_fwd_excess(m, f, s, x, sc)
    up(m=em, f=ef)
    r = B.pool_fwd64(s, x, sc)
    m32, f32_ = r["m"].astype(f32), r["f"].astype(f32)
    forms = [(g, add, ("dx", "ds"))]
    if variants:
        forms += [(g, None, ("dx", "ds")), (None, add, ("dx", "ds")), (None, None, ("dx", "ds")), (g, add, ("dx",)), (g, None, ("ds",))]
    for g_, a_, want in forms:
        dx, ds = raw_pool_bwd(g_, m32, x, f32_, a_, sc, pitched, want)
        edx, eds = B.pool_bwd_excess(dx, ds, g_, m32, x, f32_, a_, sc)
        up(dx=edx, ds=eds)
    q, kk, v, gy = B.attn_case(N, hw, K, C, family)
    sc = B.attn_scale(C)
    w, y = raw_attn_fwd(q, kk, v, sc, pitched)
    ew, ey = B.attn_fwd_excess(w, y, q, kk, v, sc)
    up(w=ew, y=ey)
    w32 = B.attn_fwd64(q, kk, v, sc)["w"].astype(f32)
    for want in [("dq", "dk", "dv")] + ([("dq",), ("dk",), ("dv",), ("dk", "dv")] if variants else []):
        got = raw_attn_bwd(gy, w32, q, kk, v, sc, pitched, want)
        assert sorted(got) == sorted(want)
        up(**B.attn_bwd_excess(got, gy, w32, q, kk, v, sc))
    return worst


@pytest.mark.parametrize("K", B.OCR_K)
@pytest.mark.parametrize("HW", B.OCR_HW, ids=lambda s: "x".join(map(str, s)))
def test_kernels_hold_the_float64_bounds(HW, K):
    worst = {}
    for N, C in ((1, 4), (1, 260), (3, 20), (3, 64)):
        worst = _merge(worst, check_case(N, HW, K, C, "normal", pitched=C in (4, 64), variants=B.hw_of(HW) <= 6 and K in (2, 19, 65)))
    _show("%s K = %d" % (HW, K), worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("family", B.FAMILIES[1:])
def test_logits_of_100_and_a_constant_class_hold_the_bounds(family):
    worst = {}
    for N, HW, K, C in ((3, (7, 10), 19, 20), (1, (33, 35), 65, 64), (3, (1, B.SLAB + 1), 2, 4)):
        worst = _merge(worst, check_case(N, HW, K, C, family, pitched=N == 3, variants=False))
    _show(family, worst)
    assert max(worst.values()) <= 1.0, worst


def test_first_size_past_the_grid_cap_of_the_kernels_that_walk_pixels():
    """the three column kernels (N slabs), k_region_wsum (N slabs at one channel chunk and one region chunk) and the three per-pixel
    kernels (N HW / 4 pixel groups, four per block) take a second trip of their grid-stride loops"""
    c = B.GRID_CASE
    hw = B.hw_of(c["HW"])
    assert c["N"] * B.cdiv(hw, B.SLAB) > B.GRID_CAP and c["N"] * B.cdiv(hw, B.PX) > 4 * B.GRID_CAP
    worst = check_case(c["N"], c["HW"], c["K"], c["C"], "normal", pitched=True, variants=False)
    _show("%d x %d pixels" % (c["N"], hw), worst)
    assert max(worst.values()) <= 1.0, worst


def test_first_size_past_the_grid_cap_of_the_kernels_that_walk_region_rows():
    """k_region_wsum_reduce (f, dv, dk: N K C / 4 float4 items, 256 per block) and k_region_rowdot (c of the pool backward: N K
    rows, four per block) take a second trip"""
    c = B.REDUCE_GRID_CASE
    assert c["N"] * c["K"] * c["C"] // 4 > 256 * B.GRID_CAP
    worst = check_case(c["N"], c["HW"], c["K"], c["C"], "normal", pitched=False, variants=False)
    _show("reduce: %d x %d rows of %d channels" % (c["N"], c["K"], c["C"]), worst)
    assert max(worst.values()) <= 1.0, worst
    c = B.ROWDOT_GRID_CASE
    assert c["N"] * c["K"] > 4 * B.GRID_CAP
    worst = check_case(c["N"], c["HW"], c["K"], c["C"], "normal", pitched=True, variants=False)
    _show("row dot: %d x %d rows" % (c["N"], c["K"]), worst)
    assert max(worst.values()) <= 1.0, worst


def test_out_of_contract_arguments_return_1001_and_leave_the_outputs_alone():
    from u2pl_amd._lib import HipError
    big = [torch.full((4096,), float(SENT), device=DEV) for _ in range(4)]
    o0, o1, o2, ws = big
    src = torch.ones(4096, device=DEV)
    off = src[1:]                                                  # a base that is not 16-byte aligned
    bad = [(PF, src, 2, src, 8, 1.0, 1, 6, 2, 6, o0, 2, o1, 8, ws),                 # C % 4
           (PF, src, 2, src, 8, 1.0, 1, 6, 0, 8, o0, 2, o1, 8, ws),                 # K = 0
           (PF, src, 256, src, 8, 1.0, 1, 6, 256, 8, o0, 256, o1, 8, ws),           # K = 256
           (PF, src, 1, src, 8, 1.0, 1, 6, 2, 8, o0, 2, o1, 8, ws),                 # pitch of s below K
           (PF, src, 2, src, 6, 1.0, 1, 6, 2, 8, o0, 2, o1, 8, ws),                 # pitch of x below C
           (PF, src, 2, src, 10, 1.0, 1, 6, 2, 8, o0, 2, o1, 8, ws),                # pitch of x not a multiple of 4
           (PF, src, 2, off, 8, 1.0, 1, 6, 2, 8, o0, 2, o1, 8, ws),                 # x not 16-byte aligned
           (PF, src, 2, src, 8, 1.0, 1, 6, 2, 8, o0, 2, o1, 8, None),               # a null workspace
           (PF, src, 2, src, 8, 1.0, 1, 6, 2, 8, None, 2, o1, 8, ws),               # a null m
           (PF, src, 2, src, 8, 1.0, 0, 6, 2, 8, o0, 2, o1, 8, ws),                 # N = 0
           (PB, src, 8, src, 2, src, 8, src, 8, None, 8, 1.0, 1, 6, 2, 8, None, 8, None, 2, ws),     # neither dx nor ds
           (PB, src, 6, src, 2, src, 8, src, 8, None, 8, 1.0, 1, 6, 2, 8, o0, 8, o1, 2, ws),         # pitch of g_f below C
           (PB, src, 8, src, 2, src, 8, src, 8, src, 9, 1.0, 1, 6, 2, 8, o0, 8, o1, 2, ws),          # pitch of add
           (PB, src, 8, src, 2, src, 8, src, 8, None, 8, 1.0, 1, 6, 2, 8, o0, 8, o1, 1, ws),         # pitch of ds below K
           (AF, src, 8, src, 8, src, 8, 0.5, 1, 6, 300, 8, o0, 300, o1, 8),         # K > 255
           (AF, src, 8, src, 8, src, 8, 0.5, 1, 6, 2, 10, o0, 2, o1, 12),           # D % 4
           (AF, src, 8, None, 8, src, 8, 0.5, 1, 6, 2, 8, o0, 2, o1, 8),            # null keys
           (AF, src, 8, src, 8, src, 8, 0.5, 1, 6, 2, 8, o0, 2, off, 8),            # y not 16-byte aligned
           (AB, src, 8, src, 2, src, 8, src, 8, src, 8, 0.5, 1, 6, 2, 8, None, 8, None, 8, None, 8, ws),      # no output asked for
           (AB, src, 8, src, 2, None, 8, src, 8, src, 8, 0.5, 1, 6, 2, 8, o0, 8, o1, 8, o2, 8, ws),          # dk without q
           (AB, src, 8, src, 2, src, 8, src, 8, src, 8, 0.5, 1, 6, 2, 8, o0, 8, o1, 6, o2, 8, ws)]           # pitch of dk
    for args in bad:
        with pytest.raises(HipError, match="1001"):
            call(*args)
    torch.cuda.synchronize()
    assert all(bool((o.view(torch.int32) == B.SENTINEL_BITS).all()) for o in big)
    for name in ("u2pl_region_pool_fwd_ws_floats", "u2pl_region_pool_bwd_ws_floats", "u2pl_region_attn_bwd_ws_floats"):
        assert query(name, 1, 6, 256, 8) == 0 and query(name, 1, 6, 2, 6) == 0 and query(name, 1, 6, 2, 8) > 0


# ---- the autograd Functions ---------------------------------------------------------------------------------------------------
def act(rows, N, H, W):
    """[N, H W, C] numpy -> channels_last [N, C, H, W] on the device"""
    return D(rows).reshape(N, H, W, -1).permute(0, 3, 1, 2)


def rows_of(t):
    """[N, C, H, W] tensor -> [N, H W, C] numpy"""
    N, C, H, W = t.shape
    return t.detach().permute(0, 2, 3, 1).reshape(N, H * W, C).cpu().numpy()


@pytest.mark.parametrize("N,C,HW,K", [(3, 20, (7, 10), 19), (1, 64, (2, 3), 2), (2, 260, (13, 21), 65)], ids=["7x10", "2x3", "13x21"])
def test_region_pool_function_gives_the_bits_of_the_raw_calls(N, C, HW, K):
    from u2pl_amd import nn as Kn
    hw = B.hw_of(HW)
    s, x, g, add = B.pool_case(N, hw, K, C)
    xd, sd = act(x, N, *HW).requires_grad_(True), act(s, N, *HW).requires_grad_(True)
    gd, ad = D(g).permute(0, 2, 1).unsqueeze(3), act(add, N, *HW)
    with recorded_calls(Kn) as seen:
        x_pass, f = Kn.region_pool(xd, sd, 0.7)
        assert x_pass.data_ptr() == xd.data_ptr() and x_pass.shape == xd.shape and f.shape == (N, C, K, 1)     # handed through
        torch.autograd.backward((x_pass, f), (ad, gd))
    torch.cuda.synchronize()
    assert {k: len(v) for k, v in seen.items()} == {PF: 1, PB: 1}
    m, fr = raw_pool_fwd(s, x, 0.7, False)
    assert B.bits_equal(rows_of(f), fr)
    dx, ds = raw_pool_bwd(g, m, x, fr, add, 0.7, False)
    assert B.bits_equal(rows_of(xd.grad), dx) and B.bits_equal(rows_of(sd.grad), ds)
    # only f used: a null add; only the pass-through used: dx is the incoming gradient and no launch is made
    xd.grad = sd.grad = None
    Kn.region_pool(xd, sd, 0.7)[1].backward(gd)
    dx, ds = raw_pool_bwd(g, m, x, fr, None, 0.7, False)
    assert B.bits_equal(rows_of(xd.grad), dx) and B.bits_equal(rows_of(sd.grad), ds)
    xd.grad = sd.grad = None
    with recorded_calls(Kn) as seen:
        Kn.region_pool(xd, sd, 0.7)[0].backward(ad)
    assert B.bits_equal(rows_of(xd.grad), add) and sd.grad is None and PB not in seen
    # s needs no gradient: the ds output is not asked for
    xd.grad = None
    with recorded_calls(Kn) as seen:
        Kn.region_pool(xd, sd.detach(), 0.7)[1].backward(gd)
    assert seen[PB][0][-3] is None and B.bits_equal(rows_of(xd.grad), dx)


@pytest.mark.parametrize("N,Dm,HW,K", [(3, 20, (7, 10), 19), (1, 64, (2, 3), 2), (2, 260, (13, 21), 65)], ids=["7x10", "2x3", "13x21"])
def test_region_attention_function_gives_the_bits_of_the_raw_calls(N, Dm, HW, K):
    from u2pl_amd import nn as Kn
    hw = B.hw_of(HW)
    q, kk, v, gy = B.attn_case(N, hw, K, Dm)
    sc = B.attn_scale(Dm)
    qd = act(q, N, *HW).requires_grad_(True)
    kd, vd = (D(t).permute(0, 2, 1).unsqueeze(3).requires_grad_(True) for t in (kk, v))
    with recorded_calls(Kn) as seen:
        y = Kn.region_attention(qd, kd, vd, sc)
        y.backward(act(gy, N, *HW))
    torch.cuda.synchronize()
    assert {k: len(v_) for k, v_ in seen.items()} == {AF: 1, AB: 1}
    w, yr = raw_attn_fwd(q, kk, v, sc, False)
    assert y.shape == qd.shape and B.bits_equal(rows_of(y), yr)
    got = raw_attn_bwd(gy, w, q, kk, v, sc, False)
    assert B.bits_equal(rows_of(qd.grad), got["dq"])
    assert B.bits_equal(kd.grad.squeeze(3).permute(0, 2, 1).cpu().numpy(), got["dk"])
    assert B.bits_equal(vd.grad.squeeze(3).permute(0, 2, 1).cpu().numpy(), got["dv"])


def test_region_shapes_are_checked_before_any_call():
    from u2pl_amd import nn as Kn
    with recorded_calls(Kn) as seen:
        for x, s in ((torch.zeros(1, 6, 2, 2), torch.zeros(1, 2, 2, 2)), (torch.zeros(1, 8, 2, 2), torch.zeros(1, 256, 2, 2)),
                     (torch.zeros(1, 8, 2, 2), torch.zeros(1, 2, 2, 3)), (torch.zeros(2, 8, 2, 2), torch.zeros(1, 2, 2, 2))):
            with pytest.raises(ValueError):
                Kn.region_pool(x.to(DEV), s.to(DEV))
        with pytest.raises(ValueError):
            Kn.region_attention(torch.zeros(1, 8, 2, 2, device=DEV), torch.zeros(1, 8, 256, 1, device=DEV),
                                torch.zeros(1, 8, 256, 1, device=DEV), 1.0)
        with pytest.raises(ValueError):
            Kn.region_attention(torch.zeros(1, 8, 2, 2, device=DEV), torch.zeros(1, 8, 3, 1, device=DEV),
                                torch.zeros(1, 8, 2, 1, device=DEV), 1.0)
    assert not seen


def test_concat_consumer_gradient_goes_in_as_the_add_operand():
    """x -> (x_pass, f); cat(y, x_pass) -> loss: the slice of the concat's gradient reaches the backward kernel as `add` (no copy:
    its pitch is the concat's width), exactly one backward launch writes dx, and x.grad holds the dx bound with that add"""
    from u2pl_amd import nn as Kn
    N, C, HW, K = 3, 20, (7, 10), 19
    hw = B.hw_of(HW)
    s, x, g, _ = B.pool_case(N, hw, K, C)
    G = np.random.default_rng(5).standard_normal((N, hw, C + 8), dtype=f32)
    xd, sd = act(x, N, *HW).requires_grad_(True), act(s, N, *HW).requires_grad_(True)
    Gd = act(G, N, *HW)
    gd = D(g).permute(0, 2, 1).unsqueeze(3)
    other = act(G[:, :, :8], N, *HW).contiguous(memory_format=CL)
    with recorded_calls(Kn) as seen:
        x_pass, f = Kn.region_pool(xd, sd, 1.0)
        feat = Kn.cat_channels((other, x_pass))
        torch.autograd.backward((feat, f), (Gd, gd))
    torch.cuda.synchronize()
    assert len(seen[PB]) == 1
    a = seen[PB][0]
    add_t, ldadd = a[8], a[9]
    assert ldadd == C + 8 and add_t.data_ptr() == Gd.data_ptr() + 8 * 4          # the slice itself, at the concat's pitch
    assert not [args for args in seen.get("u2pl_copy_rows_f32", []) if args[6]]  # no accumulating copy anywhere
    add = np.ascontiguousarray(G[:, :, 8:])
    m, fr = raw_pool_fwd(s, x, 1.0, False)
    edx, eds = B.pool_bwd_excess(rows_of(xd.grad), rows_of(sd.grad), g, m, x, fr, add, 1.0)
    print("\n  x.grad, s.grad against float64: %.3f %.3f of the bound" % (edx, eds), end="")
    assert edx <= 1.0 and eds <= 1.0
    dx, ds = raw_pool_bwd(g, m, x, fr, add, 1.0, False)
    assert B.bits_equal(rows_of(xd.grad), dx) and B.bits_equal(rows_of(sd.grad), ds)


# ---- the decoder against its float64 twin -------------------------------------------------------------------------------------
def _ocr_twin(dec, p, x):
    feat = _seq64(dec.conv3x3, p, "conv3x3", x)
    r = _seq64(dec.region, p, "region", x)
    N, C, H, W = feat.shape
    K = r.shape[1]
    m = torch.softmax(r.reshape(N, K, H * W), 2)                                          # over the pixels of an image
    f = torch.einsum("nkp,ncp->nck", m, feat.reshape(N, C, H * W)).unsqueeze(3)             # [N, C, K, 1]
    q = _seq64(dec.f_pixel, p, "f_pixel", feat)
    kk, v = _seq64(dec.f_object, p, "f_object", f), _seq64(dec.f_down, p, "f_down", f)
    Dk = q.shape[1]
    w = torch.softmax(torch.einsum("ndp,ndk->npk", q.reshape(N, Dk, H * W), kk.squeeze(3)) * dec.key_planes ** -0.5, 2)
    y = torch.einsum("npk,ndk->ndp", w, v.squeeze(3)).reshape(N, Dk, H, W)
    out = _seq64(dec.fuse, p, "fuse", torch.cat((_seq64(dec.f_up, p, "f_up", y), feat), 1))
    return dict(pred=F.conv2d(out, p["classifier.weight"], p["classifier.bias"]), region=r,
                rep=_seq64(dec.representation, p, "representation", out))


def test_ocrnet_decoder_is_no_worse_than_the_deeplabv3_decoder():
    from u2pl_amd.models.decoder import dec_ocrnet
    assert_no_worse_than_deeplabv3(
        "dec_ocrnet", lambda: dec_ocrnet(in_planes=128, inner_planes=64, key_planes=32, rep_head=True), _ocr_twin,
        ("pred", "region", "rep"),
        {"pred", "region", "rep", "dx", "conv3x3.0.weight", "region.3.bias", "f_pixel.4.weight", "f_object.3.weight", "f_down.1.bias",
         "f_up.0.weight", "fuse.0.weight", "classifier.bias", "representation.4.weight"}, show_v3=True)


# ---- the whole path -----------------------------------------------------------------------------------------------------------
OCR_DECODER = dict(type="u2pl.models.decoder.dec_ocrnet", kwargs=dict(rep_head=True))


@pytest.fixture(scope="module")
def ocrnet():
    return build_net(decoder_cfg(OCR_DECODER)), net_input()


def test_ocrnet_train_step_reaches_every_parameter(ocrnet):
    from u2pl_amd import nn as Kn
    model, x = ocrnet
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    seen, outs = step_calls(model, x, ("pred", "rep", "aux", "region"))
    assert sorted(outs) == ["aux", "pred", "region", "rep"] and outs["region"].shape == (4, 19, 9, 9)
    assert [len(seen[n_]) for n_ in (PF, PB, AF, AB)] == [1, 1, 1, 1]
    assert seen[PF][0][5:9] == (4, 81, 19, 512) and seen[AF][0][7:11] == (4, 81, 19, 256)
    assert seen[PB][0][8] is not None and seen[PB][0][15] is not None and seen[PB][0][17] is not None      # add, dx and ds are there
    missing = [n_ for n_, p in model.named_parameters() if p.grad is None]
    assert not missing, missing
    bad = [n_ for n_, p in model.named_parameters() if not bool(torch.isfinite(p.grad).all())]
    zero = [n_ for n_, p in model.named_parameters() if not bool(p.grad.ne(0).any())]
    assert not bad and not zero, (bad, zero)
    before = [p.detach().clone() for p in model.parameters()]
    opt.step()
    Kn.invalidate_weights()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))


def test_ocrnet_eval_forward_is_the_same_with_and_without_a_graph(ocrnet):
    assert_eval_forward_ignores_the_graph(ocrnet, ("pred", "rep", "region"))


def test_default_config_makes_no_region_call_and_the_same_calls_after_an_ocrnet_step(ocrnet):
    assert_default_config_is_untouched(ocrnet, PF, "u2pl_region")


def test_ocrnet_graph_replay_is_bit_identical_to_eager(monkeypatch):
    """the meters' supervised loss holds the region term"""
    a, b = (train_steps(monkeypatch, on, lambda cfg: cfg["net"].update(decoder=OCR_DECODER)) for on in (True, False))
    print("graph stats", a["stats"])
    assert_replay_equals_eager(a, b)


def test_ocrnet_region_loss_is_finite_and_reaches_only_the_region_head():
    """trainer.add_region_loss on a ResNet-50 + dec_ocrnet forward: the term is 0.4 x the cross entropy of the up-sampled regions
    of the labelled half (against torch in float64), its backward reaches the region head and not the classifier, and a decoder
    with region_loss_weight = 0 gets the supervised loss back as it is"""
    from u2pl_amd import nn as Kn
    from u2pl_amd.trainer import add_region_loss
    model, x = build_net(decoder_cfg(OCR_DECODER)).train(), net_input()
    label = torch.randint(0, 19, (2, S_NET, S_NET), generator=torch.Generator().manual_seed(2)).to(DEV)
    label[:, :6] = 255
    outs = model(x)
    zero = torch.zeros((), device=DEV)
    cfg = dict(dataset=dict(ignore_label=255))
    loss = add_region_loss(zero, model, outs, 2, (S_NET, S_NET), label, cfg)
    ref = 0.4 * F.cross_entropy(F.interpolate(outs["region"][:2].detach().double(), size=(S_NET, S_NET), mode="bilinear",
                                              align_corners=True), label, ignore_index=255)
    assert bool(torch.isfinite(loss)) and abs(float(loss) - float(ref)) <= 1e-5 * float(ref), (float(loss), float(ref))
    loss.backward()
    Kn.wgrad_stream_sync()
    torch.cuda.synchronize()
    g = model.decoder.region[3].weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and bool(g.ne(0).any())
    assert model.decoder.classifier.weight.grad is None                     # only the region head and what feeds it
    model.decoder.region_loss_weight = 0.0
    assert add_region_loss(zero, model, model(x), 2, (S_NET, S_NET), label, cfg) is zero
