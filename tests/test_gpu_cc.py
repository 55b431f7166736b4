"""-m gpu: criss-cross attention (csrc/ccattn.hip, nn._CrissCrossFn) and the CCNet decoder (models.decoder.dec_ccnet).

The two entry points through the C ABI, element-wise against float64: references, operands, tables and the bounds
|got - ref64| <= EPS min(derived, CAL_MARGIN measured (1 + arg)) unit + floor are those of tests/cc_bounds.py; tests/test_cc_cpu.py
shows that these bounds on these inputs separate a float32 emulation of the kernels' order from the faulty ones.  Inputs are read
from pitched buffers whose gaps hold NaN; every output (and w) lies in a sentinel frame that must survive; the workspace is filled
with NaN and followed by a sentinel tail; each call runs twice and must give the same bits.  The backward call is handed the
float64 forward's w rounded to fp32 (cc_bounds: the references are evaluated on exactly those values).

The decoder against its float64 twin (the plain formulas of cc_bounds in torch float64, F.conv2d, F.batch_norm):
dec_ccnet(in_planes=128, inner_planes=64, key_planes=32, rep_head=True), gamma away from 0, Dropout2d p = 0, 4 x 128 x 9 x 9, train
mode, shared and not; figures and yardstick are those of decoder_harness.assert_no_worse_than_deeplabv3:
max|got - ref| / max|ref| of every output, dx and every parameter gradient <= 2x the largest figure of
dec_deeplabv3(in_planes=128, dilations=(1, 2, 12)) against its own twin.

The whole path: ResNet-50 + dec_ccnet through ModelBuilder at 65 x 65 (a 9 x 9 decoder input)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cc_bounds as B
from decoder_harness import (DEV, SENT, D, Rows, Ws, _merge, _ptr, _seq64, _show, _twice, assert_default_config_is_untouched,
                             assert_eval_forward_ignores_the_graph, assert_no_worse_than_deeplabv3, assert_replay_equals_eager,
                             build_net, call, decoder_cfg, net_input, query, step_calls, train_steps)
from split_bounds import recorded_calls

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
CF, CB = "u2pl_cc_attn_fwd_f32", "u2pl_cc_attn_bwd_f32"
ALL = ("dq", "dk", "dv", "dgamma")


def rows3(a):
    """[N, H, W, C] -> [N, H W, C]"""
    return np.ascontiguousarray(a).reshape(a.shape[0], -1, a.shape[3])


def raw_fwd(q, k, v, res, gamma, scale, pitched):
    """u2pl_cc_attn_fwd_f32 -> (w [N, H, W, L], out [N, H, W, C])"""
    N, H, W, Dm = q.shape
    C, L = v.shape[3], H + W - 1
    qin, kin, vin = (Rows(rows3(t).shape, pitched, np.nan, rows3(t)) for t in (q, k, v))
    rin = None if res is None else Rows(rows3(res).shape, pitched, np.nan, rows3(res))
    gm = D(np.array([np.nan, gamma, np.nan], dtype=f32))[1:2]

    def run(o):
        call(CF, qin.ptr, qin.ld, kin.ptr, kin.ld, vin.ptr, vin.ld, *_ptr(rin), gm, scale, N, H, W, Dm, C, *_ptr(o["w"]), *_ptr(o["out"]))
    r = _twice("criss-cross forward", run, lambda: dict(w=Rows((N, H * W, L), pitched, SENT, wide=False), out=Rows((N, H * W, C), pitched, SENT)))
    return r["w"].reshape(N, H, W, L), r["out"].reshape(N, H, W, C)


def raw_bwd(g, w, q, k, v, gamma, scale, pitched, want=ALL, null_unread=False):
    """u2pl_cc_attn_bwd_f32 -> dict of the outputs asked for; null_unread: operands the call does not read are handed as null"""
    N, H, W, Dm = q.shape
    C, L = v.shape[3], H + W - 1
    gin, qin, kin, vin = (Rows(rows3(t).shape, pitched, np.nan, rows3(t)) for t in (g, q, k, v))
    win = Rows((N, H * W, L), pitched, np.nan, rows3(w), wide=False)
    gm = D(np.array([np.nan, gamma, np.nan], dtype=f32))[1:2]
    if null_unread:
        qin = qin if "dk" in want else None
        kin = kin if "dq" in want else None
        vin = vin if set(want) & {"dq", "dk", "dgamma"} else None

    def run(o):
        ws = Ws(query("u2pl_cc_attn_bwd_ws_floats", N, H, W, Dm, C))
        dg = o["dgamma"]
        call(CB, gin.ptr, gin.ld, win.ptr, win.ld, *_ptr(qin), *_ptr(kin), *_ptr(vin), gm, scale, N, H, W, Dm, C, *_ptr(o["dq"]),
             *_ptr(o["dk"]), *_ptr(o["dv"]), None if dg is None else dg.ptr, ws.buf)
        return ws
    shapes = dict(dq=(N, H * W, Dm), dk=(N, H * W, Dm), dv=(N, H * W, C), dgamma=(1, 1, 1))
    r = _twice("criss-cross backward", run, lambda: {n: Rows(shapes[n], pitched and n != "dgamma", SENT, wide=n != "dgamma")
                                                     if n in want else None for n in shapes})
    return {n: a.reshape(1) if n == "dgamma" else a.reshape(N, H, W, -1) for n, a in r.items()}


# the combinations of null outputs nn._CrissCrossFn can produce: any non-empty subset of (q, k, v, gamma) needs a gradient
SUBSETS = [tuple(n for i, n in enumerate(ALL) if m >> i & 1) for m in range(1, 16)]


def check_case(N, HW, Dm, C, family, pitched, variants=False, res=True, gamma=None, scale=None):
    """both entry points on one shape -> {output: largest error / bound}"""
    worst = {}

    def up(**kw):
        for n, val in kw.items():
            worst[n] = max(worst.get(n, 0.0), val)
    q, k, v, r_, g = B.cc_case(N, HW, Dm, C, family)
    r_ = r_ if res else None
    sc = B.case_scale(Dm) if scale is None else scale
    ga = B.case_gamma(HW) if gamma is None else gamma
    w, out = raw_fwd(q, k, v, r_, ga, sc, pitched)
    ew, eo = B.cc_fwd_excess(w, out, q, k, v, r_, ga, sc)
    up(w=ew, out=eo)
    w32 = B.cc_fwd64(q, k, v, r_, ga, sc)["w"].astype(f32)
    for want in [ALL] + ([s for s in SUBSETS if s != ALL] if variants else []):
        got = raw_bwd(g, w32, q, k, v, ga, sc, pitched, want, null_unread=variants)
        assert sorted(got) == sorted(want)
        up(**B.cc_bwd_excess(got, g, w32, q, k, v, ga, sc))
    return worst


@pytest.mark.parametrize("HW", B.CC_HW, ids=lambda s: "x".join(map(str, s)))
def test_kernels_hold_the_float64_bounds(HW):
    worst = {}
    for N, Dm, C in B.CC_NDC:
        worst = _merge(worst, check_case(N, HW, Dm, C, "normal", pitched=C in (4, 260)))
    _show("%d x %d, L = %d" % (HW[0], HW[1], HW[0] + HW[1] - 1), worst)
    assert max(worst.values()) <= 1.0, worst


def test_one_pixel_attends_to_itself_alone():
    q, k, v, res, g = B.cc_case(3, (1, 1), 20, 64)
    w, out = raw_fwd(q, k, v, res, 0.6, 0.7, True)
    assert w.shape == (3, 1, 1, 1) and (w == 1).all()
    assert B.bits_equal(out, B.fma(f32(0.6), v, res))


@pytest.mark.parametrize("family", B.FAMILIES[1:])
def test_scores_of_100_and_a_constant_key_hold_the_bounds(family):
    worst = {}
    for N, HW, Dm, C in ((3, (5, 3), 20, 64), (1, (33, 33), 64, 20), (3, (2, 129), 4, 4)):
        worst = _merge(worst, check_case(N, HW, Dm, C, family, pitched=N == 3))
    _show(family, worst)
    assert max(worst.values()) <= 1.0, worst


def test_every_combination_of_null_outputs_and_a_null_res():
    worst = check_case(3, (5, 3), 20, 64, "normal", pitched=True, variants=True)
    worst = _merge(worst, check_case(3, (3, 5), 8, 12, "normal", pitched=False, variants=True, res=False))
    worst = _merge(worst, check_case(1, (9, 17), 4, 260, "normal", pitched=True, res=False))
    _show("null outputs, null res", worst)
    assert max(worst.values()) <= 1.0, worst


def test_gamma_zero_and_negative_gamma():
    q, k, v, res, g = B.cc_case(3, (5, 3), 20, 64)
    sc = B.case_scale(20)
    w, out = raw_fwd(q, k, v, res, 0.0, sc, True)
    assert B.bits_equal(out, res)                                  # fma(0, sum, res)
    got = raw_bwd(g, w, q, k, v, 0.0, sc, True)
    assert not got["dq"].any() and not got["dk"].any() and not got["dv"].any()
    assert abs(float(got["dgamma"][0])) > 1e-2                     # what lets gamma leave 0
    assert max(B.cc_bwd_excess(got, g, w, q, k, v, 0.0, sc).values()) <= 1.0
    worst = check_case(3, (5, 3), 20, 64, "normal", pitched=False, gamma=-1.7)
    worst = _merge(worst, check_case(1, (32, 33), 4, 4, "normal", pitched=True, gamma=-0.3, scale=-0.9))
    _show("negative gamma", worst)
    assert max(worst.values()) <= 1.0, worst


def test_first_size_past_the_grid_cap_of_every_kernel():
    """k_cc_dots and k_cc_mix (N lines x groups work items, rows and columns), k_cc_softmax and k_cc_bwd_e (N H W pixels), four
    waves a block, take a second trip of their grid-stride loops; k_cc_sum's threads walk more than 32 partials each"""
    c = B.GRID_CASE
    H, W = c["HW"]
    assert c["N"] * H * B.cdiv(W, B.PT) > 4 * B.GRID_CAP and c["N"] * H * W > 32 * B.SUM_THREADS
    worst = check_case(c["N"], c["HW"], c["D"], c["C"], "normal", pitched=True)
    _show("%d x %d x %d pixels" % (c["N"], H, W), worst)
    assert max(worst.values()) <= 1.0, worst


def test_out_of_contract_arguments_return_1001_and_leave_the_outputs_alone():
    from u2pl_amd._lib import HipError
    big = [torch.full((4096,), float(SENT), device=DEV) for _ in range(5)]
    o0, o1, o2, o3, ws = big
    src = torch.ones(4096, device=DEV)
    off = src[1:]                                                  # a base that is not 16-byte aligned
    M = B.MAX_L

    def fwd(q=src, ldq=8, k=src, ldk=8, v=src, ldv=8, res=src, ldr=8, gamma=src, N=1, H=2, W=3, Dm=8, C=8, w=o0, ldw=4, out=o1, ldo=8):
        return (CF, q, ldq, k, ldk, v, ldv, res, ldr, gamma, 0.5, N, H, W, Dm, C, w, ldw, out, ldo)

    def bwd(g=src, ldg=8, w=src, ldw=4, q=src, ldq=8, k=src, ldk=8, v=src, ldv=8, gamma=src, N=1, H=2, W=3, Dm=8, C=8, dq=o0, lddq=8,
            dk=o1, lddk=8, dv=o2, lddv=8, dgamma=o3, ws_=ws):
        return (CB, g, ldg, w, ldw, q, ldq, k, ldk, v, ldv, gamma, 0.5, N, H, W, Dm, C, dq, lddq, dk, lddk, dv, lddv, dgamma, ws_)
    bad = [fwd(Dm=6), fwd(C=10, ldv=12, ldr=12, ldo=12), fwd(Dm=0), fwd(N=0), fwd(H=0), fwd(W=0),
           fwd(H=2, W=M, ldw=M + 1), fwd(H=M + 1, W=1, ldw=M + 1),             # L = CC_MAX_L + 1
           fwd(q=None), fwd(k=None), fwd(v=None), fwd(gamma=None), fwd(w=None), fwd(out=None),
           fwd(ldq=4), fwd(ldk=10), fwd(ldv=4), fwd(ldr=4), fwd(ldw=3), fwd(ldo=9), fwd(q=off), fwd(res=off), fwd(out=off),
           bwd(Dm=6), bwd(C=6), bwd(N=0), bwd(H=2, W=M, ldw=M + 1), bwd(g=None), bwd(w=None), bwd(gamma=None), bwd(ws_=None),
           bwd(dq=None, dk=None, dv=None, dgamma=None),                        # no output asked for
           bwd(k=None), bwd(q=None), bwd(v=None), bwd(v=None, dq=None, dk=None, dv=None),       # an operand that IS read
           bwd(ldg=4), bwd(ldw=3), bwd(lddq=4), bwd(lddk=10), bwd(lddv=4), bwd(dv=off), bwd(g=off), bwd(ws_=off)]
    for args in bad:
        with pytest.raises(HipError, match="1001"):
            call(*args)
    torch.cuda.synchronize()
    assert all(bool((o.view(torch.int32) == B.SENTINEL_BITS).all()) for o in big)
    assert query("u2pl_cc_attn_bwd_ws_floats", 1, 2, M, 8, 8) == 0 and query("u2pl_cc_attn_bwd_ws_floats", 1, 2, 3, 6, 8) == 0
    assert query("u2pl_cc_attn_bwd_ws_floats", 1, 2, 3, 8, 8) == 24 + 8
    call(*fwd())                                                   # the base case of the list is in contract
    call(*bwd())
    torch.cuda.synchronize()


# ---- the autograd Function ----------------------------------------------------------------------------------------------------
def act(a):
    """[N, H, W, C] numpy -> channels_last [N, C, H, W] on the device"""
    return D(a).permute(0, 3, 1, 2)


def map_of(t):
    """[N, C, H, W] tensor -> [N, H, W, C] numpy"""
    return t.detach().permute(0, 2, 3, 1).contiguous().cpu().numpy()


@pytest.mark.parametrize("N,Dm,C,HW", [(3, 20, 64, (7, 10)), (1, 64, 4, (2, 3)), (2, 8, 260, (13, 21))], ids=["7x10", "2x3", "13x21"])
def test_function_gives_the_bits_of_the_raw_calls(N, Dm, C, HW):
    from u2pl_amd import nn as Kn
    q, k, v, res, g = B.cc_case(N, HW, Dm, C)
    sc, ga = B.case_scale(Dm), B.case_gamma(HW)
    qd, kd, vd, rd = (act(t).requires_grad_(True) for t in (q, k, v, res))
    gm = torch.tensor([ga], device=DEV, requires_grad=True)
    gd = act(g)
    with recorded_calls(Kn) as seen:
        out = Kn.criss_cross_attention(qd, kd, vd, gm, res=rd, scale=sc)
        out.backward(gd)
    torch.cuda.synchronize()
    assert {n: len(a) for n, a in seen.items()} == {CF: 1, CB: 1}
    assert seen[CF][0][8].data_ptr() == gm.data_ptr() and seen[CB][0][10].data_ptr() == gm.data_ptr()      # gamma stays on the device
    w, outr = raw_fwd(q, k, v, res, ga, sc, False)
    assert out.shape == vd.shape and B.bits_equal(map_of(out), outr)
    got = raw_bwd(g, w, q, k, v, ga, sc, False)
    assert B.bits_equal(map_of(qd.grad), got["dq"]) and B.bits_equal(map_of(kd.grad), got["dk"]) and B.bits_equal(map_of(vd.grad), got["dv"])
    assert gm.grad.shape == (1,) and B.bits_equal(gm.grad.cpu().numpy(), got["dgamma"])
    assert rd.grad.data_ptr() == gd.data_ptr() or torch.equal(rd.grad, gd)           # the gradient of res is g itself
    # only res needs a gradient: g is handed through and no launch is made; nothing needs one: no launch either
    rd.grad = None
    with recorded_calls(Kn) as seen:
        Kn.criss_cross_attention(qd.detach(), kd.detach(), vd.detach(), gm.detach(), res=rd, scale=sc).backward(gd)
        assert Kn.criss_cross_attention(qd.detach(), kd.detach(), vd.detach(), gm.detach(), res=rd.detach(), scale=sc).grad_fn is None
    assert CB not in seen and len(seen[CF]) == 2 and torch.equal(rd.grad, gd)
    # without res; only k and gamma need a gradient: dq and dv are not asked for
    kd.grad = gm.grad = None
    with recorded_calls(Kn) as seen:
        y = Kn.criss_cross_attention(qd.detach(), kd, vd.detach(), gm, scale=sc)
        y.backward(gd)
    a = seen[CB][0]
    assert seen[CF][0][6] is None and a[17] is None and a[21] is None and a[19] is not None and a[23] is not None
    w2, y2 = raw_fwd(q, k, v, None, ga, sc, False)
    got = raw_bwd(g, w2, q, k, v, ga, sc, False, ("dk", "dgamma"))
    assert B.bits_equal(map_of(y), y2) and B.bits_equal(map_of(kd.grad), got["dk"]) and B.bits_equal(gm.grad.cpu().numpy(), got["dgamma"])


def test_shapes_are_checked_before_any_call():
    from u2pl_amd import nn as Kn
    z = lambda *s: torch.zeros(*s, device=DEV)      # noqa: E731
    gm = z(1)
    with recorded_calls(Kn) as seen:
        for q, k, v, res in ((z(1, 6, 2, 2), z(1, 6, 2, 2), z(1, 8, 2, 2), None), (z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 6, 2, 2), None),
                             (z(1, 8, 2, 2), z(1, 8, 2, 3), z(1, 8, 2, 2), None), (z(1, 8, 2, 2), z(1, 4, 2, 2), z(1, 8, 2, 2), None),
                             (z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 4, 2, 2)), (z(2, 8, 2, 2), z(1, 8, 2, 2), z(1, 8, 2, 2), None),
                             (z(1, 4, 2, Kn.CC_MAX_L), z(1, 4, 2, Kn.CC_MAX_L), z(1, 4, 2, Kn.CC_MAX_L), None)):
            with pytest.raises(ValueError):
                Kn.criss_cross_attention(q, k, v, gm, res=res)
        with pytest.raises(ValueError, match="gamma"):
            Kn.criss_cross_attention(z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 8, 2, 2), z(2))
        with pytest.raises(ValueError, match="gamma"):
            Kn.criss_cross_attention(z(1, 8, 2, 2), z(1, 8, 2, 2), z(1, 8, 2, 2), torch.zeros(1))
    assert not seen


# ---- the decoder against its float64 twin -------------------------------------------------------------------------------------
def _cc_twin(dec, p, x):
    f = _seq64(dec.conva, p, "conva", x)
    for i in range(dec.recurrence):
        pre = "cca" if dec.shared else "cca.%d" % i
        q, k, v = (F.conv2d(f, p["%s.%s.weight" % (pre, n)], p["%s.%s.bias" % (pre, n)]).permute(0, 2, 3, 1) for n in ("query", "key", "value"))
        f = f + p[pre + ".gamma"] * B.mix(torch.softmax(B.dots(q, k), 3), v).permute(0, 3, 1, 2)
    out = _seq64(dec.bottleneck, p, "bottleneck", torch.cat((x, _seq64(dec.convb, p, "convb", f)), 1))
    return dict(pred=F.conv2d(out, p["classifier.weight"], p["classifier.bias"]), rep=_seq64(dec.representation, p, "representation", out))


# the key's bias adds q[p] . b to EVERY score of the pixel p, which the softmax does not see: its exact gradient is zero (the float64
# twin gives roundings of 1e-17)
KEY_BIAS_IS_ZERO = ((".key.bias",), lambda scale, wsum: scale <= 1e-12)


@pytest.mark.parametrize("shared", [True, False])
def test_ccnet_decoder_is_no_worse_than_the_deeplabv3_decoder(shared):
    from u2pl_amd.models.decoder import dec_ccnet

    def make():
        dec = dec_ccnet(in_planes=128, inner_planes=64, key_planes=32, recurrence=2, shared=shared, rep_head=True)
        with torch.no_grad():
            for i, b in enumerate([dec.cca] if shared else dec.cca):
                b.gamma.fill_(0.7 - 1.2 * i)             # the attention is live (the second block's gamma is negative)
        return dec
    pre = "cca." if shared else "cca.1."
    assert_no_worse_than_deeplabv3(
        "dec_ccnet", make, _cc_twin, ("pred", "rep"),
        {"pred", "rep", "dx", "conva.0.weight", pre + "query.weight", pre + "key.bias", pre + "value.weight", pre + "gamma", "convb.0.weight",
         "bottleneck.0.weight", "classifier.bias", "representation.4.weight"}, zero_grad=KEY_BIAS_IS_ZERO)


# ---- the whole path -----------------------------------------------------------------------------------------------------------
CC_DECODER = dict(type="u2pl.models.decoder.dec_ccnet", kwargs=dict(rep_head=True))


@pytest.fixture(scope="module")
def ccnet():
    return build_net(decoder_cfg(CC_DECODER)), net_input()


def test_ccnet_train_step_reaches_every_parameter_and_gamma_leaves_zero(ccnet):
    from u2pl_amd import nn as Kn
    model, x = ccnet
    model.train()
    gamma = model.decoder.cca.gamma
    assert float(gamma.detach()) == 0.0
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    opt.zero_grad(set_to_none=True)
    seen, outs = step_calls(model, x)
    assert sorted(outs) == ["aux", "pred", "rep"] and outs["pred"].shape == (4, 19, 9, 9)
    assert [len(seen[n_]) for n_ in (CF, CB)] == [2, 2]                        # recurrence = 2
    assert seen[CF][0][10:15] == (4, 9, 9, 64, 512) and all(a[6] is not None for a in seen[CF])
    # at gamma = 0 the gradients of q, k and v are exactly zero: what moves first is gamma
    assert gamma.grad is not None and gamma.grad.shape == (1,) and bool(torch.isfinite(gamma.grad).all()) and float(gamma.grad) != 0.0
    missing = [n_ for n_, p in model.named_parameters() if p.grad is None]
    assert not missing, missing
    assert not [n_ for n_, p in model.named_parameters() if not bool(torch.isfinite(p.grad).all())]
    opt.step()
    Kn.invalidate_weights()
    assert float(gamma.detach()) != 0.0                                         # after the first SGD step gamma has left 0
    opt.zero_grad(set_to_none=True)
    step_calls(model, x)                                                        # the attention is live now: every parameter moves
    bad = [n_ for n_, p in model.named_parameters() if not bool(torch.isfinite(p.grad).all())]
    zero = [n_ for n_, p in model.named_parameters() if not bool(p.grad.ne(0).any())]
    assert not bad and not zero, (bad, zero)
    opt.step()
    Kn.invalidate_weights()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_ccnet_eval_forward_is_the_same_with_and_without_a_graph(ccnet):
    assert_eval_forward_ignores_the_graph(ccnet)


def test_default_config_makes_no_cc_call_and_the_same_calls_after_a_ccnet_step(ccnet):
    assert_default_config_is_untouched(ccnet, CF, "u2pl_cc_")


def test_ccnet_graph_replay_is_bit_identical_to_eager(monkeypatch):
    """gamma starts at 0 and SGD moves it between the steps; it is read on the device: a host copy taken at capture time would
    replay the first step's value"""
    a, b = (train_steps(monkeypatch, on, lambda cfg: cfg["net"].update(decoder=CC_DECODER),
                        probe=lambda model: float(model.decoder.cca.gamma.detach())) for on in (True, False))
    print("graph stats", a["stats"], "gamma after each step", a["probes"])
    assert_replay_equals_eager(a, b)
    assert a["probes"][0] != 0.0 and len(set(a["probes"])) == len(a["probes"])      # gamma moves at every step
    assert a["probes"] == b["probes"]


# ---- prediction ----------------------------------------------------------------------------------------------------------------
def test_infer_image_refuses_a_map_past_the_largest_cross_and_runs_one_inside(ccnet):
    """at stride 8 a 9 x 4089 input is a 2 x 512 map, L = 513; 9 x 4081 is 2 x 511, L = 512 = CC_MAX_L"""
    from u2pl_amd import infer as I
    from u2pl_amd import nn as Kn
    model, _ = ccnet
    model.eval()
    try:
        lut = torch.from_numpy(I.normalise_lut([123.675, 116.28, 103.53], [58.395, 57.12, 57.375])).to(DEV)
        img = torch.randint(0, 256, (9, 64, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(DEV)
        with pytest.raises(ValueError, match="too large for one cross.*%d" % Kn.CC_MAX_L):
            I.infer_image(model, img, lut, (9, 4089))
        with recorded_calls(Kn) as seen:
            label, _, pred = I.infer_image(model, img, lut, (9, 4081))[:3]
        torch.cuda.synchronize()
        assert seen[CF][0][10:13] == (1, 2, 511) and CB not in seen
        assert label.shape == (9, 64) and bool(torch.isfinite(pred).all())
    finally:
        model.train()
